"""`robot.motion.retarget` without a GPU: the float64 model the GPU tests compare with (tests/retarget_model.py) is itself held to the
oracle's FK and to its own closed-form gradient; the settings, the MJCF limits helper, the heading rule, the ingestion arithmetic and the
export refusals (which return before any launch) need no device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pbhc_amd import _lib, motion_ingest
from pbhc_amd.motion_retarget import UNLIMITED, RetargetSettings, heading_rotvec, mjcf_limits, prepare_targets
from pbhc_amd.skeleton import Skeleton
from tests import retarget_model as rm

GOLDEN = rm.GOLDEN
MATCHES = [[n, i] for i, n in enumerate(rm.G1_PICKS)]


def test_model_fk_equals_the_oracle_fk_on_a_shipped_clip():
    from oracle.fk import motion_fk

    sk = rm.skeleton("g1")
    z = np.load(os.path.join(GOLDEN, "clips", "Horse-stance_pose.npz"))
    pose, trans = z["clip0::pose_aa"][:60], z["clip0::root_trans_offset"][:60]
    want = motion_fk(dict(parents=sk.parents, offsets=sk.offsets, local_rot_wxyz=sk.local_rot_wxyz, num_bodies=sk.num_bodies), pose, trans, 1.0 / 30)["gts_t"]
    dof, root, tr = (a[:60] for a in rm.horse_pose())
    t = lambda a: torch.tensor(a)
    got, _ = rm.fk(sk, t(root), t(dof), t(tr))
    # the oracle runs in float32 down a chain of at most max depth + 2 links: the project's FK bound
    bound = (int(sk.depth.max()) + 2) * 1e-5
    assert float((got - want.double()).abs().max()) <= bound
    got32, _ = rm.fk(sk, t(root).float(), t(dof).float(), t(tr).float(), torch.float32)
    assert float((got32.double() - got).abs().max()) <= bound


@pytest.mark.parametrize("robot", ["arm", "biped", "g1"])
def test_closed_form_gradient_equals_autograd(robot):
    for frames in (1, 5, (3, 1, 6)):
        case = rm.grad_case(robot, frames)
        for ref, (L, gd, gr, go) in zip(rm.grad_reference(case, robot), rm.grad_reference(case, robot, torch.float64)):
            assert ref["residual"].min() >= 0.01
            assert abs(L - ref["loss"]) <= 1e-14
            for got, want in ((gd, ref["g_dof"]), (gr, ref["g_root_rot"]), (go, ref["g_root_off"])):
                assert np.abs(got - want).max() <= 1e-13
            # a hinge with no pick beyond it has no summands, and a zero gradient
            assert np.array_equal(ref["abs_dof"] == 0.0, ref["g_dof"] == 0.0)


def test_closed_form_gradient_near_the_zero_rotation():
    """J_l's series: a root rotation vector of 1e-6 rad"""
    case = rm.grad_case("arm", 2)
    for c in case:
        c["root_rot"] = np.full_like(c["root_rot"], 1e-6 / np.sqrt(3.0))
    for ref, (L, gd, gr, go) in zip(rm.grad_reference(case, "arm"), rm.grad_reference(case, "arm", torch.float64)):
        assert np.abs(gr - ref["g_root_rot"]).max() <= 1e-9          # (autograd divides by the 1e-6 norm: it is the less exact of the two)


def test_target_on_the_body_gives_no_gradient_and_no_nan():
    sk, picks = rm.skeleton("arm"), rm.picks_of("arm")
    dof, root, trans = rm.true_pose("arm", 3)
    kp = rm.targets("arm", dof, root, trans).astype(np.float64)
    pos, _ = rm.fk(sk, torch.tensor(root), torch.tensor(dof), torch.tensor(trans))
    ref = rm.analytic_grad(sk, picks, pos.numpy()[:, picks], trans, dof, root, np.zeros(3))
    assert ref["loss"] == 0.0 and not ref["g_dof"].any() and not ref["g_root_rot"].any() and not ref["g_root_off"].any()


@pytest.mark.parametrize("N", [1, 2, 3, 5, 7])
def test_filter_equals_a_hand_written_convolution(N):
    rng = np.random.default_rng(N)
    x = rng.standard_normal((N, 3))
    w = np.exp(-np.arange(-2, 3) ** 2 / (2 * 0.75 ** 2))
    w /= w.sum()
    want = np.zeros_like(x)
    for i in range(N):
        for k in range(-2, 3):
            want[i] += w[k + 2] * x[min(max(i + k, 0), N - 1)]
    assert np.abs(rm.filter5(torch.tensor(x), 0.75).numpy() - want).max() <= 1e-15
    assert np.allclose(rm.filter_weights(0.75).numpy(), w, rtol=0, atol=1e-15) and abs(w.sum() - 1.0) < 1e-15 and w[2] == w.max()
    assert N > 1 or np.allclose(want, x, atol=1e-15)                     # one frame: every tap is that frame


def test_settings_parse_and_defaults():
    assert RetargetSettings.from_config(None) is None
    s = RetargetSettings.from_config(dict(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 23, heading_from=list(rm.G1_HEADING)))
    assert (s.iterations, s.dof_lr, s.root_lr, s.filter, s.filter_sigma, s.ground) == (1000, 100.0, 0.01, True, 0.75, "none") and s.active
    sk = rm.skeleton("g1")
    assert s.picks(sk) == rm.picks_of("g1") and s.keypoint_columns(14) == list(range(14))
    p = s.to_c(sk)
    assert p.num_picks == 14 and list(p.pick)[:14] == rm.picks_of("g1") and p.filter_taps == 5 and abs(p.filter_sigma - 0.75) < 1e-7
    assert (p.rho, p.beta1, p.beta2) == tuple(np.float32(v) for v in (0.9, 0.9, 0.999)) and p.limits[22][0] == -1.0 and p.limits[22][1] == 1.0
    off = RetargetSettings.from_config(dict(enable=False))
    assert off is not None and not off.active
    named = RetargetSettings(enable=True, joint_matches=[["pelvis", "Pelvis"], ["head_link", "Head"]], limits=[[-1, 1]] * 23)
    assert named.keypoint_columns(3, ["Head", "x", "Pelvis"]) == [2, 0]
    g1 = RetargetSettings.from_config(dict(enable=True, joint_matches=MATCHES, filter=False), mjcf=os.path.join(GOLDEN, "mjcf", "g1_23dof_lock_wrist_fitmotionONLY.xml"))
    assert g1.to_c(sk).filter_taps == 0 and np.array_equal(g1.limits_array(sk), rm.g1_limits())


@pytest.mark.parametrize("node, text", [
    (dict(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 23, speed=1), "unknown key"),
    (dict(enable=True, limits=[[-1, 1]] * 23), "joint_matches is empty"),
    (dict(enable=True, joint_matches=MATCHES), "MJCF"),
    (dict(enable=True, joint_matches=MATCHES, limits="urdf"), "limits 'urdf'"),
    (dict(enable=True, joint_matches=MATCHES, limits=[[1, -1]] * 23), "lo <= hi"),
    (dict(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 23, iterations=-1), "iterations"),
    (dict(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 23, iterations=0), "iterations 0 must be an integer >= 1"),
    (dict(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 23, iterations=2.5), "iterations"),
    (dict(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 23, dof_lr=-1.0), "dof_lr"),
    (dict(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 23, filter_sigma=0.0), "filter_sigma"),
    (dict(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 23, ground="mesh"), "ground 'mesh'"),
    (dict(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 23, heading_from=["pelvis", "torso_link"]), "heading_from"),
    (dict(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 23, heading_from=["pelvis"]), "heading_from"),
    (dict(enable=True, joint_matches=[["pelvis", 0, 1]], limits=[[-1, 1]] * 23), "pair"),
    (dict(enable=True, joint_matches=[["pelvis", 0]] * 37, limits=[[-1, 1]] * 23), "at most"),
])
def test_settings_refusals(node, text):
    with pytest.raises(_lib.PbhcError, match=text):
        RetargetSettings.from_config(node)


def test_refusals_that_need_the_skeleton_or_the_clip():
    sk = rm.skeleton("g1")
    lim = [[-1, 1]] * 23
    with pytest.raises(_lib.PbhcError, match="'left_toe'"):
        RetargetSettings(enable=True, joint_matches=[["pelvis", 0], ["left_toe", 1]], limits=lim).picks(sk)
    with pytest.raises(_lib.PbhcError, match="23 dofs"):
        RetargetSettings(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 22).limits_array(sk)
    s = RetargetSettings(enable=True, joint_matches=MATCHES, limits=lim)
    with pytest.raises(_lib.PbhcError, match="outside"):
        s.keypoint_columns(13)
    with pytest.raises(_lib.PbhcError, match="'Head'"):
        RetargetSettings(enable=True, joint_matches=[["pelvis", "Head"]], limits=lim).keypoint_columns(3, ["a", "b", "c"])
    clip = dict(keypoints=np.zeros((4, 14, 3)), fps=30)
    with pytest.raises(_lib.PbhcError, match="heading_from is not set"):
        prepare_targets([clip], sk, s)
    with pytest.raises(_lib.PbhcError, match="no key point is matched to the root"):
        prepare_targets([clip], sk, RetargetSettings(enable=True, joint_matches=MATCHES[1:], limits=lim, heading_from=list(rm.G1_HEADING)))
    with pytest.raises(_lib.PbhcError, match="keypoints of shape"):
        prepare_targets([dict(keypoints=np.zeros((4, 14)), fps=30)], sk, s)


def test_prepare_targets_defaults():
    """no root_trans_offset: the key point matched to the root body; no root_rot_init: the heading rule"""
    sk = rm.skeleton("g1")
    fx = rm.g1_fit_clips((4, 2))
    s = RetargetSettings(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 23, heading_from=list(rm.G1_HEADING))
    kp, trans, rot, nframes, fps = prepare_targets([dict(keypoints=c["keypoints"], fps=30) for c in fx], sk, s)
    assert nframes == [4, 2] and fps == [30, 30] and kp.dtype == trans.dtype == rot.dtype == np.float32 and kp.shape == (6, 14, 3)
    assert np.array_equal(trans, kp[:, 0]) and np.array_equal(rot, np.concatenate([c["root_rot_init"] for c in fx]))
    shipped = prepare_targets([dict(keypoints=c["keypoints"], root_trans_offset=c["trans"], root_rot_init=c["root_rot_init"] * 2, fps=50) for c in fx], sk, s)
    assert np.array_equal(shipped[1], np.concatenate([c["trans"] for c in fx])) and np.array_equal(shipped[2], 2 * rot) and shipped[4] == [50, 50]


def test_mjcf_limits_helper():
    arm, biped, g1 = rm.skeleton("arm"), rm.skeleton("biped"), rm.skeleton("g1")
    # neither hand-written model gives a range: every hinge is unlimited
    assert np.array_equal(mjcf_limits(os.path.join(GOLDEN, "mjcf", "three_link_arm.xml"), arm), np.tile([[-UNLIMITED, UNLIMITED]], (3, 1)))
    assert np.array_equal(mjcf_limits(os.path.join(GOLDEN, "mini_biped.xml"), biped), np.tile([[-UNLIMITED, UNLIMITED]], (7, 1)))
    lim = rm.g1_limits()                                                 # <compiler angle="radian">
    assert lim.shape == (23, 2) and bool((lim[:, 0] < lim[:, 1]).all())
    names = ["left_hip_pitch", "left_hip_roll", "left_hip_yaw", "left_knee", "left_ankle_pitch", "left_ankle_roll"]
    want = [[-2.5307, 2.8798], [-0.5236, 2.9671], [-2.7576, 2.7576], [-0.087267, 2.8798], [-0.87267, 0.5236], [-0.2618, 0.2618]]
    assert [n + "_link" for n in names] == g1.body_names[1:7] and np.array_equal(lim[:6], np.asarray(want))
    assert np.array_equal(lim[[18, 22]], [[-1.0472, 2.0944]] * 2)      # the elbows, last dof of each arm
    with pytest.raises(_lib.PbhcError, match="3 dofs"):
        mjcf_limits(os.path.join(GOLDEN, "mini_biped.xml"), arm)


def test_mjcf_limits_in_degrees_and_unlimited(tmp_path):
    path = tmp_path / "deg.xml"
    path.write_text('<mujoco><worldbody><body name="a"><joint type="free"/><body name="b"><joint axis="0 0 1" range="-90 45"/>'
                    '<body name="c"><joint axis="0 1 0" range="-1 1" limited="false"/></body></body></body></worldbody></mujoco>')
    sk = Skeleton.from_mjcf(str(path))
    lim = mjcf_limits(str(path), sk)
    assert np.allclose(lim[0], [-np.pi / 2, np.pi / 4], rtol=0, atol=1e-15) and np.array_equal(lim[1], [-UNLIMITED, UNLIMITED])


def test_heading_rule():
    # the robot faces +x with its left side on +y: no yaw; turned a quarter to the left its left side is on -x
    left, right = np.array([[0.0, 0.1, 0.9], [-0.2, 0.0, 1.0], [0.1, 0.1, 0.3]]), np.array([[0.0, -0.1, 0.7], [0.2, 0.0, 1.0], [0.0, 0.0, 0.8]])
    got = heading_rotvec(left, right)
    assert np.array_equal(got[:, :2], np.zeros((3, 2))) and np.allclose(got[:, 2], [0.0, np.pi / 2, -np.pi / 4], rtol=0, atol=1e-15)
    # against the model: the +y axis of that yaw points from right to left on the ground plane
    y = rm.rotvec_matrix(torch.tensor(got[1:]))[:, :, 1].numpy()
    d = (left - right)[1:, :2]
    assert np.allclose(y[:, :2], d / np.linalg.norm(d, axis=1, keepdims=True), atol=1e-15) and np.allclose(y[:, 2], 0.0)
    with pytest.raises(_lib.PbhcError, match="coincide"):
        heading_rotvec(left, left + [0.0, 0.0, 0.3])


def test_ingestion_without_the_stage_leaves_a_library_unchanged():
    ordinary = [dict(pose_aa=np.zeros((3, 27, 3), np.float32), root_trans_offset=np.zeros((3, 3), np.float32), fps=30)]
    for settings in (None, RetargetSettings(enable=False), RetargetSettings.from_config(dict(enable=False, joint_matches=MATCHES))):
        out, report = motion_ingest.retarget(ordinary, rm.skeleton("g1"), "cpu", settings)
        assert out is ordinary and report is None
    # enabled, but no key-point clip in the library: still no launch, the same dicts, an empty report
    on = RetargetSettings(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 23)
    out, report = motion_ingest.retarget(ordinary, rm.skeleton("g1"), "cpu", on)
    assert out is ordinary and report["clips"].tolist() == [] and report["first_loss"].shape == (0,)


def test_ingestion_fits_only_the_key_point_clips(monkeypatch):
    """a mixed library: the key-point clips go to `fit` in order, as one batch; the ordinary ones pass through as the objects they are"""
    from pbhc_amd import motion_retarget

    ordinary = dict(pose_aa=np.zeros((3, 27, 3), np.float32), root_trans_offset=np.zeros((3, 3), np.float32), fps=30, contact_mask=np.ones((3, 2)))
    both = dict(ordinary, keypoints=np.zeros((3, 14, 3)))               # has a pose already: not fitted
    kp1, kp2 = dict(keypoints=np.zeros((2, 14, 3)), fps=30), dict(keypoints=np.ones((4, 14, 3)), fps=50)
    seen = {}

    def fake_fit(targets, skeleton, settings, device):
        seen["targets"] = targets
        nf = [t["keypoints"].shape[0] for t in targets]
        batch = motion_ingest.ClipBatch(torch.arange(sum(nf) * 27 * 3, dtype=torch.float32).reshape(-1, 27, 3), torch.ones(sum(nf), 3), None, nf,
                                        [t["fps"] for t in targets])
        return batch, None, None, torch.tensor([[0.05, 0.06], [0.03, 0.04], [0.01, 0.02]])

    monkeypatch.setattr(motion_retarget, "fit", fake_fit)
    on = RetargetSettings(enable=True, joint_matches=MATCHES, limits=[[-1, 1]] * 23)
    clips = [kp1, ordinary, both, kp2]
    out, report = motion_ingest.retarget(clips, rm.skeleton("g1"), "cpu", on)
    assert seen["targets"][0] is kp1 and seen["targets"][1] is kp2 and len(seen["targets"]) == 2
    assert out[1] is ordinary and out[2] is both and clips[0] is kp1 and "pose_aa" not in kp1
    assert [o["pose_aa"].shape[0] for o in out] == [2, 3, 3, 4] and out[3]["fps"] == 50 and "contact_mask" not in out[0] and "keypoints" not in out[0]
    assert out[3]["pose_aa"][0, 0, 0] == 2 * 27 * 3 and report["clips"].tolist() == [0, 3]
    assert np.allclose(report["first_loss"], [0.05, 0.06]) and np.allclose(report["last_loss"], [0.01, 0.02])
    assert motion_ingest.derive_flags(out, type("CD", (), dict(overwrite=False))()) == [True, False, False, True]


# ---- the exports' refusals: every one returns before any launch, so none needs a GPU -------------------------------------------------------
def _call(sk, p, total, starts, which="loss_grad"):
    lib, one = _lib.lib(), C.c_void_p(8)                                 # (non-NULL pointers that are never followed)
    st = np.asarray(starts, np.int32)
    sp = st.ctypes.data_as(C.c_void_p)
    csk = sk.to_c()
    if which == "loss_grad":
        return lib.pbhc_retarget_loss_grad(C.byref(csk), C.byref(p), one, one, one, one, one, total, len(st) - 1, sp, one, one, one, one, one, None, one, None)
    state = _lib.PbhcRetargetState()
    for name in ("dof", "dof_sq", "dof_acc", "root_rot", "root_m", "root_v", "root_off", "off_m", "off_v", "scratch"):
        setattr(state, name, 8)
    if which == "fit":
        return lib.pbhc_retarget_fit(C.byref(csk), C.byref(p), one, one, total, len(st) - 1, sp, one, C.byref(state), 3, one, None)
    return lib.pbhc_retarget_finish(C.byref(csk), C.byref(p), one, total, len(st) - 1, sp, one, C.byref(state), one, one, one, None)


def good_params(sk):
    return RetargetSettings(enable=True, joint_matches=[["link3", 0], ["base", 1]], limits=[[-1, 1]] * 3).to_c(sk)


@pytest.mark.parametrize("which", ["loss_grad", "fit", "finish"])
def test_export_refusals(which):
    sk, EINVAL = rm.skeleton("arm"), _lib.K["PBHC_EINVAL"]

    def refused(mutate, total=4, starts=(0, 3, 4), text=""):
        p = good_params(sk)
        mutate(p)
        assert _call(sk, p, total, starts, which) == EINVAL
        msg = _lib.lib().pbhc_last_error().decode()
        assert f"pbhc_retarget_{which}" in msg and text in msg, msg

    refused(lambda p: setattr(p, "num_picks", 0), text="num_picks 0")
    refused(lambda p: setattr(p, "num_picks", _lib.K["PBHC_MAX_BODIES"] + 1), text="num_picks 37")
    refused(lambda p: p.pick.__setitem__(1, 4), text="pick 1 is body 4")
    refused(lambda p: p.pick.__setitem__(0, -1), text="pick 0 is body -1")
    refused(lambda p: setattr(p, "filter_taps", 3), text="filter_taps 3")
    refused(lambda p: p.limits[2].__setitem__(0, 2.0), text="limits of dof 2")
    refused(lambda p: None, total=5, text="total 5 is not starts[2] = 4")
    refused(lambda p: None, starts=(0, 2, 2, 4), text="clip 1 has 0 frames")
    refused(lambda p: None, starts=(1, 3, 4), text="starts[0] 1")
    assert _lib.PbhcRetargetParams.pick.size == 4 * _lib.K["PBHC_MAX_BODIES"] and _lib.lib().pbhc_sizeof_retarget_params() == C.sizeof(_lib.PbhcRetargetParams)
