"""`robot.motion.retarget` on the GPU (pbhc_amd/motion_retarget.py, csrc/pbhc_retarget.hip) against the float64 model of
tests/retarget_model.py, which tests/test_motion_retarget_cpu.py holds to the oracle's FK and to its own closed-form gradient.

Fixture of the fits: targets by the model's FK from frames 1..40 of the shipped horse-stance clip on the 23-dof G1, 14 picks, joints from
0, the root from yaw only (frame 0 is left out and the conditioning asserted: `retarget_model.g1_fit_clips`).  Bounds come from the model
itself, never from the kernel:
  gradient    per element c * 2^-24 * (sum of the absolute values of the element's summands, from the model), c = 8 x the float32-CPU model's
              own worst ratio over the same cases.  The ratio is large (thousands): an element's error is set by |lever arm| * |error of the
              unit residual| — positions rounded to 1e-7 m over residuals of centimetres — not by its summands, which can be small where the
              hinge axis is nearly perpendicular to (lever arm x residual).  So a second bound is asserted beside it, with that error as a
              term of its own and c = 256: c * 2^-24 * sum |summands| + `retarget_model.input_error_terms` (worst-case rounding of positions,
              unit residuals and axes, reasoned there).  Both figures are in profiles/retarget.txt.
  trajectory  per quantity and iteration, 8 x the float32-CPU model's distance from the float64 model (floor 1e-6): 1e-6 to 2.5e-5 rad.
  convergence last loss <= 0.25 x first and <= 1.15 x the float64 model's last (the float32 model ends 1 % off the float64 model here)."""
import numpy as np
import pytest
import torch

from pbhc_amd import _lib
from pbhc_amd.motion_lib import MotionLib
from pbhc_amd.motion_retarget import Fitter, RetargetSettings, fit
from tests import retarget_model as rm
from tests.test_gpu_motion_ingest import run_build_one
from tests.test_gpu_motion_screen import clip, cut
from tests.test_motion_retarget_cpu import test_export_refusals as cpu_export_refusals

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATE = ("dof", "dof_sq", "dof_acc", "root_rot", "root_m", "root_v", "root_off", "off_m", "off_v")
_cache = {}


def settings_for(robot, **kw):
    sk = rm.skeleton(robot)
    kw.setdefault("limits", rm.limits_of(robot).tolist())
    return RetargetSettings(enable=True, joint_matches=[[sk.body_names_ext[b], l] for l, b in enumerate(rm.picks_of(robot))], **kw)


def fitter_for(robot, clips, **kw):
    """clips: list of dict(keypoints, trans, root_rot_init or root_rot[, dof, root_off]) -> a Fitter at that state"""
    sk = rm.skeleton(robot)
    cat = lambda k: np.concatenate([np.asarray(c[k], np.float32) for c in clips])
    f = Fitter(sk, settings_for(robot, **kw).to_c(sk), cat("keypoints"), cat("trans"), cat("root_rot_init" if "root_rot_init" in clips[0] else "root_rot"),
               [c["keypoints"].shape[0] for c in clips], DEV)
    if "dof" in clips[0]:
        f.dof.copy_(torch.from_numpy(cat("dof")))
        f.root_off.copy_(torch.from_numpy(np.stack([np.asarray(c["root_off"], np.float32) for c in clips])))
    return f


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().astype(np.float64)


def bits(t):
    torch.cuda.synchronize()
    return t.cpu().contiguous().view(torch.int32).numpy()


def split(a, fitter):
    return [a[fitter.starts[c]:fitter.starts[c + 1]] for c in range(fitter.M)]


def model_runs(dof_lr, iterations=10, limits=None):
    """the float64 and the float32 model on the 40-frame fixture, once per setting"""
    key = (dof_lr, iterations, None if limits is None else float(np.asarray(limits)[0, 1]))
    if key not in _cache:
        sk, picks, lim = rm.skeleton("g1"), rm.picks_of("g1"), rm.g1_limits() if limits is None else limits
        _cache[key] = tuple(rm.fit(sk, picks, rm.g1_fit_clips((40,)), lim, iterations, dof_lr=dof_lr, dtype=dt) for dt in (torch.float64, torch.float32))
    return _cache[key]


# ---- 1. FK consistency -----------------------------------------------------------------------------------------------------------------------
def test_body_positions_equal_the_build_kernels():
    sk = rm.skeleton("g1")
    dof, root, trans = (a.astype(np.float32) for a in rm.true_pose("g1", 40))
    f = fitter_for("g1", [dict(keypoints=rm.targets("g1", dof, root, trans), trans=trans, root_rot=root, dof=dof, root_off=np.zeros(3))])
    pos = host(f.loss_grad(body_pos=True)[4])
    pose = np.zeros((40, sk.num_bodies_ext, 3), np.float32)
    pose[:, 0], pose[:, 1:1 + sk.num_dof] = root, sk.dof_axis[None] * dof[:, :, None]
    D, Bx = sk.num_dof, sk.num_bodies_ext
    rows = host(run_build_one(sk, pose, trans, np.zeros((40, 2), np.float32), 30))
    want = rows[:, 2 * D + 2:2 * D + 2 + 3 * Bx].reshape(40, Bx, 3)
    err = np.abs(pos - want).max()
    print(f"retarget FK against pbhc_motion_build: max |dp| = {err:.3e} m")
    assert err <= (int(sk.depth.max()) + 2) * 1e-5


# ---- 2. gradient -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", rm.GRAD_FRAMES, ids=str)
@pytest.mark.parametrize("robot", ["arm", "biped", "g1"])
def test_gradient_against_the_float64_model(robot, frames):
    c = 8.0 * rm.float32_model_ratio()
    case = rm.grad_case(robot, frames)
    f = fitter_for(robot, case)
    loss, g_dof, g_rr, g_off, _ = f.loss_grad()
    loss, g_dof, g_rr, g_off = host(loss), split(host(g_dof), f), split(host(g_rr), f), host(g_off)
    worst = tight = 0.0
    for k, ref in enumerate(rm.grad_reference(case, robot)):
        assert ref["residual"].min() >= 0.01, "the evaluation point must keep every pick a centimetre from its target"
        worst = max(worst, rm.ratio(g_dof[k], ref["g_dof"], ref["abs_dof"]), rm.ratio(g_rr[k], ref["g_root_rot"], ref["abs_root_rot"]),
                    rm.ratio(g_off[k], ref["g_root_off"], ref["abs_root_off"]), rm.ratio(loss[k], ref["loss"], ref["abs_loss"]))
        tight = max(tight, rm.tight_ratio(g_dof[k], ref["g_dof"], ref["abs_dof"], ref["lev_dof"]),
                    rm.tight_ratio(g_rr[k], ref["g_root_rot"], ref["abs_root_rot"], ref["lev_root_rot"]),
                    rm.tight_ratio(g_off[k], ref["g_root_off"], ref["abs_root_off"], ref["lev_root_off"]),
                    rm.tight_ratio(loss[k], ref["loss"], ref["abs_loss"], ref["lev_loss"]))
    print(f"retarget gradient {robot} {frames}: kernel worst ratio {worst:.1f}, float32 model worst ratio over all cases {c / 8.0:.1f}, c = {c:.1f}; "
          f"share of the bound with the input-error term at c = 256: {tight:.4f}")
    assert worst <= c
    assert tight <= 1.0


def test_target_on_the_body_gives_zero_loss_and_gradient():
    dof, root, trans = (a.astype(np.float32) for a in rm.true_pose("biped", 5))
    base = dict(keypoints=rm.targets("biped", dof, root, trans), trans=trans, root_rot=root, dof=dof, root_off=np.float32([0.01, 0.0, -0.02]))
    pos = host(fitter_for("biped", [base]).loss_grad(body_pos=True)[4])
    # the kernel's own positions, bit for bit; the filter off, so that joints without a gradient stay where they are
    on = fitter_for("biped", [dict(base, keypoints=pos[:, rm.picks_of("biped")].astype(np.float32))], filter=False)
    for t in on.loss_grad()[:4]:
        assert not host(t).any()                                      # zero everywhere, no NaN
    hist = host(on.run(2))
    assert not hist.any() and np.array_equal(host(on.dof), dof.astype(np.float64)) and np.isfinite(host(on.root_rot)).all()


# ---- 3. trajectory ---------------------------------------------------------------------------------------------------------------------------
def assert_trajectory(f, hist, m64, m32, it, what):
    for name in ("dof", "root_rot", "root_off"):
        want, near = m64[name][it - 1][0], m32[name][it - 1][0]
        bound = max(8.0 * np.abs(near - want).max(), 1e-6)
        err = np.abs(host(getattr(f, name)).reshape(want.shape) - want).max()
        print(f"retarget trajectory {what} it {it} {name}: kernel {err:.3e}, float32 model {np.abs(near - want).max():.3e}, bound {bound:.3e}")
        assert err <= bound, (what, it, name)
    for k in range(it):
        want, near = m64["loss_history"][k, 0], m32["loss_history"][k, 0]
        assert abs(hist[k, 0] - want) <= max(8.0 * abs(near - want), 1e-6), (what, "loss", k)


@pytest.mark.parametrize("it", [1, 2, 3, 10])
@pytest.mark.parametrize("dof_lr", [100.0, 10.0])
def test_trajectory_against_the_float64_model(dof_lr, it):
    m64, m32 = model_runs(dof_lr)
    f = fitter_for("g1", rm.g1_fit_clips((40,)), dof_lr=dof_lr)
    hist = host(f.run(it))
    assert f.state.step == it
    assert_trajectory(f, hist, m64, m32, it, f"lr {dof_lr:g}")


# ---- 4. clip boundaries, batch invariance ------------------------------------------------------------------------------------------------------
def test_a_clip_alone_and_inside_a_batch_give_the_same_bits():
    clips = rm.g1_fit_clips((3, 1, 66))
    batch = fitter_for("g1", clips)
    hist = bits(batch.run(20))
    other = [dict(c) for c in clips]
    other[1] = dict(other[1], keypoints=other[1]["keypoints"] + np.float32(0.1))
    moved = fitter_for("g1", other)
    hist_moved = bits(moved.run(20))
    for k, c in enumerate(clips):
        alone = fitter_for("g1", [c])
        assert np.array_equal(bits(alone.run(20))[:, 0], hist[:, k]), k
        for name in STATE:
            rows = (lambda a, fit_: a[k:k + 1] if name in ("root_off", "off_m", "off_v") else split(a, fit_)[k])
            assert np.array_equal(bits(getattr(alone, name)), rows(bits(getattr(batch, name)), batch)), (k, name)
            if k != 1:                                                # a neighbour's targets changed: this clip's result did not
                assert np.array_equal(rows(bits(getattr(moved, name)), moved), rows(bits(getattr(batch, name)), batch)), (k, name)
    assert np.array_equal(hist_moved[:, [0, 2]], hist[:, [0, 2]]) and not np.array_equal(hist_moved[:, 1], hist[:, 1])
    assert np.isfinite(host(batch.dof)).all() and host(batch.dof).any()


# ---- 5. split run ------------------------------------------------------------------------------------------------------------------------------
def test_six_plus_four_iterations_equal_ten():
    clips = rm.g1_fit_clips((7, 40))
    whole, parts = fitter_for("g1", clips), fitter_for("g1", clips)
    h10 = bits(whole.run(10))
    h6, h4 = bits(parts.run(6)), bits(parts.run(4))
    assert whole.state.step == parts.state.step == 10
    assert np.array_equal(np.concatenate([h6, h4]), h10)
    for name in STATE:
        assert np.array_equal(bits(getattr(whole, name)), bits(getattr(parts, name))), name
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(whole.finish(), parts.finish()))


# ---- 6. clamp ----------------------------------------------------------------------------------------------------------------------------------
def test_tight_limits_hold_after_every_iteration():
    lim = np.tile([[-0.05, 0.05]], (23, 1))
    m64, m32 = model_runs(100.0, 5, lim)
    f = fitter_for("g1", rm.g1_fit_clips((40,)), limits=lim.tolist())
    lo, hi = np.float64(np.float32(-0.05)), np.float64(np.float32(0.05))
    hist = []
    for it in range(1, 6):
        hist.append(host(f.run(1)))
        dof = host(f.dof)
        assert dof.min() >= lo and dof.max() <= hi, it
        assert_trajectory(f, np.concatenate(hist), m64, m32, it, "limits 0.05")
    assert np.abs(host(f.dof)).max() >= hi - 1e-6, "the fixture was to drive some joint to its limit"
    pose, _, _ = f.finish()
    assert np.abs(host(pose)[:, 1:24]).max() <= hi


# ---- 7. convergence ----------------------------------------------------------------------------------------------------------------------------
def test_convergence_at_rate_ten():
    m64, _ = model_runs(10.0, 10)
    key = "conv64"
    if key not in _cache:
        _cache[key] = rm.fit(rm.skeleton("g1"), rm.picks_of("g1"), rm.g1_fit_clips((40,)), rm.g1_limits(), 300, dof_lr=10.0)["loss_history"][:, 0]
    want = _cache[key]
    f = fitter_for("g1", rm.g1_fit_clips((40,)), dof_lr=10.0)
    hist = host(f.run(300))[:, 0]
    print(f"retarget convergence: device {hist[0] * 1e3:.2f} -> {hist[-1] * 1e3:.3f} mm, float64 model {want[0] * 1e3:.2f} -> {want[-1] * 1e3:.3f} mm")
    assert abs(hist[0] - m64["loss_history"][0, 0]) <= 1e-6
    assert hist[-1] <= 0.25 * hist[0]
    assert hist[-1] <= 1.15 * want[-1]


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------------------------
def kp_clip():
    c = rm.g1_fit_clips((40,))[0]
    return dict(keypoints=c["keypoints"], root_trans_offset=c["trans"], fps=30)


def e2e_settings(**kw):
    return settings_for("g1", iterations=15, dof_lr=10.0, heading_from=list(rm.G1_HEADING), **kw)


def test_library_from_a_key_point_clip_and_an_ordinary_one():
    sk, ordinary = rm.skeleton("g1"), cut(clip("walk"), 10, 22)
    ml = MotionLib(sk, [kp_clip(), ordinary], 4, DEV, retarget=e2e_settings())
    batch, dof, quat, hist = fit([kp_clip()], sk, e2e_settings(), DEV)
    fitted = batch.to_host_clips()[0]
    assert fitted["pose_aa"].shape == (40, 27, 3) and "contact_mask" not in fitted and tuple(dof.shape) == (40, 23) and tuple(quat.shape) == (40, 4)
    assert np.array_equal(fitted["pose_aa"][:, 1:24], sk.dof_axis[None] * dof.cpu().numpy()[:, :, None]) and not fitted["pose_aa"][:, 24:].any()
    assert np.allclose(np.linalg.norm(quat.cpu().numpy(), axis=1), 1.0, atol=1e-6)
    want = MotionLib(sk, [fitted, ordinary], 4, DEV)
    assert ml.num_frames.tolist() == [40, 12] and torch.equal(ml.frames.view(torch.int32), want.frames.view(torch.int32))
    rep, h = ml.retarget_report, hist.cpu().numpy()
    assert rep["clips"].tolist() == [0] and rep["first_loss"][0] == h[0, 0] and rep["last_loss"][0] == h[-1, 0] and 0.0 < h[-1, 0] < h[0, 0]
    assert want.retarget_report is None
    # the stage off: the ordinary clip's rows are what they are without the key
    off, plain = MotionLib(sk, [ordinary], 4, DEV, retarget=RetargetSettings(enable=False)), MotionLib(sk, [ordinary], 4, DEV)
    assert off.retarget_report is None and torch.equal(off.frames.view(torch.int32), plain.frames.view(torch.int32))


def test_ground_option_puts_the_first_frame_on_the_floor():
    sk = rm.skeleton("g1")
    flat, _, _, _ = fit([kp_clip()], sk, e2e_settings(), DEV)
    down, _, _, _ = fit([kp_clip()], sk, e2e_settings(ground="first_frame_min_body"), DEV)
    assert torch.equal(flat.pose, down.pose) and torch.equal(flat.trans[:, :2], down.trans[:, :2])
    D, Bx = sk.num_dof, sk.num_bodies_ext
    c = down.to_host_clips()[0]
    rows = host(run_build_one(sk, c["pose_aa"], c["root_trans_offset"], np.zeros((40, 2), np.float32), 30))
    z = rows[:, 2 * D + 2:2 * D + 2 + 3 * Bx].reshape(40, Bx, 3)[0, :, 2]
    assert abs(z.min()) <= 1e-6 and float((flat.trans[:, 2] - down.trans[:, 2]).std()) <= 1e-6


# ---- 9. export refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["loss_grad", "fit", "finish"])
def test_export_refusals_leave_the_device_alone(which):
    sentinel = torch.full((64,), -77.0, device=DEV)
    cpu_export_refusals(which)
    torch.cuda.synchronize()
    assert bool((sentinel == -77.0).all())
    with pytest.raises(_lib.PbhcError, match="keypoints"):
        Fitter(rm.skeleton("arm"), settings_for("arm").to_c(rm.skeleton("arm")), np.zeros((4, 3, 3)), np.zeros((4, 3)), np.zeros((4, 3)), [4], DEV)


# ---- the command-line tool -----------------------------------------------------------------------------------------------------------------------
def test_tool_fits_a_key_point_file(tmp_path, capsys):
    import os

    from pbhc_amd.motion_lib import load_motion_file
    from pbhc_amd.utils.config import load_unresolved, save_unresolved, set_by_path
    from tools import retarget_motion

    c = rm.g1_fit_clips((40,))[0]
    names = [f"kp_{n}" for n in rm.G1_PICKS]
    order = list(reversed(range(14)))                                    # the file holds the key points in another order: matched by name
    np.savez(tmp_path / "kp.npz", **{"horse::keypoints": c["keypoints"][:, order], "horse::root_trans_offset": c["trans"], "horse::fps": np.int64(30),
                                     "horse::keypoint_names": np.array([names[i] for i in order])})
    cfg = load_unresolved(os.path.join(rm.GOLDEN, "configs", "v2_g1_23dof_student.yaml"))
    set_by_path(cfg, "robot.motion.retarget", dict(enable=False, joint_matches=[[n, "kp_" + n] for n in rm.G1_PICKS], iterations=15, dof_lr=10.0,
                                                   heading_from=list(rm.G1_HEADING)))
    save_unresolved(cfg, str(tmp_path / "cfg.yaml"))
    mjcf = os.path.join(rm.GOLDEN, "mjcf", "g1_23dof_lock_wrist_fitmotionONLY.xml")
    assert retarget_motion.main(["--config", str(tmp_path / "cfg.yaml"), "--in", str(tmp_path / "kp.npz"), "--out", str(tmp_path / "out.npz"), "--mjcf", mjcf]) == 0
    (name, got), = load_motion_file(str(tmp_path / "out.npz"))
    want = fit([dict(keypoints=c["keypoints"], root_trans_offset=c["trans"], fps=30)], rm.skeleton("g1"), e2e_settings(), DEV)[0].to_host_clips()[0]
    assert name == "horse" and got["fps"] == 30 and "contact_mask" not in got
    # (the tool's skeleton comes from the JSON tables, this test's from the MJCF: the same tables, bit for bit)
    assert np.array_equal(got["pose_aa"], want["pose_aa"]) and np.array_equal(got["root_trans_offset"], want["root_trans_offset"])
    assert "horse: mean key-point distance 56.6 mm" in capsys.readouterr().out
