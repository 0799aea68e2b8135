"""`robot.motion.augmentation` on the GPU: the one-launch kernel (`pbhc_motion_augment_batch`, csrc/pbhc_motion_augment.hip) against the float64
restatement of tests/test_motion_augment_cpu.py, then the library built on it.

Bounds.  What the kernel copies or permutes — variant 0, the mirror at speed 1, the frames a speed hits exactly — is compared with `==`
(a mirrored zero is -0.0, so not by bit pattern).  An interpolated translation or joint value a + t (b - a) is formed in double on both
sides without a fused multiply-add and rounded once: 2 float32 ulp of the larger neighbour allows for one differing rounding on each side
(none was seen).  The root rotation vector goes through sin / cos / atan2 of two different maths libraries: 1e-6, the bound the extension's
root row is held to.  Positions from the tables: (max chain depth + 2) x the skeleton's offset asymmetry, as on the CPU.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from pbhc_amd import _lib
from pbhc_amd.motion_augment import Augmentation, mirror_tables
from pbhc_amd.motion_interp import Interpolation
from pbhc_amd.motion_lib import MotionLib
from tests.helpers import fixture_config
from tests.test_gpu_motion_interp import run_export as run_extend
from tests.test_motion_augment_cpu import CLIP29, cut, frames_at_speed, load_clip, restate, skeleton, walk_with_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77.0
SPEEDS = [0.5, 2.0, 1.3]
ROOT_TOL = 1e-6


def run_augment(sk, clips, aug, perm):
    """clips: clip dicts -> per OUTPUT clip (pose_aa, trans, contact or None) from ONE launch.  The outputs are pre-filled with a sentinel,
    3 frames more than needed: every frame must be written and nothing behind them."""
    Bx = sk.num_bodies_ext
    with_contact = all("contact_mask" in c for c in clips)
    nf = [np.asarray(c["pose_aa"]).shape[0] for c in clips]
    out_n = [frames_at_speed(F, aug.variant(v)[1]) for F in nf for v in range(aug.num_variants)]
    in_start = np.concatenate([[0], np.cumsum(nf)]).astype(np.int32)
    out_start = np.concatenate([[0], np.cumsum(out_n)]).astype(np.int32)
    tin, tout = int(in_start[-1]), int(out_start[-1])
    up = lambda key: torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(c[key], np.float32) for c in clips]))).to(DEV)
    d_pose, d_trans = up("pose_aa"), up("root_trans_offset")
    d_contact = up("contact_mask") if with_contact else None
    assert d_pose.shape[1] == Bx
    o_pose = torch.full((tout + 3, Bx, 3), SENTINEL, device=DEV)
    o_trans = torch.full((tout + 3, 3), SENTINEL, device=DEV)
    o_contact = torch.full((tout + 3, 2), SENTINEL, device=DEV) if with_contact else None
    d_perm = torch.from_numpy(np.asarray(perm, np.int32)).to(DEV) if aug.mirror else None
    d_in, d_out = torch.from_numpy(in_start).to(DEV), torch.from_numpy(out_start).to(DEV)
    csk = sk.to_c()
    _lib.check(_lib.lib().pbhc_motion_augment_batch(C.byref(csk), _lib.ptr(d_pose), _lib.ptr(d_trans), _lib.ptr(d_contact), tin, len(clips), _lib.ptr(d_in),
                                                    _lib.ptr(d_out), tout, aug.to_c(), _lib.ptr(d_perm), _lib.ptr(o_pose), _lib.ptr(o_trans),
                                                    _lib.ptr(o_contact), _lib.current_stream()), "pbhc_motion_augment_batch")
    torch.cuda.synchronize()
    for o in (o_pose, o_trans) + ((o_contact,) if with_contact else ()):
        assert bool((o[tout:] == SENTINEL).all()), "the launch wrote behind its output"
        assert not bool((o[:tout] == SENTINEL).any()), "the launch left output frames unwritten"
    o_pose, o_trans = o_pose.cpu().numpy(), o_trans.cpu().numpy()
    o_contact = o_contact.cpu().numpy() if with_contact else None
    return [(o_pose[a:b], o_trans[a:b], None if o_contact is None else o_contact[a:b]) for a, b in zip(out_start[:-1], out_start[1:])]


def arrays(clip):
    return (np.asarray(clip["pose_aa"], np.float32), np.asarray(clip["root_trans_offset"], np.float32),
            np.asarray(clip["contact_mask"], np.float32) if "contact_mask" in clip else None)


def neighbour_ulp(src, speed, Fo, perm, mirrored, what):
    """2 float32 ulp of the larger of the two source values every output element was interpolated from"""
    F = src.shape[0]
    x = np.arange(Fo) * float(speed)
    i0 = np.minimum(np.floor(x).astype(np.int64), F - 1)
    i1 = np.minimum(i0 + 1, F - 1)
    big = np.maximum(np.abs(src[i0]), np.abs(src[i1]))
    if mirrored and what == "pose":
        big = big[:, perm]
    return 2.0 * np.spacing(big.astype(np.float32)).astype(np.float64)


def check_batch(sk, clips):
    perm = mirror_tables(sk, 1e-4).body_perm
    aug = Augmentation(mirror=True, speeds=SPEEDS)
    V = aug.num_variants
    assert V == 8
    got = run_augment(sk, clips, aug, perm)
    assert len(got) == len(clips) * V
    worst = dict(lin=0.0, root=0.0)
    for ci, clip in enumerate(clips):
        pose, trans, contact = arrays(clip)
        F = pose.shape[0]
        for v in range(V):
            mirrored, speed = aug.variant(v)
            g = got[ci * V + v]
            what = f"clip {ci} variant {v} (mirror {mirrored}, speed {speed})"
            Fo = frames_at_speed(F, speed)
            assert g[0].shape[0] == Fo and g[1].shape[0] == Fo, (what, "frame count")                       # 1. the host formula
            want = restate(clip, mirrored, speed, perm)
            if speed == 1.0:                                                                                 # 2. and 3.: exact
                for a, b in zip(g, (pose, trans, contact) if not mirrored else want):
                    assert (a is None and b is None) or np.all(a == b), (what, "not a copy / a permutation and sign flip")
                continue
            if not mirrored:                                                                                 # 4. the frames a speed hits exactly
                hit = dict(pose=pose, trans=trans, contact=contact)
                for name, a in zip(("pose", "trans", "contact"), g):
                    if a is None:
                        continue
                    if speed == 2.0:
                        assert np.all(a == hit[name][::2]), (what, name, "frame k is not source frame 2 k")
                    if speed == 0.5:
                        assert np.all(a[::2] == hit[name]), (what, name, "even frames are not the source frames")
            # 5. everything against the restatement
            if contact is not None:
                # the nearer frame's mask, never a blend: no value the source does not hold (the horse stance's own mask has 0.5 entries)
                assert np.all(g[2] == want[2]) and set(np.unique(g[2])) <= set(np.unique(contact)), (what, "contact mask")
            d_pose = np.abs(g[0].astype(np.float64) - want[0].astype(np.float64))
            d_trans = np.abs(g[1].astype(np.float64) - want[1].astype(np.float64))
            tol_pose = neighbour_ulp(pose, speed, Fo, perm, mirrored, "pose")
            tol_trans = neighbour_ulp(trans, speed, Fo, perm, mirrored, "trans")
            assert np.all(d_pose[:, 1:] <= tol_pose[:, 1:]), (what, "joint rows", float((d_pose[:, 1:] - tol_pose[:, 1:]).max()))
            assert np.all(d_trans <= tol_trans), (what, "translation", float((d_trans - tol_trans).max()))
            assert d_pose[:, 0].max() <= ROOT_TOL, (what, "root rotation vector", float(d_pose[:, 0].max()))
            worst["lin"] = max(worst["lin"], float(d_pose[:, 1:].max()), float(d_trans.max()))
            worst["root"] = max(worst["root"], float(d_pose[:, 0].max()))
    print(f"max |kernel - restatement|: joint rows / translation {worst['lin']:.3e}, root rotation vector {worst['root']:.3e} (bound {ROOT_TOL:.0e})")
    # 6. the mirror of the mirror is the source
    only = Augmentation(mirror=True)
    once = run_augment(sk, clips, only, perm)
    mirrored_clips = []
    for ci, clip in enumerate(clips):
        p, t, c = once[2 * ci + 1]
        m = dict(pose_aa=p, root_trans_offset=t, fps=clip["fps"])
        if c is not None:
            m["contact_mask"] = c
        mirrored_clips.append(m)
    twice = run_augment(sk, mirrored_clips, only, perm)
    for ci, clip in enumerate(clips):
        for a, b in zip(twice[2 * ci + 1], arrays(clip)):
            assert (a is None and b is None) or np.all(a == b), (ci, "mirroring twice does not give the source back")


def test_kernel_23dof_batch_matches_the_restatement():
    """walk (122 frames, a synthetic alternating mask) and horse stance [20:60] with its own mask, 27 bodies, one launch of 16 output clips"""
    horse = cut(load_clip("Horse-stance_pose.npz"), 20, 60)
    assert "contact_mask" in horse and horse["pose_aa"].shape == (40, 27, 3)
    check_batch(skeleton("g1_23dof"), [walk_with_mask(), horse])


def test_kernel_29dof_clip_without_a_mask_matches_the_restatement():
    """33 bodies (99 floats per frame: the lanes' second round is partial), NULL contact in and out"""
    clip = cut(load_clip(CLIP29), 0, 40)
    assert "contact_mask" not in clip and clip["pose_aa"].shape == (40, 33, 3)
    check_batch(skeleton("g1_29dof"), [clip])


def test_inconsistent_start_arrays_leave_the_output_unwritten():
    """the kernel's guard: an out_start that gives a variant another frame count than the formula indexes nothing"""
    sk = skeleton("g1_23dof")
    clip = cut(load_clip("g1_walk_45cms_23dof.npz"), 0, 24)
    aug = Augmentation(speeds=[2.0])                                            # 24 + 12 frames
    d_pose = torch.from_numpy(np.ascontiguousarray(clip["pose_aa"])).to(DEV)
    d_trans = torch.from_numpy(np.ascontiguousarray(clip["root_trans_offset"])).to(DEV)
    o_pose, o_trans = torch.full((36, 27, 3), SENTINEL, device=DEV), torch.full((36, 3), SENTINEL, device=DEV)
    d_in = torch.tensor([0, 24], dtype=torch.int32, device=DEV)
    d_out = torch.tensor([0, 25, 36], dtype=torch.int32, device=DEV)            # 25 + 11: the total is right, both clips are wrong
    csk = sk.to_c()
    _lib.check(_lib.lib().pbhc_motion_augment_batch(C.byref(csk), _lib.ptr(d_pose), _lib.ptr(d_trans), None, 24, 1, _lib.ptr(d_in), _lib.ptr(d_out), 36,
                                                    aug.to_c(), None, _lib.ptr(o_pose), _lib.ptr(o_trans), None, _lib.current_stream()), "pbhc_motion_augment_batch")
    torch.cuda.synchronize()
    assert bool((o_pose == SENTINEL).all()) and bool((o_trans == SENTINEL).all())


# ---- the library -----------------------------------------------------------------------------------------------------------------------
CFG = "v2_g1_23dof_student.yaml"
N = 16


def _lib_clips():
    """two source clips of different lengths, both with a contact mask"""
    return [walk_with_mask(), cut(load_clip("Horse-stance_pose.npz"), 20, 60)]


@pytest.fixture(scope="module")
def libs():
    sk = skeleton("g1_23dof")
    aug = Augmentation.from_config(fixture_config(CFG, N, {"robot.motion.augmentation": {"mirror": True, "speeds": [0.8, 1.25]}}).robot.motion.augmentation)
    return sk, aug, MotionLib(sk, _lib_clips(), N, DEV), MotionLib(sk, _lib_clips(), N, DEV, augmentation=aug)


def test_library_holds_every_variant_as_an_ordinary_clip(libs):
    sk, aug, plain, ml = libs
    V = aug.num_variants
    assert V == 6 and ml._num_unique_motions == 2 * V and plain._num_unique_motions == 2 and plain.augmentation is None
    want_frames = [frames_at_speed(F, aug.variant(v)[1]) for F in (122, 40) for v in range(V)]
    assert ml.num_frames.tolist() == want_frames and ml.table.num_motions == 2 * V
    assert ml.length_starts.tolist() == np.concatenate([[0], np.cumsum(want_frames)])[:-1].tolist()
    assert torch.allclose(ml._motion_lengths.cpu(), torch.tensor([(F - 1) / 30.0 for F in want_frames]), atol=1e-6)
    assert ml.variant_source.device.type == "cuda" and ml.variant_source.dtype == torch.int64
    assert ml.variant_source.tolist() == [0] * V + [1] * V and plain.variant_source.tolist() == [0, 1]
    assert ml.variant_info == [(s, m, sp) for s in (0, 1) for sp in (1.0, 0.8, 1.25) for m in (False, True)]
    assert plain.variant_info == [(0, False, 1.0), (1, False, 1.0)] and plain.mirror_body_perm is None
    mt = mirror_tables(sk, 1e-4)
    assert ml.mirror_body_perm.tolist() == mt.body_perm.tolist() and ml.mirror_dof_perm.tolist() == mt.dof_perm.tolist()
    assert ml.mirror_dof_sign.tolist() == mt.dof_sign.tolist()
    for t in (ml._sampling_prob, ml._termination_history, ml._success_rate, ml._sampling_history):
        assert t.shape == (2 * V,)
    ids = ml.load_motions(random_sample=False)
    assert ids.tolist() == [i % (2 * V) for i in range(N)]
    # the rows of every variant 0 are those of a library built without the key, byte for byte
    for src in (0, 1):
        a, F = int(ml.length_starts[src * V]), int(ml.num_frames[src * V])
        b = int(plain.length_starts[src])
        assert F == int(plain.num_frames[src])
        assert torch.equal(ml.frames[a:a + F].view(torch.int32), plain.frames[b:b + F].view(torch.int32)), src
    # mirror off and no speed: the key absent
    off = MotionLib(sk, _lib_clips(), N, DEV, augmentation=Augmentation.from_config({"mirror": False, "speeds": []}))
    assert off.augmentation is None and torch.equal(off.frames.view(torch.int32), plain.frames.view(torch.int32))


def test_motion_state_of_a_mirrored_variant_is_the_mirrored_state(libs):
    sk, aug, plain, ml = libs
    mt = mirror_tables(sk, 1e-4)
    ml.load_motions(random_sample=False)                                        # slot i holds clip i: slot 0 the walk, slot 1 its mirror image
    assert ml.variant_info[1] == (0, True, 1.0)
    times = torch.tensor([0.0, 1.0, 1.0 + 0.37 / 30.0], device=DEV)           # frame 0, frame 30, strictly between frames 30 and 31
    src = ml.get_motion_state(torch.zeros(3, dtype=torch.long, device=DEV), times)
    mir = ml.get_motion_state(torch.ones(3, dtype=torch.long, device=DEV), times)
    perm_d, sign = torch.from_numpy(mt.dof_perm).to(DEV), torch.from_numpy(mt.dof_sign).to(DEV)
    assert torch.equal(mir["dof_pos"], src["dof_pos"][:, perm_d] * sign), "dof_pos: permuted and signed exactly"
    assert torch.equal(mir["contact_mask"], src["contact_mask"].flip(1)), "contact mask: swapped"
    perm_b = torch.from_numpy(mt.body_perm).to(DEV)
    want = src["rg_pos_t"][:, perm_b] * torch.tensor([1.0, -1.0, 1.0], device=DEV)
    err = float((mir["rg_pos_t"].double() - want.double()).abs().max())
    bound = (int(sk.depth.max()) + 2) * mt.asymmetry
    print(f"max |state(mirror) - mirror(state)| body position {err:.3e} m, bound {bound:.3e} m")
    assert err <= bound
    assert float((mir["rg_pos_t"][:, :, 1] + src["rg_pos_t"][:, :, 1]).abs().max()) > 0.05     # a mirror, not a copy: left and right differ


def test_augmentation_then_interpolation_is_the_extension_of_the_variants():
    sk = skeleton("g1_23dof")
    rc = fixture_config(CFG, N).robot
    ip = Interpolation.from_config({"start_frames": 3, "end_frames": 2}, sk.num_dof, robot=rc)
    aug = Augmentation(mirror=True, speeds=[1.25])
    clips = _lib_clips()
    ml = MotionLib(sk, clips, N, DEV, interpolation=ip, augmentation=aug)
    variants = run_augment(sk, clips, aug, mirror_tables(sk, 1e-4).body_perm)
    want = run_extend(sk, variants, 3, 2, False, ip.default_pose, contact_fill=ip.contact)
    got = ml.extended_clips()
    assert len(got) == len(want) == 8 and ml.num_frames.tolist() == [frames_at_speed(F, sp) + 5 for F in (122, 40) for sp in (1.0, 1.0, 1.25, 1.25)]
    for g, w in zip(got, want):                                                 # lead-in / lead-out frames at full length on every variant
        assert np.all(g["pose_aa"] == w[0]) and np.all(g["root_trans_offset"] == w[1]) and np.all(g["contact_mask"] == w[2]) and g["fps"] == 30
    ref = MotionLib(sk, got, N, DEV)                                            # and the tables are those of these clips
    assert torch.equal(ml.frames.view(torch.int32), ref.frames.view(torch.int32)) and ml.num_frames.tolist() == ref.num_frames.tolist()


def test_max_len_crops_are_drawn_from_the_variants():
    sk = skeleton("g1_23dof")
    aug = Augmentation(mirror=True, speeds=[2.0])
    K = 48
    ml = MotionLib(sk, [walk_with_mask()], 4, DEV, max_len=K, augmentation=aug)
    ref = MotionLib(sk, ml.extended_clips(), 4, DEV, max_len=K)
    starts = torch.tensor([0, 70, 5, 13])                                       # slot i holds variant i: 122, 122, 61, 61 frames
    for m in (ml, ref):
        m.load_motions(random_sample=False, max_len=K, crop_starts=starts)
    assert ml.max_len == K and ml.num_frames.tolist() == [K] * 4 and len(ml._raw) == 4
    assert torch.equal(ml.frames.view(torch.int32), ref.frames.view(torch.int32))


def test_target_heading_is_refused_with_the_mirror_and_works_with_speeds_alone():
    sk = skeleton("g1_23dof")
    heading = np.array([0.0, 0.0, np.sin(0.55), np.cos(0.55)])
    ml = MotionLib(sk, _lib_clips(), N, DEV, augmentation=Augmentation(mirror=True))
    with pytest.raises(_lib.PbhcError, match=r"target_heading.*robot\.motion\.augmentation\.mirror"):
        ml.load_motions(random_sample=False, target_heading=heading)
    from pbhc_amd.motion_lib import rebase_heading

    aug = Augmentation(speeds=[1.25])
    sp = MotionLib(sk, _lib_clips(), N, DEV, augmentation=aug)
    ptr = sp.frames.data_ptr()
    sp.load_motions(random_sample=False, target_heading=heading)
    ref = MotionLib(sk, [rebase_heading(c, heading) for c in _lib_clips()], N, DEV, augmentation=aug)
    assert sp.frames.data_ptr() == ptr and torch.equal(sp.frames.view(torch.int32), ref.frames.view(torch.int32))


def test_env_is_built_on_the_variants():
    from tests.helpers import build_hip_env

    cfg, env = build_hip_env(CFG, N, general=True, overrides={"robot.motion.augmentation": {"mirror": True, "speeds": [0.8]}})
    ml = env._motion_lib
    F = int(load_clip("g1_ue_walk_23dof.npz")["pose_aa"].shape[0])
    assert ml._num_unique_motions == 4 and ml.num_frames.tolist() == [F, F, frames_at_speed(F, 0.8), frames_at_speed(F, 0.8)]
    env.reset_all()
    for _ in range(2):
        obs, rew, reset, _ = env.step({"actions": torch.zeros(N, env.num_dof, device=DEV)})
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in obs.values()) and torch.isfinite(rew).all()
    assert env.clip_of_env(0)["pose_aa"].shape[0] == int(ml.num_frames[int(ml.slot_clip[0])])
