"""`robot.motion.contact_detection` / `robot.motion.screening` on the GPU: the two launches of the pre-pass (`pbhc_motion_screen_frames`,
`pbhc_motion_screen_clips`, csrc/pbhc_motion_screen.hip) against the float64 restatement of tests/test_motion_screen_cpu.py and the
reference's recorded outputs (tests/golden/motion_screen.npz), then everything built on them: MotionLib, tables, crops, variants, an env.

Bounds.
Contact masks: equal element for element, except inside a narrow band of the restatement, |dp^2 - vel_threshold| < 3e-6 or
|z - height_threshold| < 1e-5, and at most 1 % of a clip's elements there.  The build kernel's FK matches the reference's to 2–3e-6 in
position, so dp^2 at the threshold (|dp| = sqrt(0.002)) is off by at most 2 sqrt(0.002) 2 x 3e-6 = 5.4e-7; the band is about five times that.
With the oracle's FK no element of the 23-dof clips is in the band (closest 1.2e-5 / 2.5e-4): their masks must be equal everywhere.
Distances: |d - restatement| <= 1e-4 max(1, largest |coordinate| of the frame): positions good to 3e-6 make a weight exp(-10 z) good to 3e-5
relative, which moves a weighted mean of points about 1 m apart by at most 3e-5; the centre-of-mass term adds less than 1e-6.  That is below
the closest approach of any shipped clip's distance to epsilon_stab (4.5e-4 on the 29-dof clip, 1.6e-3 on the horse stance), so verdicts
must be equal.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pbhc_amd import _lib, motion_screen
from pbhc_amd.motion_augment import Augmentation
from pbhc_amd.motion_interp import Interpolation
from pbhc_amd.motion_lib import MotionLib, load_motion_file
from pbhc_amd.motion_screen import ContactDetection, Screening
from pbhc_amd.skeleton import Skeleton
from tests.helpers import GOLDEN, build_hip_env, fixture_config
from tests.test_motion_screen_cpu import (CLIP_FILES, SKELETON_JSON, fixture, restate_contact, restate_distance, restate_fk, restate_verdict, skeleton_mjcf,
                                          verdict_cases)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77.0
VEL_BAND, HEIGHT_BAND, BAND_SHARE = 3e-6, 1e-5, 0.01
_clips = {}


def clip(name):
    if name not in _clips:
        c = dict(load_motion_file(os.path.join(GOLDEN, "clips", CLIP_FILES[name]))[0][1])
        c["pose_aa"], c["root_trans_offset"] = np.asarray(c["pose_aa"], np.float32), np.asarray(c["root_trans_offset"], np.float32)
        _clips[name] = c
    return _clips[name]


def cut(c, a, b):
    return {k: (np.asarray(v)[a:b] if k in ("pose_aa", "root_trans_offset", "contact_mask") else v) for k, v in c.items()}


def skeleton_json(robot):
    return Skeleton.from_json(os.path.join(GOLDEN, SKELETON_JSON[robot]))


def params_of(sk, cd=None, sc=None):
    return motion_screen.to_c(cd, sc, sk)


def up(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def run_frames(sk, clips, params, contact=True, stability=True):
    """ONE call of pbhc_motion_screen_frames on the clips concatenated -> (starts, foot_pos [total,2,3] or None, dist [total] or None) on the
    host; every output has sentinel rows behind it that must stay untouched, and every row in front of them must be written"""
    Bx = sk.num_bodies_ext
    nf = [c["pose_aa"].shape[0] for c in clips]
    starts = np.concatenate([[0], np.cumsum(nf)]).astype(np.int32)
    total, M = int(starts[-1]), len(clips)
    d_pose = up(np.concatenate([c["pose_aa"][:, :Bx] for c in clips]))
    d_trans = up(np.concatenate([c["root_trans_offset"] for c in clips]))
    d_start = up(starts, np.int32)
    foot = torch.full((total + 3, 2, 3), SENTINEL, device=DEV) if contact else None
    dist = torch.full((total + 3,), SENTINEL, device=DEV) if stability else None
    ground = torch.full((M + 3,), SENTINEL, device=DEV) if stability else None
    d_mass = up(sk.body_mass) if stability else None
    d_com = up(sk.body_com) if stability else None
    csk = sk.to_c()
    _lib.check(_lib.lib().pbhc_motion_screen_frames(C.byref(csk), _lib.ptr(d_pose), _lib.ptr(d_trans), total, M, _lib.ptr(d_start), params, _lib.ptr(d_mass),
                                                    _lib.ptr(d_com), _lib.ptr(ground), _lib.ptr(foot), _lib.ptr(dist), _lib.current_stream()),
               "pbhc_motion_screen_frames")
    torch.cuda.synchronize()
    for o, n in ((foot, total), (dist, total), (ground, M)):
        if o is not None:
            assert bool((o[n:] == SENTINEL).all()), "the launch wrote behind its output"
            assert not bool((o[:n] == SENTINEL).any()), "the launch left rows unwritten"
    return starts, None if foot is None else foot[:total].cpu().numpy(), None if dist is None else dist[:total].cpu().numpy()


def run_clips(starts, params, foot_pos=None, dist=None, derive=None):
    """ONE call of pbhc_motion_screen_clips -> (mask [total,2] or None, report [M,8] or None) on the host, sentinels checked as above; mask rows
    of clips with derive == 0 must come back as the sentinel"""
    starts = np.asarray(starts, np.int32)
    total, M = int(starts[-1]), len(starts) - 1
    derive = np.ones(M, np.int32) if derive is None else np.asarray(derive, np.int32)
    d_foot = None if foot_pos is None else up(foot_pos)
    d_dist = None if dist is None else up(dist)
    mask = torch.full((total + 3, 2), SENTINEL, device=DEV) if foot_pos is not None else None
    report = torch.full((M + 2, _lib.K["PBHC_SCREEN_REPORT"]), SENTINEL, device=DEV) if dist is not None else None
    d_start, d_derive = up(starts, np.int32), up(derive, np.int32)        # (named: a temporary's memory is handed out again at once)
    _lib.check(_lib.lib().pbhc_motion_screen_clips(_lib.ptr(d_foot), _lib.ptr(d_dist), total, M, _lib.ptr(d_start), _lib.ptr(d_derive),
                                                   params, _lib.ptr(mask), _lib.ptr(report), _lib.current_stream()), "pbhc_motion_screen_clips")
    torch.cuda.synchronize()
    if mask is not None:
        assert bool((mask[total:] == SENTINEL).all()), "the launch wrote behind the mask"
        mask = mask[:total].cpu().numpy()
        for c in range(M):
            rows = mask[starts[c]:starts[c + 1]]
            assert (rows != SENTINEL).all() if derive[c] else (rows == SENTINEL).all(), (c, "derive flag not honoured")
    if report is not None:
        assert bool((report[M:] == SENTINEL).all()) and not bool((report[:M] == SENTINEL).any())
        report = report[:M].cpu().numpy()
    return mask, report


def assert_mask(got, foot_pos64, what, want=None, band_allowed=True):
    """got [F,2] against the restatement of foot_pos64 (and against `want`, the reference's recorded mask), element for element outside the band"""
    mask, dp2, z = restate_contact(foot_pos64)
    band = (np.abs(dp2 - 0.002) < VEL_BAND) | (np.abs(z - 0.12) < HEIGHT_BAND)
    band[0] = False
    print(f"{what}: {int(band.sum())} element(s) in the band, closest |dp2 - thr| = {np.abs(dp2[1:] - 0.002).min() if len(dp2) > 1 else np.inf:.2e}, "
          f"|z - thr| = {np.abs(z - 0.12).min():.2e}, differing from the restatement: {int((got != mask).sum())}")
    assert band.sum() <= BAND_SHARE * band.size, (what, int(band.sum()))
    if not band_allowed:
        assert not band.any(), (what, "an element of this clip is inside the band")
    assert set(np.unique(got)) <= {0.0, 1.0} and (got[0] == 1.0).all()
    assert np.array_equal(got[~band], mask[~band]), (what, np.argwhere((got != mask) & ~band)[:5])
    if want is not None:
        assert np.array_equal(got[~band], want[~band]), (what, "differs from the reference's recorded mask", np.argwhere((got != want) & ~band)[:5])


# ---- 1. contact masks --------------------------------------------------------------------------------------------------------------------
def test_contact_masks_of_the_23dof_clips_in_one_launch():
    """walk, ue_walk, horse stance, a 1-frame and a 2-frame cut and a clip whose mask is not wanted, concatenated: clip boundaries fall inside
    workgroups (4 frames each).  A skeleton without masses: the contact half needs none."""
    sk = skeleton_json("g1_23dof")
    names = ["walk", "ue_walk", "horse"]
    clips = [clip(n) for n in names] + [cut(clip("walk"), 50, 51), cut(clip("ue_walk"), 100, 102), cut(clip("horse"), 0, 7)]
    p = params_of(sk, ContactDetection(enable=True))
    starts, foot, _ = run_frames(sk, clips, p, stability=False)
    mask, _ = run_clips(starts, p, foot_pos=foot, derive=[1, 1, 1, 1, 1, 0])
    fx = fixture()
    for i, c in enumerate(clips[:5]):
        a, b = starts[i], starts[i + 1]
        pos, _ = restate_fk(sk, c["pose_aa"], c["root_trans_offset"])
        err = float(np.abs(foot[a:b] - pos[:, p.foot[:]]).max())
        print(f"clip {i}: max |foot position - float64 FK| = {err:.2e}")
        assert err <= 3e-6 * max(1.0, float(np.abs(pos).max()))
        want = fx[f"contact::{names[i]}::mask"] if i < 3 else None
        assert_mask(mask[a:b], pos[:, p.foot[:]], f"23dof clip {i}", want=want, band_allowed=False)
        if want is not None:
            assert np.array_equal(mask[a:b], want)                  # no element in the band: equal everywhere
    assert (mask[starts[3]:starts[4]] == 1.0).all() and (mask[starts[4]] == 1.0).all()


def test_contact_mask_of_the_29dof_clip():
    sk = skeleton_json("g1_29dof")
    c = clip("rig29")
    p = params_of(sk, ContactDetection(enable=True))
    starts, foot, _ = run_frames(sk, [c], p, stability=False)
    mask, _ = run_clips(starts, p, foot_pos=foot)
    pos, _ = restate_fk(sk, c["pose_aa"], c["root_trans_offset"])
    assert_mask(mask, pos[:, p.foot[:]], "29dof", want=fixture()["contact::rig29::mask"])
    # thresholds are parameters, not constants: other values give the restatement's other mask
    cd = ContactDetection(enable=True, vel_threshold=0.0005, height_threshold=0.2, foot_bodies=["right_ankle_roll_link", "left_ankle_roll_link"])
    p2 = params_of(sk, cd)
    starts, foot2, _ = run_frames(sk, [c], p2, stability=False)
    assert np.array_equal(foot2[:, 0], foot[:, 1]) and np.array_equal(foot2[:, 1], foot[:, 0])       # column 0 is the first name
    mask2, _ = run_clips(starts, p2, foot_pos=foot2)
    want2, dp2, z = restate_contact(pos[:, p2.foot[:]], 0.0005, 0.2)
    off = (np.abs(dp2 - 0.0005) < VEL_BAND) | (np.abs(z - 0.2) < HEIGHT_BAND)
    assert off.sum() <= BAND_SHARE * off.size and np.array_equal(mask2[~off], want2[~off]) and not np.array_equal(mask2, mask[:, ::-1])


# ---- 2. distances and verdicts of the shipped clips ----------------------------------------------------------------------------------------
def _distances(robot, names, extra=()):
    sk = skeleton_mjcf(robot)
    clips = [clip(n) for n in names] + list(extra)
    p = params_of(sk, None, Screening(enable=True))
    starts, _, dist = run_frames(sk, clips, p, contact=False)
    for i, c in enumerate(clips):
        d = dist[starts[i]:starts[i + 1]]
        want, scale = restate_distance(sk, c["pose_aa"], c["root_trans_offset"])
        err = np.abs(d.astype(np.float64) - want)
        print(f"{robot} clip {i}: max |d - restatement| = {err.max():.2e} (bound 1e-4 x {np.maximum(1.0, scale).max():.1f}), d in [{want.min():.4f}, {want.max():.4f}]")
        assert np.isfinite(d).all() and (err <= 1e-4 * np.maximum(1.0, scale)).all(), (robot, i, float(err.max()))
    return sk, clips, starts, dist


def test_distances_and_verdicts_of_the_23dof_clips():
    sk, clips, starts, dist = _distances("g1_23dof", ["walk", "ue_walk", "horse"], extra=[cut(clip("walk"), 50, 51), cut(clip("horse"), 100, 102)])
    for N, want in ((100, [True, True, True]), (50, [True, True, False])):
        _, rep = run_clips(starts, params_of(sk, None, Screening(enable=True, epsilon_stab_frames=N)), dist=dist)
        for i, c in enumerate(clips):
            r = restate_verdict(restate_distance(sk, c["pose_aa"], c["root_trans_offset"])[0], 0.1, N)
            assert bool(rep[i, 0]) == r["stable"] and int(rep[i, 5]) == r["max_gap"], (N, i, rep[i], r)
            assert abs(rep[i, 1] - r["first_dist"]) <= 1e-4 and abs(rep[i, 2] - r["last_dist"]) <= 1e-4 and abs(rep[i, 3] - r["max_dist"]) <= 1e-4
            assert abs(rep[i, 4] - r["unstable_share"]) <= 1e-6 and (rep[i, 6:] == 0).all()
        assert [bool(s) for s in rep[:3, 0]] == want
        assert int(rep[2, 5]) == 77                                  # the horse stance's largest gap


def test_distance_and_verdict_of_the_29dof_clip():
    sk, clips, starts, dist = _distances("g1_29dof", ["rig29"])
    _, rep = run_clips(starts, params_of(sk, None, Screening(enable=True)), dist=dist)
    r = restate_verdict(restate_distance(sk, clips[0]["pose_aa"], clips[0]["root_trans_offset"])[0])
    assert not bool(rep[0, 0]) and not r["stable"] and int(rep[0, 5]) == r["max_gap"]
    assert abs(rep[0, 2] - 9.0) < 0.1 and abs(rep[0, 4] - r["unstable_share"]) <= 1e-6


# ---- 3. the verdict rule on the fixture's synthetic sequences ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [10, 100])
def test_verdict_rule_on_synthetic_sequences(N):
    """every case of the fixture with this N in ONE launch, clips of different lengths (1 ... 700 frames: fewer and more than a workgroup's
    256 threads), against the reference's recorded verdict and the restatement's report"""
    fx = fixture()
    cases = [c for c in verdict_cases() if int(fx[f"verdict::{c}::params"][1]) == N]
    assert len(cases) >= 4
    seqs = [fx[f"verdict::{c}::dist"] for c in cases]
    starts = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32)
    p = _lib.PbhcMotionScreen()
    p.epsilon_stab, p.epsilon_stab_frames = 0.1, N
    _, rep = run_clips(starts, p, dist=np.concatenate(seqs))
    for i, c in enumerate(cases):
        r = restate_verdict(seqs[i].astype(np.float32), 0.1, N)
        print(c, rep[i, :6], r)
        assert bool(rep[i, 0]) == bool(fx[f"verdict::{c}::stable"]) == r["stable"], c
        assert int(rep[i, 5]) == r["max_gap"], c
        assert rep[i, 3] == np.float32(r["max_dist"]) and abs(rep[i, 4] - r["unstable_share"]) <= 1e-6, c
        assert np.array_equal(rep[i, 1:3], np.float32([r["first_dist"], r["last_dist"]]), equal_nan=True), c


def test_start_arrays_that_do_not_describe_the_input_index_nothing():
    """a clip whose start entries run past the input, backwards, or below zero is left unwritten by both launches; the others are not harmed"""
    sk = skeleton_mjcf("g1_23dof")
    c = cut(clip("walk"), 0, 12)
    Bx, total = sk.num_bodies_ext, 12
    good = np.array([0, 5, 12], np.int32)
    p = params_of(sk, ContactDetection(enable=True), Screening(enable=True))
    _, foot_ok, dist_ok = run_frames(sk, [cut(c, 0, 5), cut(c, 5, 12)], p)
    csk = sk.to_c()
    d_mass, d_com, d_derive, d_good = up(sk.body_mass), up(sk.body_com), up([1, 1], np.int32), up(good, np.int32)
    for bad in ([0, 5, 40], [0, 9, 5], [-3, 5, 12], [0, 2 ** 30, 12]):
        d_pose, d_trans, d_start = up(c["pose_aa"][:, :Bx]), up(c["root_trans_offset"]), up(bad, np.int32)
        foot = torch.full((total, 2, 3), SENTINEL, device=DEV)
        dist = torch.full((total,), SENTINEL, device=DEV)
        ground = torch.full((2,), SENTINEL, device=DEV)
        mask = torch.full((total, 2), SENTINEL, device=DEV)
        report = torch.full((2, 8), SENTINEL, device=DEV)
        st = _lib.current_stream()
        _lib.check(_lib.lib().pbhc_motion_screen_frames(C.byref(csk), _lib.ptr(d_pose), _lib.ptr(d_trans), total, 2, _lib.ptr(d_start), p, _lib.ptr(d_mass),
                                                        _lib.ptr(d_com), _lib.ptr(ground), _lib.ptr(foot), _lib.ptr(dist), st), "frames")
        _lib.check(_lib.lib().pbhc_motion_screen_clips(_lib.ptr(foot), _lib.ptr(dist), total, 2, _lib.ptr(d_start), _lib.ptr(d_derive), p,
                                                       _lib.ptr(mask), _lib.ptr(report), st), "clips")
        torch.cuda.synchronize()
        foot, dist, mask, report = foot.cpu().numpy(), dist.cpu().numpy(), mask.cpu().numpy(), report.cpu().numpy()
        for ci in range(2):
            a, b = int(bad[ci]), int(bad[ci + 1])
            ok = a >= 0 and b - a >= 1 and b <= total
            if not ok:
                assert (report[ci] == SENTINEL).all(), (bad, ci)
            else:
                assert np.array_equal(foot[a:b], foot_ok[a:b]) and (mask[a:b] != SENTINEL).all() and (report[ci] != SENTINEL).all(), (bad, ci)
        written = foot[:, 0, 0] != SENTINEL
        for f in np.flatnonzero(written):                             # whatever was written is the right frame's value
            assert np.array_equal(foot[f], foot_ok[f]), (bad, f)
    lib = _lib.lib()
    assert lib.pbhc_motion_screen_clips(None, None, 12, 2, _lib.ptr(d_good), None, p, None, None, None) == _lib.K["PBHC_EINVAL"]
    assert lib.pbhc_motion_screen_frames(C.byref(csk), None, None, 12, 2, None, p, None, None, None, None, None, None) == _lib.K["PBHC_EINVAL"]


# ---- 4. through MotionLib ----------------------------------------------------------------------------------------------------------------
def with_mask(c, mask):
    return dict(c, contact_mask=np.asarray(mask, np.float32))


def direct_mask(sk, c):
    p = params_of(sk, ContactDetection(enable=True))
    starts, foot, _ = run_frames(sk, [c], p, stability=False)
    return run_clips(starts, p, foot_pos=foot)[0]


def bits(t):
    return t.contiguous().view(torch.int32)


def test_library_derives_the_masks_and_builds_the_same_tables():
    sk = skeleton_json("g1_23dof")
    walk, horse = clip("walk"), clip("horse")
    want = direct_mask(sk, walk)
    cd = ContactDetection(enable=True)
    a = MotionLib(sk, [walk], 4, DEV, contact_detection=cd)
    assert a.has_contact_mask and a.contact_derived == [True] and a.screen_report is None
    assert np.array_equal(a._clips[0]["contact_mask"], want) and "contact_mask" not in walk            # a copy: the caller's dict is untouched
    b = MotionLib(sk, [with_mask(walk, want)], 4, DEV)
    assert torch.equal(bits(a.frames), bits(b.frames)) and a.num_frames.tolist() == b.num_frames.tolist()
    D = sk.num_dof
    assert np.array_equal(a.frames[:, 2 * D:2 * D + 2].cpu().numpy(), want)
    # a mixed library: the horse stance ships its mask and keeps it bit for bit
    m = MotionLib(sk, [walk, horse], 4, DEV, contact_detection=cd)
    assert m.contact_derived == [True, False] and m.has_contact_mask
    assert m._clips[1] is horse and np.array_equal(m.frames[122:, 2 * D:2 * D + 2].cpu().numpy().view(np.uint32), np.asarray(horse["contact_mask"], np.float32).view(np.uint32))
    n = MotionLib(sk, [with_mask(walk, want), horse], 4, DEV)
    assert torch.equal(bits(m.frames), bits(n.frames))
    # overwrite: every clip is derived
    o = MotionLib(sk, [walk, horse], 4, DEV, contact_detection=ContactDetection(enable=True, overwrite=True))
    assert o.contact_derived == [True, True] and np.array_equal(o._clips[1]["contact_mask"], direct_mask(sk, horse))
    assert not np.array_equal(o._clips[1]["contact_mask"], horse["contact_mask"])
    # every clip ships a mask and nothing is overwritten: nothing is derived
    q = MotionLib(sk, [horse], 4, DEV, contact_detection=cd)
    assert q.contact_derived == [False] and q._clips[0] is horse


def test_detection_under_crops_and_with_variants_and_extension():
    sk = skeleton_json("g1_23dof")
    walk = clip("walk")
    want = direct_mask(sk, walk)
    cd = ContactDetection(enable=True)
    N, K = 4, 48
    starts = torch.tensor([0, 10, 40, 122 - K])
    a = MotionLib(sk, [walk], N, DEV, max_len=K, contact_detection=cd)
    b = MotionLib(sk, [with_mask(walk, want)], N, DEV, max_len=K)
    for ml in (a, b):
        ml.load_motions(random_sample=False, max_len=K, crop_starts=starts)
    assert a.max_len == K and a.has_contact_mask and torch.equal(bits(a.frames), bits(b.frames))
    D = sk.num_dof
    assert np.array_equal(a.frames[K:2 * K, 2 * D:2 * D + 2].cpu().numpy(), want[10:10 + K])
    # augmentation + interpolation: the mask is derived on the source clip, then mirrored / extended like a shipped one
    rc = fixture_config("v1_g1_23dof_walk.yaml", 4).robot
    pose0 = [0.0, 0.0, 0.8, 0.0, 0.0, 0.0, 1.0] + [float(rc.init_state.default_joint_angles[n]) for n in rc.dof_names]
    ip = Interpolation(num_dof=23, default_pose=np.asarray(pose0), start_frames=4, end_frames=3)
    v = MotionLib(sk, [walk], N, DEV, interpolation=ip, augmentation=Augmentation(mirror=True), contact_detection=cd)
    w = MotionLib(sk, [with_mask(walk, want)], N, DEV, interpolation=ip, augmentation=Augmentation(mirror=True))
    assert v.num_frames.tolist() == [129, 129] and torch.equal(bits(v.frames), bits(w.frames))
    src, mir = v.extended_clips()
    assert np.array_equal(src["contact_mask"][4:126], want) and np.array_equal(mir["contact_mask"][4:126], want[:, ::-1])
    for c in (src, mir):
        assert (c["contact_mask"][:4] == 0.5).all() and (c["contact_mask"][126:] == 0.5).all()
    assert v.built_clip(1)["contact_mask"].shape == (129, 2)


def test_screening_report_and_exclude():
    sk = skeleton_mjcf("g1_23dof")
    walk, horse = clip("walk"), clip("horse")
    rep = MotionLib(sk, [walk, horse], 4, DEV, screening=Screening(enable=True, epsilon_stab_frames=50))
    r = rep.screen_report
    assert r["stable"].tolist() == [True, False] and r["kept"].tolist() == [0, 1] and rep._num_unique_motions == 2
    assert r["max_gap"].tolist() == [1, 77] and set(r) == set(motion_screen.REPORT_FIELDS) | {"kept"}
    d = rep.stability_distance(1)
    want, scale = restate_distance(sk, horse["pose_aa"], horse["root_trans_offset"])
    assert d.shape == (210,) and (np.abs(d - want) <= 1e-4 * np.maximum(1.0, scale)).all()
    assert abs(r["first_dist"][1] - want[0]) <= 1e-4 and abs(r["max_dist"][1] - want.max()) <= 1e-4 and not rep.has_contact_mask
    plain = MotionLib(sk, [walk, horse], 4, DEV)
    assert torch.equal(bits(rep.frames), bits(plain.frames))                       # `report` changes nothing else
    ex = MotionLib(sk, [walk, horse], 4, DEV, screening=Screening(enable=True, epsilon_stab_frames=50, action="exclude"))
    assert ex.screen_report["kept"].tolist() == [0] and ex.screen_report["stable"].tolist() == [True, False]
    assert ex._sampling_prob.shape == (1,) and ex._num_unique_motions == 1 and ex.num_frames.tolist() == [122] and len(ex._clips) == 1
    assert ex.load_motions(random_sample=False).tolist() == [0, 0, 0, 0] and ex.stability_distance(1).shape == (210,)
    assert torch.equal(bits(ex.frames), bits(MotionLib(sk, [walk], 4, DEV).frames))
    keep = MotionLib(sk, [walk, horse], 4, DEV, screening=Screening(enable=True, action="exclude"))             # N = 100: both pass
    assert keep.screen_report["kept"].tolist() == [0, 1] and keep._num_unique_motions == 2
    both = MotionLib(sk, [horse, walk], 4, DEV, contact_detection=ContactDetection(enable=True),
                     screening=Screening(enable=True, epsilon_stab_frames=50, action="exclude"))
    assert both.contact_derived == [False, True] and both.screen_report["kept"].tolist() == [1] and both.has_contact_mask
    assert np.array_equal(both._clips[0]["contact_mask"], direct_mask(sk, walk))
    with pytest.raises(_lib.PbhcError, match="empty"):                            # nothing left, a one-clip library included
        MotionLib(sk, [horse], 4, DEV, screening=Screening(enable=True, epsilon_stab_frames=50, action="exclude"))
    with pytest.raises(_lib.PbhcError, match="MJCF"):
        MotionLib(skeleton_json("g1_23dof"), [walk], 4, DEV, screening=Screening(enable=True))
    with pytest.raises(_lib.PbhcError, match="left_toe"):
        MotionLib(sk, [walk], 4, DEV, contact_detection=ContactDetection(enable=True, foot_bodies=["left_toe", "right_ankle_roll_link"]))


def test_absent_keys_leave_the_tables_byte_identical():
    sk = skeleton_json("g1_23dof")
    walk, horse = clip("walk"), clip("horse")
    plain = MotionLib(sk, [walk, horse], 4, DEV)
    off = MotionLib(sk, [walk, horse], 4, DEV, contact_detection=ContactDetection(enable=False), screening=Screening(enable=False))
    none = MotionLib(sk, [walk, horse], 4, DEV, contact_detection=None, screening=None)
    for ml in (off, none):
        assert torch.equal(bits(ml.frames), bits(plain.frames)) and not ml.has_contact_mask and ml.contact_derived == [False, False]
        assert ml.screen_report is None and ml.contact_detection is None and ml.screening is None
    mcfg = fixture_config("v1_g1_23dof_walk.yaml", 4).robot.motion
    assert mcfg.get("contact_detection", None) is None and mcfg.get("screening", None) is None
    assert torch.equal(bits(MotionLib.from_config(mcfg, sk, 4, DEV).frames), bits(MotionLib(sk, [walk], 4, DEV).frames))
    with pytest.raises(_lib.PbhcError, match="without robot.motion.screening"):
        plain.stability_distance(0)


# ---- 5. an env ---------------------------------------------------------------------------------------------------------------------------
def test_env_with_the_contact_mask_reward_on_a_clip_without_a_mask():
    ov = {"rewards.reward_scales.teleop_contact_mask": 0.5}
    with pytest.raises(AttributeError, match="contact_mask"):                     # as today
        build_hip_env("v1_g1_23dof_walk.yaml", 16, overrides=ov)
    cfg, env = build_hip_env("v1_g1_23dof_walk.yaml", 16, overrides=dict(ov, **{"robot.motion.contact_detection": {"enable": True}}))
    ml = env._motion_lib
    assert ml.has_contact_mask and ml.contact_derived == [True]
    assert np.array_equal(ml._clips[0]["contact_mask"], direct_mask(env.skeleton, clip("walk")))
    env.reset_all()
    for _ in range(3):
        obs, rew, reset, _ = env.step({"actions": torch.zeros(16, env.num_dof, device=DEV)})
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in obs.values()) and torch.isfinite(rew).all()
    ref = ml.get_motion_state(torch.zeros(1, dtype=torch.long, device=DEV), torch.zeros(1, device=DEV))
    assert ref["contact_mask"].tolist() == [[1.0, 1.0]]
