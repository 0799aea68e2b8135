"""Diagnostic (GPU box): what the pre-pass of `robot.motion.contact_detection` + `robot.motion.screening` costs at ingestion — the
tools/ingest_probe.py workload (2048 synthetic clips made from the shipped 29-DoF clip) with both keys absent and with both on (every mask
derived, action report), alternating, five runs each.  Prints the wall-time medians of MotionLib(...), the pre-pass's own wall time
(upload, launches, the two read-backs) and the device time of its launches alone (events around `pbhc_motion_screen_frames` +
`pbhc_motion_screen_clips` on arrays already uploaded).  Output kept in profiles/motion_screen.txt."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from pbhc_amd import _lib, motion_screen
from pbhc_amd.motion_lib import MotionLib
from pbhc_amd.motion_screen import ContactDetection, Screening
from pbhc_amd.skeleton import Skeleton
from tests.helpers import GOLDEN, clip_from_env_golden

M = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
RUNS = 5
DEV = "cuda:0"
g = dict(np.load(os.path.join(GOLDEN, "env_v2_teacher29.npz")))
js = json.load(open(os.path.join(GOLDEN, "skeleton_g1_29dof_rev_1_0.json")))
B = len(js["body_names"])
ext = [dict(joint_name=n, parent_name=js["body_names"][js["parents"][i]], pos=js["offsets"][i], rot=js["local_rot_wxyz"][i])
       for i, n in enumerate(js["body_names_ext"]) if i >= B]
sk = Skeleton.from_mjcf(os.path.join(GOLDEN, "mjcf", "g1_29dof_rev_1_0.xml"), ext)          # the MJCF route: link masses
clips = bench.synth_library(clip_from_env_golden(g), M, seed=7)
cd, sc = ContactDetection(enable=True, overwrite=True), Screening(enable=True)

pre_ms = []
_screen = MotionLib._screen_device


def _timed(self, cl):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = _screen(self, cl)
    torch.cuda.synchronize()
    pre_ms.append((time.perf_counter() - t0) * 1e3)
    return out


MotionLib._screen_device = _timed


def ingest(on):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ml = MotionLib(sk, clips, 4096, DEV, contact_detection=cd if on else None, screening=sc if on else None)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, ml


for warm in (False, True):                                                     # module load, allocator growth
    MotionLib(sk, clips[:4], 8, DEV, contact_detection=cd if warm else None, screening=sc if warm else None)
    ingest(warm)
pre_ms.clear()
wall = {"absent": [], "on": []}
for _ in range(RUNS):
    for name, on in (("absent", False), ("on", True)):
        ms, ml = ingest(on)
        wall[name].append(ms)
        if on:
            rep = ml.screen_report
        total = int(ml.frames.shape[0])
        del ml
med = {k: statistics.median(v) for k, v in wall.items()}
print(f"library: {M} clips, {total} frames, Bx = {sk.num_bodies_ext}; stable {int(rep['stable'].sum())} of {M}, masks derived for all")
for k in wall:
    print(f"ingestion, {k}: median {med[k]:.1f} ms of {RUNS} runs ({', '.join(f'{v:.1f}' for v in wall[k])})")
print(f"pre-pass wall time (upload + 3 launches + read-back of masks [{total},2] and report [{M},8]): median {statistics.median(pre_ms):.1f} ms "
      f"({', '.join(f'{v:.1f}' for v in pre_ms)})")

# the launches alone, on arrays already on the device
Bx = sk.num_bodies_ext
nf = [c["pose_aa"].shape[0] for c in clips]
starts = np.concatenate([[0], np.cumsum(nf)]).astype(np.int32)
up = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(DEV)
d_pose = up(np.concatenate([np.asarray(c["pose_aa"], np.float32)[:, :Bx] for c in clips]))
d_trans = up(np.concatenate([np.asarray(c["root_trans_offset"], np.float32) for c in clips]))
d_start, d_derive = up(starts, np.int32), up(np.ones(M), np.int32)
d_mass, d_com = up(sk.body_mass), up(sk.body_com)
foot, dist, ground = torch.empty(total, 2, 3, device=DEV), torch.empty(total, device=DEV), torch.empty(M, device=DEV)
mask, report = torch.empty(total, 2, device=DEV), torch.empty(M, 8, device=DEV)
p, csk, lib = motion_screen.to_c(cd, sc, sk), sk.to_c(), _lib.lib()
frames_ms, clips_ms = [], []
for it in range(RUNS + 2):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    st = _lib.current_stream()
    e[0].record()
    _lib.check(lib.pbhc_motion_screen_frames(C.byref(csk), _lib.ptr(d_pose), _lib.ptr(d_trans), total, M, _lib.ptr(d_start), p, _lib.ptr(d_mass), _lib.ptr(d_com),
                                             _lib.ptr(ground), _lib.ptr(foot), _lib.ptr(dist), st), "frames")
    e[1].record()
    _lib.check(lib.pbhc_motion_screen_clips(_lib.ptr(foot), _lib.ptr(dist), total, M, _lib.ptr(d_start), _lib.ptr(d_derive), p, _lib.ptr(mask), _lib.ptr(report), st),
               "clips")
    e[2].record()
    e[2].synchronize()
    if it >= 2:
        frames_ms.append(e[0].elapsed_time(e[1]))
        clips_ms.append(e[1].elapsed_time(e[2]))
fm, cm = statistics.median(frames_ms), statistics.median(clips_ms)
print(f"launches alone (events, 2 warm-up + {RUNS}): pbhc_motion_screen_frames (2 kernels) median {fm:.3f} ms ({', '.join(f'{v:.3f}' for v in frames_ms)}) = "
      f"{fm * 1e6 / total:.1f} ns per frame; pbhc_motion_screen_clips (1 kernel) median {cm:.3f} ms ({', '.join(f'{v:.3f}' for v in clips_ms)}); "
      f"3 launches, {fm + cm:.3f} ms")
