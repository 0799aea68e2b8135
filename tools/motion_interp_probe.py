"""Diagnostic (GPU box): what `robot.motion.interpolation` costs at ingestion — the tools/ingest_probe.py workload (2048 synthetic clips made from
the shipped 29-DoF clip) with the key absent and with (30, 30) lead-in / lead-out frames, alternating, five runs each.  Prints the wall-time
medians, the extension launch's own time (device events around `pbhc_motion_extend_batch`), the build's time per frame and the yardstick:
the plain ingestion plus the build's per-frame time x the frames the extension adds.  Output kept in profiles/motion_interp.txt."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from pbhc_amd.motion_interp import Interpolation
from pbhc_amd.motion_lib import MotionLib
from pbhc_amd.skeleton import Skeleton
from tests.helpers import GOLDEN, clip_from_env_golden, fixture_config

M = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
RUNS = 5
g = dict(np.load(os.path.join(GOLDEN, "env_v2_teacher29.npz")))
sk = Skeleton.from_json(os.path.join(GOLDEN, "skeleton_g1_29dof_rev_1_0.json"))
clips = bench.synth_library(clip_from_env_golden(g), M, seed=7)
rc = fixture_config("v2_g1_29dof_teacher.yaml", 4).robot
ip = Interpolation.from_config({"start_frames": 30, "end_frames": 30}, sk.num_dof, robot=rc)

ext_ms = []


def timed(fn, sink):
    def wrapped(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a, **k)
        e1.record()
        e1.synchronize()
        sink.append(e0.elapsed_time(e1))
        return out
    return wrapped


MotionLib._extend_device = timed(MotionLib._extend_device, ext_ms)             # device time of the one launch (+ its start arrays' upload)


def ingest(interpolation):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ml = MotionLib(sk, clips, 4096, "cuda:0", interpolation=interpolation)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, int(ml.frames.shape[0])


for warm in (None, ip):                                                       # module load, allocator growth
    MotionLib(sk, clips[:4], 8, "cuda:0", interpolation=warm)
    ingest(warm)
ext_ms.clear()
wall = {"absent": [], "(30,30)": []}
frames = {}
for _ in range(RUNS):
    for name, spec in (("absent", None), ("(30,30)", ip)):
        ms, F = ingest(spec)
        wall[name].append(ms)
        frames[name] = F
med = {k: statistics.median(v) for k, v in wall.items()}
added = frames["(30,30)"] - frames["absent"]
per_frame_us = med["absent"] * 1e3 / frames["absent"]
ext = statistics.median(ext_ms)
print(f"library: {M} clips, {frames['absent']} frames; with (30,30): {frames['(30,30)']} frames (+{added}, +{100.0 * added / frames['absent']:.1f} %)")
for k in wall:
    print(f"ingestion, key {k}: median {med[k]:.1f} ms of {RUNS} runs ({', '.join(f'{v:.1f}' for v in wall[k])})")
print(f"extension launch (events around pbhc_motion_extend_batch, start arrays' upload included): median {ext:.3f} ms "
      f"({', '.join(f'{v:.3f}' for v in ext_ms)}) = {ext * 1e6 / frames['(30,30)']:.1f} ns per output frame")
print(f"plain ingestion per frame: {per_frame_us:.3f} us -> yardstick for (30,30): {med['absent']:.1f} + {per_frame_us * added / 1e3:.1f} = "
      f"{med['absent'] + per_frame_us * added / 1e3:.1f} ms; measured {med['(30,30)']:.1f} ms")
print(f"extension launch vs ingestion's per-frame time x added frames: {ext:.3f} ms vs {per_frame_us * added / 1e3:.3f} ms")
