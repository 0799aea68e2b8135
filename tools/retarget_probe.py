"""The key-point fit (pbhc_amd/motion_retarget.py, csrc/pbhc_retarget.hip) under a stopwatch: microseconds per iteration and per kernel,
launches per iteration, bytes per iteration, and for context the float32 CPU model's time per iteration.

    python3 tools/retarget_probe.py [--iterations 200] [--cpu-threads 16]

Shapes: 1 clip x 200 frames and 256 clips x 300 frames of the 23-dof G1, 14 picks; the targets are the FK of the shipped horse-stance clip
(repeated to length), formed on the device by `pbhc_retarget_loss_grad`'s body positions.  The per-iteration time is the device time between
two events around one `pbhc_retarget_fit` call (all iterations enqueued, no synchronisation between them); the per-kernel times come from
torch's profiler over the same call.  Bytes per iteration: what the two launches read and write per frame, counted once,
    12 P + 12                                 key points, root translation
  + 4 D (1 + 2 + 2 + 1)                       joints read; square_avg, acc_delta read + written; the clamped joints written
  + 12 (2 + 2 + 2) + 16                       root rotation, its two Adam moments read + written; the frame's four partial sums
  + 16 + 4 D (1 + 1)                          clip launch: partial sums, pre-filter joints read (each once from memory, 5 x from cache), joints written
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pbhc_amd.motion_retarget import Fitter, RetargetSettings, heading_rotvec  # noqa: E402
from tests import retarget_model as rm  # noqa: E402

DEV = "cuda:0"


def settings():
    sk = rm.skeleton("g1")
    return sk, RetargetSettings(enable=True, joint_matches=[[n, i] for i, n in enumerate(rm.G1_PICKS)], limits=rm.g1_limits().tolist(), dof_lr=10.0)


def make_fitter(num_clips, frames):
    sk, st = settings()
    dof, root, trans = rm.horse_pose()
    idx = np.arange(frames) % dof.shape[0]
    dof, root, trans = (np.tile(a[idx].astype(np.float32), (num_clips, 1)) for a in (dof, root, trans))
    nf = [frames] * num_clips
    seed = Fitter(sk, st.to_c(sk), np.zeros((len(dof), 14, 3), np.float32), trans, root, nf, DEV)
    seed.dof.copy_(torch.from_numpy(dof))
    kp = seed.loss_grad(body_pos=True)[4][:, rm.picks_of("g1")].contiguous().cpu().numpy()
    l, r = (rm.G1_PICKS.index(n) for n in rm.G1_HEADING)
    return Fitter(sk, st.to_c(sk), kp, trans, heading_rotvec(kp[:, l], kp[:, r]), nf, DEV)


def bytes_per_frame(P, D):
    return 12 * P + 12 + 4 * D * 6 + 12 * 6 + 16 + 16 + 4 * D * 2


def measure(num_clips, frames, iterations):
    f = make_fitter(num_clips, frames)
    f.run(20)                                            # warm-up: code objects loaded, the state off its start
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        hist = f.run(iterations)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / iterations)
    per_kernel, launches = {}, None
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            f.run(iterations)
            torch.cuda.synchronize()
        for e in prof.key_averages():
            if "k_retarget" in e.key:
                name = "k_retarget_frame" if "frame" in e.key else "k_retarget_clip"
                dt = getattr(e, "device_time_total", None)
                per_kernel[name] = ((dt if dt is not None else e.cuda_time_total) / e.count, e.count)
        launches = sum(c for _, c in per_kernel.values()) / iterations if per_kernel else None
    except Exception as exc:                             # the profiler is a convenience: the event times above stand without it
        print(f"  (torch profiler not usable here: {type(exc).__name__}: {exc})")
    nbytes = bytes_per_frame(14, 23) * num_clips * frames
    med = float(np.median(times))
    print(f"{num_clips} clip(s) x {frames} frames ({num_clips * frames} frames, state + targets {nbytes / 1e6:.2f} MB per iteration)")
    print(f"  per iteration: median {med:.1f} us, min {min(times):.1f} us over 5 runs of {iterations} iterations; last loss {float(hist[-1].mean()) * 1e3:.2f} mm")
    for name, (us, count) in sorted(per_kernel.items()):
        print(f"  {name}: {us:.1f} us mean over {count} dispatches")
    if launches is not None:
        print(f"  launches per iteration: {launches:g}")
    print(f"  bytes per iteration / time: {nbytes / med / 1e6:.3f} TB/s")
    return med


def cpu_model(frames, threads, iterations=5):
    torch.set_num_threads(threads)
    sk, picks = rm.skeleton("g1"), rm.picks_of("g1")
    clips = rm.g1_fit_clips((frames,))
    t = time.perf_counter()
    rm.fit(sk, picks, clips, rm.g1_limits(), iterations, dof_lr=10.0, dtype=torch.float32)
    return (time.perf_counter() - t) / iterations * 1e6


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--cpu-threads", type=int, default=16)
    args = ap.parse_args(argv)
    for num_clips, frames in ((1, 200), (256, 300)):
        measure(num_clips, frames, args.iterations)
    print(f"float32 CPU model (torch autograd, {args.cpu_threads} threads), 1 clip x 200 frames: {cpu_model(200, args.cpu_threads):.0f} us per iteration")
    return 0


if __name__ == "__main__":
    sys.exit(main())
