"""The library sweep (env.library_sweep) and its scoring kernel under the profiler / the clock.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/library_eval_probe.py kernels ENVS
        20 "steps" on random in-range states of the 29-DoF G1 against a one-clip table, each step three dispatches on one stream:
        k_sim_fk, k_motion_state (the unfused alternative: what k_clip_track computes, stored to memory) and k_clip_track itself with
        every env active and none reset (its most expensive case)
  python3 tools/library_eval_probe.py summary DIR [DIR ...]
        per directory: median (minimum) of the dispatches of the three kernels, microseconds, the first two dispatches of each dropped
  python3 tools/library_eval_probe.py sweep [ENVS [CLIPS]]
        wall time of one library_sweep of v2_teacher29 (bench.py's configs[2] build) with a synthetic library, untrained policy, a
        synthetic replay window installed per wave; the second of two sweeps is the figure (the first one selects the GEMM kernels and
        generates the replay windows)
"""
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("k_sim_fk", "k_motion_state", "k_clip_track")


def kernels(num_envs):
    import ctypes as C

    import numpy as np
    import torch

    from pbhc_amd import _lib
    from pbhc_amd.motion_lib import MotionLib, load_motion_file
    from pbhc_amd.skeleton import Skeleton

    dev, N = "cuda:0", num_envs
    sk = Skeleton.from_json(os.path.join(ROOT, "tests", "golden", "skeleton_g1_29dof_rev_1_0.json"))
    clip = load_motion_file(os.path.join(ROOT, "tests", "golden", "clips", "g1_rig_Skeleton_Sequence_converted_processed_g1_29dof_rev_1_0.npz"))[0][1]
    ml = MotionLib(sk, [clip], 1, dev)
    csk, lib = sk.to_c(), _lib.lib()
    D, B, Bx = sk.num_dof, sk.num_bodies, sk.num_bodies_ext
    g = torch.Generator(device=dev).manual_seed(0)
    ids = torch.zeros(N, dtype=torch.int64, device=dev)
    times = torch.rand(N, device=dev, generator=g) * ml._motion_lengths[0]
    origins = torch.randn(N, 3, device=dev, generator=g)
    ref = torch.empty(N, ml.row, device=dev)
    st = _lib.current_stream()
    _lib.check(lib.pbhc_motion_state(C.byref(ml.table), Bx, D, ids.data_ptr(), times.data_ptr(), origins.data_ptr(), N, ref.data_ptr(), st), "pbhc_motion_state")
    o = 2 * D + 2
    root = torch.zeros(N, 13, device=dev)
    root[:, 0:3] = ref[:, o:o + 3] + 0.02 * torch.randn(N, 3, device=dev, generator=g)
    root[:, 3:7] = ref[:, o + 3 * Bx:o + 3 * Bx + 4]
    dof_state = torch.stack([ref[:, :D] + 0.02 * torch.randn(N, D, device=dev, generator=g), ref[:, D:2 * D]], dim=-1).contiguous()
    bodies = torch.empty(N, B, 13, device=dev)
    reset = torch.zeros(N, dtype=torch.int64, device=dev)
    M = N
    slot = torch.arange(N, dtype=torch.int64, device=dev)                  # as in a sweep: every add of a launch on its own row
    window = torch.zeros(M, 4, dtype=torch.int64, device=dev)
    for _ in range(20):
        _lib.check(lib.pbhc_sim_fk(C.byref(csk), root.data_ptr(), dof_state.data_ptr(), dof_state.data_ptr() + 4, 2, N, bodies.data_ptr(), st), "pbhc_sim_fk")
        _lib.check(lib.pbhc_motion_state(C.byref(ml.table), Bx, D, ids.data_ptr(), times.data_ptr(), origins.data_ptr(), N, ref.data_ptr(), st), "pbhc_motion_state")
        _lib.check(lib.pbhc_clip_track(C.byref(csk), C.byref(ml.table), root.data_ptr(), dof_state.data_ptr(), times.data_ptr(), origins.data_ptr(),
                                       ids.data_ptr(), reset.data_ptr(), slot.data_ptr(), None, N, M, window.data_ptr(), st), "pbhc_clip_track")
    torch.cuda.synchronize()
    w = window.cpu().numpy()
    print(f"envs {N}: frames per row {int(w[:, 0].min())}..{int(w[:, 0].max())}, mean E_gmpbpe {float(np.mean(w[:, 1] / 1048576.0 / w[:, 0])):.4f} m")


def summary(dirs):
    for d in dirs:
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
        print(d)
        for k in KERNELS:
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"]))
                  if r["Kernel_Name"].startswith(k + "(") or r["Kernel_Name"] == k][2:]
            if us:
                print(f"  {k:16s} {len(us):3d} dispatches  median {statistics.median(us):7.2f} us  (min {min(us):.2f})")
        print("  kernels in the trace:", ", ".join(sorted({r["Kernel_Name"].split("(")[0] for r in rows})))


def sweep(num_envs=4096, num_clips=256):
    import torch

    import bench

    dev = "cuda:0"
    cfg, env, Algo = bench.build(num_envs, dev, seed=1234, workload="v2_teacher29", num_clips=num_clips)
    algo = Algo(env=env, config=cfg.algo.config, log_dir=None, device=dev)
    algo.setup()
    env.reset_all()
    ml = env._motion_lib
    T = int(float(ml._motion_lengths.max()) / env.dt) + 12

    windows = {}

    def before_wave(w, clip_ids):
        if w not in windows:                                 # (generated in the first sweep, reused by the timed one)
            # the state make_replay_on_device reads, as the reset that follows will leave it: episode clock 0, motion time 0
            env._episode_length_buf.zero_()
            env.motion_start_times.zero_()
            env.motion_len.copy_(ml.get_motion_length(env.motion_ids))
            windows[w] = bench.make_replay_on_device(env, T, seed=5 + w)
        env.simulator.set_replay(*windows[w])

    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = algo.evaluate_library(before_wave=before_wave)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"sweep {rep}: {num_envs} envs, {num_clips} clips, {out['waves']} wave(s), {out['steps']} steps, {dt * 1e3:.1f} ms wall "
              f"({dt * 1e3 / out['steps']:.3f} ms per step), success_rate {out['success_rate']:.3f}, "
              f"unfinished {len(out['unfinished'])}, E_gmpbpe {out['E_gmpbpe_mean']:.4f} m, E_mpbpe {out['E_mpbpe_mean']:.4f} m, "
              f"E_mpjpe {out['E_mpjpe_mean']:.4f} rad, specialised={env.is_specialised}")


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "kernels":
        kernels(int(sys.argv[2]))
    elif mode == "summary":
        summary(sys.argv[2:])
    elif mode == "sweep":
        sweep(*[int(x) for x in sys.argv[2:4]])
    else:
        raise SystemExit(__doc__)
