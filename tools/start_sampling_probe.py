"""The start-time collector and draw (env.config.start_sampling) under the profiler.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/start_sampling_probe.py sweep
        k_start_stats, k_start_draw and k_clip_stats alone on the same synthetic arrays: SWEEP_REPS launches of each for every
        (envs, clips, fraction of envs that reset) of SWEEP, in order; K = 32 bins
  python3 tools/start_sampling_probe.py sweep-summary DIR
        median (minimum) per configuration and kernel of that trace, microseconds
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/start_sampling_probe.py rollout ENVS [on|off [WORKLOAD [CLIPS]]]
        four rollouts of a bench.py workload (default v1_walk; the last three replay the rollout's hipGraph), a fold after each
  python3 tools/start_sampling_probe.py rollout-summary DIR
        how many k_start_* dispatches the trace holds, their medians, and in the replayed rollouts the gap between the end of the last
        k_start_draw of a step and the start of the next k_env_step
"""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWEEP = [(n, m, f) for n in (4096, 32768) for m in (1, 256) for f in (0.0, 0.008, 1.0)]
SWEEP_REPS = 30
BINS = 32
KERNELS = ("k_start_stats", "k_start_draw", "k_clip_stats")


def sweep():
    import torch

    from pbhc_amd import _lib

    lib, dev = _lib.lib(), "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    for n, m, frac in SWEEP:
        reset = (torch.rand(n, device=dev, generator=g) < frac).long()
        tout = torch.zeros(n, dtype=torch.uint8, device=dev)
        ratio, length = torch.rand(n, device=dev, generator=g), torch.randint(0, 1000, (n,), device=dev, generator=g)
        slot = torch.randint(0, m, (n,), device=dev, generator=g)
        clip_len = torch.full((m,), 60.0, device=dev)
        window = torch.zeros(m, BINS, 2, dtype=torch.int64, device=dev)
        clip_window = torch.zeros(m, 4, dtype=torch.int64, device=dev)
        cdf = torch.cumsum(torch.full((m, BINS), 1.0 / BINS, dtype=torch.float64, device=dev), dim=1).contiguous()
        counter = torch.zeros(1, dtype=torch.float64, device=dev)
        start = torch.zeros(n, device=dev)
        torch.cuda.synchronize()
        st = _lib.current_stream()
        for _ in range(SWEEP_REPS):
            _lib.check(lib.pbhc_start_stats(reset.data_ptr(), tout.data_ptr(), ratio.data_ptr(), length.data_ptr(), slot.data_ptr(), clip_len.data_ptr(),
                                            0.02, n, m, BINS, window.data_ptr(), st), "pbhc_start_stats")
        for _ in range(SWEEP_REPS):
            _lib.check(lib.pbhc_start_draw(cdf.data_ptr(), clip_len.data_ptr(), slot.data_ptr(), reset.data_ptr(), None, n, m, BINS, 1, counter.data_ptr(),
                                           0, start.data_ptr(), st), "pbhc_start_draw")
        for _ in range(SWEEP_REPS):
            _lib.check(lib.pbhc_clip_stats(reset.data_ptr(), tout.data_ptr(), ratio.data_ptr(), length.data_ptr(), slot.data_ptr(), n, m,
                                           clip_window.data_ptr(), st), "pbhc_clip_stats")
        torch.cuda.synchronize()
        assert int(window[:, :, 0].sum()) <= SWEEP_REPS * int(reset.sum()) and int(clip_window[:, 0].sum()) == SWEEP_REPS * int(reset.sum())
        print(f"envs {n} clips {m} reset fraction {frac}: {int(reset.sum())} resets per launch")


def _rows(d):
    f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
    rows = list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return rows


def _us(r):
    return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3


def sweep_summary(d):
    rows = _rows(d)
    print("envs   clips  resetting   " + "   ".join(f"{k} median (min) us" for k in KERNELS))
    per = {k: [r for r in rows if k in r["Kernel_Name"]] for k in KERNELS}
    for k in KERNELS:
        assert len(per[k]) == SWEEP_REPS * len(SWEEP), (k, len(per[k]))
    for i, (n, m, frac) in enumerate(SWEEP):
        cells = []
        for k in KERNELS:
            us = [_us(r) for r in per[k][i * SWEEP_REPS:(i + 1) * SWEEP_REPS]][5:]
            cells.append(f"{statistics.median(us):6.2f} ({min(us):5.2f})")
        print(f"{n:<6d} {m:<6d} {frac:<10g}  " + "        ".join(cells))


def rollout(num_envs, on, workload="v1_walk", clips=1):
    import torch

    import bench
    import pbhc_amd.utils.config as config

    orig = config.load_config
    if on:                                           # (bench.build has no way to pass an override)
        config.load_config = lambda path, ov=None, **kw: orig(path, dict(ov or {}, **{"env.config.start_sampling": {"enable": True}}), **kw)
    try:
        cfg, env, Algo = bench.build(num_envs, "cuda:0", 0, workload, num_clips=clips)
    finally:
        config.load_config = orig
    algo = Algo(env=env, config=cfg.algo.config, log_dir=None, device="cuda:0")
    algo.setup()
    obs = env.reset_all()
    env.simulator.set_replay(*bench.make_replay_on_device(env, 24 * 5 + 2, seed=1))
    algo._train_mode()
    used = []
    for _ in range(4):
        obs = algo._rollout_step(obs)
        used.append(bool(algo._rollout_used_graph))
        algo.storage.clear()
    torch.cuda.synchronize()
    print(f"{workload}, {clips} clips, envs {num_envs}: start_sampling {'on' if on else 'absent'}, rollouts as one graph: {used}" +
          (f", log {({k: float(v) for k, v in env.read_log().items() if k.startswith('start_')})}" if on else ""))


def rollout_summary(d):
    rows = _rows(d)
    for k in ("k_env_step", "k_env_finalize", "k_start_stats", "k_start_draw", "k_start_sampling_update"):
        us = [_us(r) for r in rows if k in r["Kernel_Name"]]
        print(f"  {k:24s} {len(us)} dispatches" + (f", median {statistics.median(us):6.2f} (min {min(us):5.2f}) us" if us else ""))
    steps = [r for r in rows if "k_env_step" in r["Kernel_Name"]]
    draws = [r for r in rows if "k_start_draw" in r["Kernel_Name"]]
    gaps = []
    for a, b in zip(steps, steps[1:]):
        inside = [int(r["End_Timestamp"]) for r in draws if int(a["End_Timestamp"]) <= int(r["Start_Timestamp"]) < int(b["Start_Timestamp"])]
        if len(inside) == 1:                         # (a fold's redraw-all makes two: between rollouts, not inside one)
            gaps.append((int(b["Start_Timestamp"]) - inside[0]) / 1e3)
    if gaps:
        tail = gaps[len(gaps) // 4:]                 # the replayed rollouts
        print(f"  end of k_start_draw -> start of the next k_env_step: median {statistics.median(tail):6.2f} us, min {min(tail):6.2f} us over {len(tail)} steps")


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "sweep":
        sweep()
    elif mode == "sweep-summary":
        sweep_summary(sys.argv[2])
    elif mode == "rollout":
        rollout(int(sys.argv[2]), (sys.argv[3] if len(sys.argv) > 3 else "on") == "on", *(sys.argv[4:5] or ["v1_walk"]),
                clips=int(sys.argv[5]) if len(sys.argv) > 5 else 1)
    else:
        rollout_summary(sys.argv[2])
