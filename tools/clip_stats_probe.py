"""The per-clip statistics collector (env.config.clip_statistics) under the profiler.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/clip_stats_probe.py steps ENVS
        reset_all + 20 control steps of the v1 walk config with the switch on, on one stream: one k_env_step, one k_env_finalize and one
        k_clip_stats dispatch per step
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/clip_stats_probe.py rollout ENVS [on|off]
        four MHPPO rollouts (the last three replay the rollout's hipGraph): the collector on the finalize stream, next to the policy forward
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/clip_stats_probe.py sweep
        the collector alone on synthetic arrays: SWEEP_REPS launches for every (envs, clips, fraction of envs that reset) of SWEEP, in order
  python3 tools/clip_stats_probe.py sweep-summary DIR
        median (minimum) per configuration of that trace, microseconds
  python3 tools/clip_stats_probe.py summary DIR [DIR ...]
        per directory: median (minimum) of the dispatches of the three kernels, microseconds; for a rollout trace also on which queue
        k_clip_stats ran and how many of its dispatches overlap a k_mlp_fwd (policy) dispatch in time; and every kernel name of the trace
"""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _config(num_envs, on):
    from pbhc_amd.utils.config import load_config

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ov = {"num_envs": num_envs, "simulator._target_": "pbhc_amd.simulator.replay_stub.ReplaySimStub"}
    if on:
        ov["env.config.clip_statistics"] = True
    return load_config(os.path.join(root, "tests", "golden", "configs", "v1_g1_23dof_walk.yaml"), ov, now="probe")


def steps(num_envs):
    import torch

    import bench
    from pbhc_amd.envs.motion_tracking import LeggedRobotMotionTracking

    torch.manual_seed(0)
    env = LeggedRobotMotionTracking(_config(num_envs, True).env.config, "cuda:0")
    env.reset_all()
    env.simulator.set_replay(*bench.make_replay_on_device(env, 24, seed=1))
    a = torch.zeros(num_envs, env.num_dof, device="cuda:0")
    for _ in range(20):
        env.step({"actions": a})
    torch.cuda.synchronize()
    st = env.clip_statistics()
    print(f"envs {num_envs}: specialised={env.is_specialised}, episodes {int(st['episodes'].sum())}, failures {int(st['failures'].sum())}")


def rollout(num_envs, on):
    import torch

    import bench
    from pbhc_amd.agents.mh_ppo import MHPPO
    from pbhc_amd.envs.motion_tracking import LeggedRobotMotionTracking

    torch.manual_seed(0)
    cfg = _config(num_envs, on)
    env = LeggedRobotMotionTracking(cfg.env.config, "cuda:0")
    algo = MHPPO(env=env, config=cfg.algo.config, log_dir=None, device="cuda:0")
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
    print(f"envs {num_envs}: switch {'on' if on else 'off'}, rollouts as one graph: {used}" +
          (f", episodes {int(env.clip_statistics()['episodes'].sum())}" if on else ""))


SWEEP = [(n, m, f) for n in (4096, 32768) for m in (1, 256) for f in (0.0, 0.008, 1.0)]
SWEEP_REPS = 30


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
        window = torch.zeros(m, 4, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for _ in range(SWEEP_REPS):
            _lib.check(lib.pbhc_clip_stats(reset.data_ptr(), tout.data_ptr(), ratio.data_ptr(), length.data_ptr(), slot.data_ptr(), n, m,
                                           window.data_ptr(), _lib.current_stream()), "pbhc_clip_stats")
        torch.cuda.synchronize()
        assert int(window[:, 0].sum()) == SWEEP_REPS * int(reset.sum())
        print(f"envs {n} clips {m} reset fraction {frac}: {int(reset.sum())} resets per launch")


def sweep_summary(d):
    f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
    rows = [r for r in csv.DictReader(open(f)) if "k_clip_stats" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == SWEEP_REPS * len(SWEEP), len(rows)
    print("envs   clips  resetting   k_clip_stats median (min) us")
    for i, (n, m, frac) in enumerate(SWEEP):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[i * SWEEP_REPS:(i + 1) * SWEEP_REPS]][5:]
        print(f"{n:<6d} {m:<6d} {frac:<10g}  {statistics.median(us):6.2f} ({min(us):5.2f})")


def summary(dirs):
    for d in dirs:
        f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
        rows = list(csv.DictReader(open(f)))
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        span = lambda r: (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
        print(d)
        for name in ("k_env_step", "k_env_finalize", "k_clip_stats"):
            us = [(span(r)[1] - span(r)[0]) / 1e3 for r in rows if name in r["Kernel_Name"]]
            if len(us) > 2:
                print(f"  {name:16s} median {statistics.median(us[2:]):7.2f} (min {min(us[2:]):7.2f}) us over {len(us[2:])} of {len(us)} dispatches")
            else:
                print(f"  {name:16s} {len(us)} dispatches")
        clip = [r for r in rows if "k_clip_stats" in r["Kernel_Name"]]
        policy = [span(r) for r in rows if "k_mlp_fwd" in r["Kernel_Name"]]
        if clip and policy:
            step_q = {r["Queue_Id"] for r in rows if "k_env_step" in r["Kernel_Name"]}
            fin_q = {r["Queue_Id"] for r in rows if "k_env_finalize" in r["Kernel_Name"]}
            other = sum(r["Queue_Id"] not in step_q for r in clip)
            with_fin = sum(r["Queue_Id"] in fin_q for r in clip)
            over = sum(any(s < span(r)[1] and span(r)[0] < e for s, e in policy) for r in clip)
            print(f"  k_clip_stats: {other} of {len(clip)} dispatches on a queue k_env_step never uses, {with_fin} on a queue of k_env_finalize; "
                  f"{over} overlap a k_mlp_fwd dispatch in time")
        names = sorted({r["Kernel_Name"].split("(")[0][:70] for r in rows})
        print(f"  {len(names)} kernel names: " + "; ".join(names))


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "steps":
        steps(int(sys.argv[2]))
    elif mode == "sweep":
        sweep()
    elif mode == "sweep-summary":
        sweep_summary(sys.argv[2])
    elif mode == "rollout":
        rollout(int(sys.argv[2]), (sys.argv[3] if len(sys.argv) > 3 else "on") == "on")
    else:
        summary(sys.argv[2:])
