"""Diagnostic (GPU box): what `algo.config.symmetry` costs in the update.

  python3 tools/symmetry_probe.py [ENVS [CLIPS]]

`_training_step` of the bench.py workload v2_teacher29 (default 4096 envs, a 256-clip library: 128 synthetic source clips and their mirror
images) with the key absent and with `symmetry: {enable: true}`, alternating, five runs each after one warm-up, on the same rollout buffer
and permutation: medians of device time (events).  Then the two kernels alone on the update's shapes: `pbhc_mirror_rows` with the three jobs
of one update ([T * N] rows) and `pbhc_symmetry_loss` on one minibatch.  Output kept in profiles/symmetry_loss.txt.
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RUNS = 5
REPS = 20


def build(envs, clips, symmetry, direct=True):
    """direct False: the actor-side stacks (actor, privileged encoder) hand their gradients back to autograd, which accumulates them — what
    both of their applications do while the key is on — instead of storing them into the flat gradient buffer"""
    import torch

    import bench
    from pbhc_amd import motion_lib as ML
    from pbhc_amd.utils.config import load_config

    w = bench.WORKLOADS["v2_teacher29"]
    ov = {"num_envs": envs, "simulator._target_": "pbhc_amd.simulator.replay_stub.ReplaySimStub", "algo.config.teacher_model_path": None,
          "algo.config.dagger_only": False, "robot.motion.augmentation": {"mirror": True}}
    if symmetry:
        ov["algo.config.symmetry"] = {"enable": True, "coef": 1.0}
    cfg = load_config(os.path.join(bench.ROOT, "tests", "golden", "configs", w["cfg"]), ov, now="probe")
    torch.manual_seed(1)
    from pbhc_amd.agents.ppo_mimic import PPO
    from pbhc_amd.envs.general_tracking import LeggedRobotGeneralTracking

    orig = ML.load_motion_file
    ML.load_motion_file = lambda path: [(f"synth{i}", c) for i, c in enumerate(bench.synth_library(orig(path)[0][1], clips // 2, seed=7))]
    try:
        env = LeggedRobotGeneralTracking(cfg.env.config, "cuda:0")
    finally:
        ML.load_motion_file = orig
    algo = PPO(env=env, config=cfg.algo.config, log_dir=None, device="cuda:0")
    algo.setup()
    if not direct:
        from pbhc_amd.agents import fused_mlp

        for m in (algo.alg.actor.actor_module, algo.alg.actor.priv_encoder):
            fused_mlp.grad_direct(m.module, False)
    algo._train_mode()
    algo.storage.clear()
    algo._rollout_step(env.reset_all())
    return env, algo


def timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    import torch

    from pbhc_amd import _lib

    envs = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    clips = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    algos = {"absent": build(envs, clips, False), "on": build(envs, clips, True), "absent, actor-side gradients through autograd": build(envs, clips, False, direct=False)}
    env, algo = algos["on"]
    n = algo.storage.num_envs * algo.storage.num_transitions_per_env
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to("cuda:0")
    times = {k: [] for k in algos}
    for run in range(RUNS + 1):
        for k, (_, a) in algos.items():
            ms = timed(lambda: a._training_step(indices=perm))
            if run:
                times[k].append(ms)
    steps = algo.num_learning_epochs * algo.num_mini_batches
    print(f"v2_teacher29, {envs} envs, {clips} clips ({clips // 2} sources + mirror images), {n} rows per update, {steps} optimiser steps of {algo._mb} rows")
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print(f"_training_step, symmetry {k}: median {med[k]:.2f} ms of {RUNS} runs ({', '.join(f'{x:.2f}' for x in v)})")
    print(f"symmetry on - absent: {med['on'] - med['absent']:+.2f} ms per update = {(med['on'] - med['absent']) / steps:+.3f} ms per optimiser step "
          f"({100.0 * (med['on'] / med['absent'] - 1.0):+.1f} %)")
    auto = med["absent, actor-side gradients through autograd"] - med["absent"]
    print(f"autograd accumulation instead of direct gradient stores, ONE application of the actor-side stacks: {auto:+.2f} ms per update = "
          f"{auto / steps:+.3f} ms per optimiser step")
    # ---- the kernels alone
    st = algo.storage
    keys = algo.MIRRORED_KEYS
    src = {k: getattr(st, k).flatten(0, 1)[perm].contiguous() for k in keys}
    dst = {k: torch.empty_like(v) for k, v in src.items()}
    jobs = [(k, src[k], dst[k]) for k in keys]
    ms = [timed(lambda: env.mirror_rows(jobs)) for _ in range(REPS)]
    moved = 2 * 4 * sum(v.numel() for v in src.values())
    m = statistics.median(ms)
    print(f"pbhc_mirror_rows, 3 jobs x {n} rows (widths {[v.shape[1] for v in src.values()]}): median {m * 1e3:.1f} us (min {min(ms) * 1e3:.1f}) of {REPS}; "
          f"{moved / 1e6:.0f} MB read + written = {moved / m / 1e6:.0f} GB/s")
    B, A = algo._mb, algo.num_act
    mu, mu_m = torch.randn(B, A, device="cuda:0"), torch.randn(B, A, device="cuda:0")
    index, sign = env.mirror_maps()["actions"]
    lib = _lib.lib()
    call = lambda: _lib.check(lib.pbhc_symmetry_loss(mu.data_ptr(), mu_m.data_ptr(), index.data_ptr(), sign.data_ptr(), B, A, 1.0, algo._grad_mu_m.data_ptr(),
                                                     algo._sym_scratch.data_ptr(), algo._sym_scalar.data_ptr(), None, _lib.current_stream()), "pbhc_symmetry_loss")
    ms = [timed(call) for _ in range(REPS)]
    print(f"pbhc_symmetry_loss, B {B} x A {A} (two launches): median {statistics.median(ms) * 1e3:.1f} us (min {min(ms) * 1e3:.1f}) of {REPS}")


if __name__ == "__main__":
    main()
