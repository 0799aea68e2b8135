"""Exact resume on the GPU (DESIGN.md §8 "Exact resume"): a run continued from a checkpoint with a training state ends bit for bit where the
run that wrote the checkpoint ends when it carries on.  Every comparison is torch.equal / ==; there is no tolerance anywhere.

Each case builds its runs inside one process from the same seeds (torch, numpy, random) and the same seeded replay window, as
tests/test_gpu_parity.py::_rollouts_with_split does.  64 envs, num_steps_per_env of the config, 2 + 2 iterations; the overrides make the
state move inside those four rollouts (time-outs inside one rollout, noise and DR on, a motion resample every 30 steps) and every case
asserts that it did.

Case 1 of the issue asks for `reinit_epis_rand` > 0 AND (case 4) for a rollout through the captured graph; `rollout_graph_safe` never
allows the graph with `reinit_epis_rand` > 0 (the re-draw is decided on the host in every step), so the two live in two runs here: the
`after_loop` case runs with the re-draw schedule on (every rollout eager), the graph case repeats it with the schedule off and checks the
same equality over an eager first and a replayed second rollout.

The clocks are the one thing no two runs share: `tot_time` sums measured device times.  It is restored, so a resumed run equals the run it
continues; a run that never saves is compared with one that saves every iteration on everything but `tot_time`.
"""
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from pbhc_amd import _lib
from pbhc_amd.envs.env_config import SIGMA_KEYS
from pbhc_amd.utils import resume
from tests.helpers import ROOT, build_hip_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V1 = "v1_g1_23dof_walk.yaml"
SEED = 11
DT = 0.02                                                  # control step of both configs (200 Hz, decimation 4)
# 15-step episodes (time-outs inside every 24-step rollout), a resample of every slot each 30 steps (< two rollouts)
MOVING = {"env.config.max_episode_length_s": 15 * DT - 1e-3, "env.config.resample_motion_when_training": True,
          "env.config.resample_time_interval_s": 30 * DT - 1e-3, "algo.config.save_training_state": True}
V1_OV = dict(MOVING, **{"env.config.start_sampling": {"enable": True, "bins": 8, "update_every_rollouts": 1}})
V1_REINIT = dict(V1_OV, **{"domain_rand.reinit_epis_rand": 20})
# the graph case: resamples at steps 50 and 100 only, so that the rollouts from steps 51 and 75 hold none and may run as the captured graph
V1_GRAPH = dict(V1_OV, **{"env.config.resample_time_interval_s": 50 * DT - 1e-3})
V2_OV = dict(MOVING, **{"robot.motion.augmentation": {"mirror": True, "speeds": [0.8]}, "env.config.clip_sampling": {"enable": True},
                        "robot.motion.motion_max_len": 40, "algo.config.dagger_update_freq": 2, "algo.config.save_interval": 1,
                        "rewards.reward_penalty_curriculum": True})           # (the teacher config ships with every curriculum off)


def _seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def _build(kind, overrides, seed=SEED, num_envs=64, log_dir=None):
    """env + agent from the seeds, with the seeded replay window in place, and the event log of its rollouts"""
    import bench

    _seed_all(seed)
    if kind == "v1":
        from pbhc_amd.agents.mh_ppo import MHPPO

        cfg, env = build_hip_env(V1, num_envs, noise_off=False, overrides=overrides)
        algo = MHPPO(env=env, config=cfg.algo.config, log_dir=log_dir, device=DEV)
        algo.setup()
    else:
        from tests.test_gpu_parity_v2 import _v2_algo

        cfg, env, algo = _v2_algo(num_envs, overrides=overrides, noise_off=False)
        algo.log_dir = log_dir
    env.simulator.set_replay(*bench.make_replay_on_device(env, 4 * algo.num_steps_per_env + 8, seed=5))
    ev = dict(graph=[], time_outs=0, resamples=0, hist=[])
    roll, resample = algo._rollout_step, env.resample_motion

    def rollout(obs):
        out = roll(obs)
        ev["graph"].append(bool(algo._rollout_used_graph))
        ev["time_outs"] += int(algo._time_outs.sum())
        ev["hist"].append(bool(getattr(algo, "hist_encoding", False)))
        return out

    def resample_motion(*a, **k):
        ev["resamples"] += 1
        return resample(*a, **k)

    algo._rollout_step, env.resample_motion = rollout, resample_motion
    return env, algo, ev


def _end_state(algo):
    torch.cuda.synchronize()
    out = {}
    for k in ("_pflat", "_mflat", "_vflat", "_lr", "_adam_step"):
        v = getattr(algo, k)
        for i, vi in enumerate(v if isinstance(v, (list, tuple)) else [v]):          # (ppo_mimic: one moment buffer per optimiser)
            out[f"{k}.{i}"] = vi.clone()
    for path, leaf in resume.leaves(algo.training_state()):
        out["training_state." + path] = leaf
    return out


def _same(a, b):
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())
    return type(a) is type(b) and a == b


def _assert_same_state(a, b, skip=()):
    assert a.keys() == b.keys()
    differing = [k for k in a if k not in skip and not _same(a[k], b[k])]
    assert not differing, differing


def _assert_state_moved(env, ev):
    """at least one time-out, one resample, a changed curriculum value or sigma — a run that never leaves the initial state proves nothing"""
    K = _lib.K
    g, g0 = env.globals.cpu(), torch.tensor(env.layout.globals0, dtype=torch.float64)
    s = slice(K["PBHC_G_SIGMA"], K["PBHC_G_SIGMA"] + len(SIGMA_KEYS))
    assert ev["time_outs"] > 0 and ev["resamples"] > 0
    assert not torch.equal(g[s], g0[s]) or g[K["PBHC_G_PENALTY_SCALE"]] != g0[K["PBHC_G_PENALTY_SCALE"]]
    assert g[K["PBHC_G_AVG_EP_LEN"]] != g0[K["PBHC_G_AVG_EP_LEN"]]


_CACHE = {}


def _after_loop_pair(tag, overrides, tmp):
    """A: learn(2), save, learn(2).  B: fresh env and agent, load, learn(2).  -> (end of A, end of B, events of A, events of B, envs, path);
    computed once per `tag` and shared"""
    if tag not in _CACHE:
        path = os.path.join(str(tmp), f"after_loop_{tag}.pt")
        env_a, a, ev_a = _build("v1", overrides)
        a.learn(2)
        a.save(path, infos={"tag": tag})
        a.learn(2)
        end_a = _end_state(a)
        env_b, b, ev_b = _build("v1", overrides)
        assert b.load(path) == {"tag": tag}
        b.learn(2)
        _CACHE[tag] = (end_a, _end_state(b), ev_a, ev_b, env_a, env_b, path)
    return _CACHE[tag]


@pytest.fixture(scope="module")
def shared_tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("resume")


def test_v1_after_loop_resume_is_bit_identical(shared_tmp):
    """case 1: MHPPO, start statistics + start sampling on, reinit_epis_rand > 0"""
    end_a, end_b, ev_a, ev_b, env_a, env_b, _ = _after_loop_pair("reinit", V1_REINIT, shared_tmp)
    _assert_state_moved(env_a, ev_a)
    assert ev_b["resamples"] > 0 and ev_b["time_outs"] > 0            # ... and it moved after the resume point too
    assert env_a._reinit.counter > 0 and env_a._start_redraws > 1
    assert not any(ev_a["graph"] + ev_b["graph"])                       # (reinit_epis_rand: the re-draw is decided on the host every step)
    _assert_same_state(end_a, end_b)


def test_v1_resume_hands_over_from_an_eager_rollout_to_the_graph(shared_tmp):
    """case 4: B's first rollout runs eagerly (nothing has run in its process yet, whatever the restored rollout count says), its second
    through the captured graph — and B still ends where A ends"""
    end_a, end_b, ev_a, ev_b, env_a, env_b, _ = _after_loop_pair("graph", V1_GRAPH, shared_tmp)
    _assert_state_moved(env_a, ev_a)
    assert ev_b["graph"] == [False, True], ev_b
    assert ev_a["graph"] == [False, False, True, True], ev_a           # (the second rollout holds the resample of step 50)
    assert int(end_b["training_state.rollouts_done"]) == 4
    _assert_same_state(end_a, end_b)


def _in_loop_triple(kind, overrides, tmp_path):
    """A: learn(4), saving every iteration.  B: fresh, loads A's model_1.pt, learn(2).  A'': learn(4) without a log_dir: never saves."""
    ov = dict(overrides, **{"algo.config.save_interval": 1})
    env_a, a, ev_a = _build(kind, ov, log_dir=str(tmp_path))
    a.learn(4)
    end_a = _end_state(a)
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".pt")) == [f"model_{i}.pt" for i in range(5)]
    env_b, b, ev_b = _build(kind, ov)
    b.load(os.path.join(str(tmp_path), "model_1.pt"))
    assert b.current_learning_iteration == 2 and b._resume_in_loop
    steps_before = env_b.common_step_counter
    b.learn(2)
    assert env_b.common_step_counter == steps_before + 2 * b.num_steps_per_env      # no reset_all() step: the preamble was skipped
    _assert_state_moved(env_a, ev_a)
    assert ev_b["resamples"] > 0 and ev_b["time_outs"] > 0
    _assert_same_state(end_a, _end_state(b))
    return ov, end_a, ev_a, ev_b


def test_v1_in_loop_resume_is_bit_identical_and_saving_is_not_an_event(tmp_path):
    """case 2"""
    ov, end_a, ev_a, ev_b = _in_loop_triple("v1", V1_REINIT, tmp_path)
    env_n, never, ev_n = _build("v1", ov, log_dir=None)
    never.learn(4)
    assert ev_n["graph"] == ev_a["graph"]
    _assert_same_state(end_a, _end_state(never), skip=("training_state.tot_time",))      # (a sum of measured times: see the module docstring)


def test_v2_in_loop_resume_is_bit_identical(tmp_path):
    """case 3: ppo_mimic.PPO teacher, four clips from one (mirror + one speed), failure-weighted clip sampling, 40-frame crops per slot,
    dagger_update_freq 2: hist_encoding flips across the resume boundary, a wrong next_iteration would show"""
    ov, end_a, ev_a, ev_b = _in_loop_triple("v2", V2_OV, tmp_path)
    assert ev_a["hist"] == [True, False, True, False] and ev_b["hist"] == [True, False]
    assert int(end_a["training_state.agent.counter"]) == 6                       # 4 PPO updates + 2 DAgger updates
    assert float(end_a["_adam_step.0"][1]) > 0                                    # the history encoder's optimiser has stepped


def test_refusals_leave_the_env_untouched_and_old_files_load_as_before(tmp_path):
    """case 5"""
    env, algo, _ = _build("v1", V1_OV)
    before = dict(resume.leaves(env.state_dict()))
    for what, kw in (("seed", dict(seed=SEED + 1)), ("num_envs", dict(num_envs=32))):
        _, other, _ = _build("v1", V1_OV, **kw)
        ts = other.training_state()
        with pytest.raises(_lib.PbhcError, match=what + r".*the saved state has \S+, this run has \S+"):
            env.load_state_dict(ts["env"])
        with pytest.raises(_lib.PbhcError, match=what):
            algo.load_training_state(ts)
        del other
    with pytest.raises(_lib.PbhcError, match="version"):
        algo.load_training_state(dict(algo.training_state(), version=resume.STATE_VERSION + 1))
    _assert_same_state(before, dict(resume.leaves(env.state_dict())))
    # the key absent: today's keys, loads as today
    algo.config["save_training_state"] = False
    algo.learn(1)
    plain, full = str(tmp_path / "plain.pt"), str(tmp_path / "full.pt")
    algo.save(plain, infos={"x": 1})
    d = torch.load(plain, map_location="cpu", weights_only=True)
    assert set(d.keys()) == {"actor_model_state_dict", "critic_model_state_dict", "actor_optimizer_state_dict", "critic_optimizer_state_dict", "iter", "infos"}
    algo.config["save_training_state"] = True
    algo.save(full)
    assert set(torch.load(full, map_location="cpu", weights_only=True).keys()) == set(d.keys()) | {"training_state"}
    weights = (algo._pflat.clone(), algo._mflat.clone(), algo._vflat.clone())
    algo.learn(1)
    moved = dict(resume.leaves(env.state_dict()))
    assert algo.load(plain) == {"x": 1} and algo.current_learning_iteration == d["iter"]
    assert all(torch.equal(x, y) for x, y in zip(weights, (algo._pflat, algo._mflat, algo._vflat)))
    _assert_same_state(moved, dict(resume.leaves(env.state_dict())))             # a file without the key leaves the env alone
    # load_training_state: false — weights and optimiser only
    algo.learn(1)
    moved = dict(resume.leaves(env.state_dict()))
    algo.config["load_training_state"] = False
    algo.load(full)
    assert all(torch.equal(x, y) for x, y in zip(weights, (algo._pflat, algo._mflat, algo._vflat)))
    _assert_same_state(moved, dict(resume.leaves(env.state_dict())))
    assert not algo.__dict__.get("_resume_in_loop", False)


def digest_of(algo):
    """one line per leaf of the end state: its path and the sha256 of its bytes (case 6: compared as files)"""
    lines = []
    for k, v in sorted(_end_state(algo).items()):
        raw = (str(v.dtype) + str(tuple(v.shape))).encode() + v.cpu().contiguous().numpy().tobytes() if isinstance(v, torch.Tensor) else repr(v).encode()
        lines.append(f"{k} {hashlib.sha256(raw).hexdigest()}")
    return "\n".join(lines) + "\n"


def child_main(role, path, out):
    """one process of case 6: "A" runs learn(2), save, learn(2); "B" loads and runs learn(2); each writes the digest of its end state"""
    env, algo, ev = _build("v1", V1_REINIT)
    if role == "A":
        algo.learn(2)
        algo.save(path)
    else:
        algo.load(path)
    algo.learn(2)
    assert ev["time_outs"] > 0 and ev["resamples"] > 0
    with open(out, "w") as f:
        f.write(digest_of(algo))


def test_resume_across_processes(tmp_path):
    """case 6: the writer and the resumed run in two processes of their own (PBHC_GEMM_TUNING=0: the library GEMMs pick their solutions
    the same way in both)"""
    env = dict(os.environ, PBHC_GEMM_TUNING="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    ckpt = str(tmp_path / "model.pt")
    outs = []
    for role in ("A", "B"):
        out = str(tmp_path / f"digest_{role}.txt")
        code = f"from tests.test_gpu_resume import child_main; child_main({role!r}, {ckpt!r}, {out!r})"
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0, (role, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        outs.append(open(out).read())
    assert len(outs[0].splitlines()) > 60
    a, b = outs[0].splitlines(), outs[1].splitlines()
    assert [x for x in a if x not in b] == [] and a == b
