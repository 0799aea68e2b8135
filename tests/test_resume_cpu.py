"""Exact resume, the parts that need no GPU: generator states through a checkpoint file, the re-draw schedule, the config fingerprint and
the version check (DESIGN.md §8 "Exact resume")."""
import random

import numpy as np
import pytest
import torch

from pbhc_amd import _lib
from pbhc_amd.agents.base import _load_checkpoint
from pbhc_amd.envs.motion_tracking import ReinitSchedule
from pbhc_amd.utils import resume, rng_state
from tests.helpers import build_env_config

CFG = "v1_g1_23dof_walk.yaml"


def _through_file(tmp_path, obj):
    """what a checkpoint does to it: torch.save, then the non-executing loader the agents use"""
    p = str(tmp_path / "state.pt")
    torch.save({"training_state": obj}, p)
    return _load_checkpoint(p, "cpu")["training_state"]


def test_torch_cpu_generator_round_trip(tmp_path):
    g = torch.Generator().manual_seed(7)
    torch.rand(5, generator=g)
    packed = _through_file(tmp_path, rng_state.pack_torch(g.get_state()))
    want = torch.rand(16, generator=g)
    h = torch.Generator()
    h.set_state(rng_state.unpack_torch(packed))
    assert torch.equal(torch.rand(16, generator=h), want)


def test_python_random_round_trip(tmp_path):
    r = random.Random(7)
    r.gauss(0.0, 1.0)                                  # (leaves gauss_next set: the third member is a float, not None)
    packed = _through_file(tmp_path, rng_state.pack_python(r.getstate()))
    want = [r.randint(0, 10**9) for _ in range(16)] + [r.gauss(0.0, 1.0)]
    q = random.Random()
    q.setstate(rng_state.unpack_python(packed))
    assert [q.randint(0, 10**9) for _ in range(16)] + [q.gauss(0.0, 1.0)] == want
    fresh = rng_state.unpack_python(_through_file(tmp_path, rng_state.pack_python(random.Random(3).getstate())))
    assert fresh == random.Random(3).getstate()        # gauss_next None survives as None


def test_numpy_global_state_round_trip(tmp_path):
    before = np.random.get_state()
    try:
        np.random.seed(7)
        np.random.randn(3)                             # (an odd count: has_gauss / cached_gaussian are live)
        packed = _through_file(tmp_path, rng_state.pack_numpy(np.random.get_state()))
        want = np.concatenate([np.random.rand(16), np.random.randn(1)])
        np.random.seed(99)
        np.random.set_state(rng_state.unpack_numpy(packed))
        assert np.array_equal(np.concatenate([np.random.rand(16), np.random.randn(1)]), want)
    finally:
        np.random.set_state(before)


def test_reinit_schedule_state_round_trip(tmp_path):
    before = np.random.get_state()
    try:
        np.random.seed(5)
        a = ReinitSchedule(30.0)
        fired_a = [a.due(k) for k in range(1, 40)]
        saved = _through_file(tmp_path, {"counter": float(a.counter), "numpy": rng_state.pack_numpy(np.random.get_state())})
        more_a = [a.due(k) for k in range(40, 400)]
        np.random.seed(123)
        b = ReinitSchedule(30.0)
        b.counter = float(saved["counter"])
        np.random.set_state(rng_state.unpack_numpy(saved["numpy"]))
        assert [b.due(k) for k in range(40, 400)] == more_a and b.counter == a.counter
        assert fired_a[0] and sum(more_a) >= 2           # the schedule did fire after the save
        off = _through_file(tmp_path, {"counter": float(ReinitSchedule(-1).counter)})
        assert off["counter"] == float("inf")
    finally:
        np.random.set_state(before)


def _fingerprint(seed=3, num_envs=16, overrides=None):
    cfg, skel, c, L = build_env_config(CFG, overrides, num_envs=num_envs, seed=seed, general=False, has_contact_mask=True)
    return resume.config_fingerprint(c, num_clips=1, clip_frames=[120])


@pytest.fixture(scope="module")
def base_fingerprint():
    return _fingerprint()


def test_config_fingerprint_agrees_between_builds_and_holds_no_address(base_fingerprint):
    a = base_fingerprint
    ballast = [torch.zeros(4096 + 17 * i) for i in range(8)]      # the second build allocates at other addresses
    b = _fingerprint()
    del ballast
    assert a == b
    assert all(isinstance(k, str) and isinstance(v, str) for k, v in a.items())


def test_config_fingerprint_moves_with_seed_num_envs_and_a_reward_scale(base_fingerprint):
    a, other_seed = base_fingerprint, _fingerprint(seed=4)
    assert {k for k in a if a[k] != other_seed[k]} == {"seed"}
    assert {k for k in a if a[k] != _fingerprint(num_envs=32)[k]} >= {"num_envs"}
    scale = "rewards.reward_scales.teleop_body_position_extend"
    moved = _fingerprint(overrides={scale: 1.25})
    assert moved != a and moved["seed"] == a["seed"] and moved["num_envs"] == a["num_envs"]
    with pytest.raises(_lib.PbhcError, match="seed.*the saved state has .* this run has"):
        resume.check_fingerprint("load_state_dict", a, other_seed)
    with pytest.raises(_lib.PbhcError, match="motion.num_clips.*'1'.*'2'"):
        resume.check_fingerprint("load_state_dict", a, dict(a, **{"motion.num_clips": "2"}))


def test_unknown_version_is_refused():
    for bad in ({"version": resume.STATE_VERSION + 1}, {"version": None}, {}):
        with pytest.raises(_lib.PbhcError, match="version"):
            resume.check_version(bad, "load_training_state")
    resume.check_version({"version": resume.STATE_VERSION}, "load_training_state")


def test_training_state_of_an_unknown_version_is_refused_before_anything_else():
    """`check_training_state` looks at the version first: a state of another version may hold anything else"""
    from pbhc_amd.agents.base import OnDeviceAgent

    agent = OnDeviceAgent.__new__(OnDeviceAgent)       # (no env, no device: the check must not get that far)
    with pytest.raises(_lib.PbhcError, match=f"version {resume.STATE_VERSION + 7}"):
        agent.check_training_state({"version": resume.STATE_VERSION + 7})


def test_training_state_is_refused_with_more_than_one_rank():
    """every rank owns an env shard and only rank 0 writes: refused at the point of use, naming the key"""
    from pbhc_amd.agents.base import OnDeviceAgent

    agent = OnDeviceAgent.__new__(OnDeviceAgent)
    agent.world_size = 2
    with pytest.raises(NotImplementedError, match="save_training_state"):
        agent.training_state()
    with pytest.raises(NotImplementedError, match="load_training_state"):
        agent.load_training_state({"version": resume.STATE_VERSION})


def test_env_state_is_refused_during_a_recording_and_during_a_library_sweep():
    from pbhc_amd.envs.motion_tracking import LeggedRobotMotionTracking

    env = LeggedRobotMotionTracking.__new__(LeggedRobotMotionTracking)
    env._rec, env._rec_dumped, env._start_suspended = {"dof_pos": None}, False, False
    assert "save_motion" in env._state_dict_refusal()
    with pytest.raises(_lib.PbhcError, match="save_motion"):
        env.state_dict()
    env._rec, env._start_suspended = None, True
    with pytest.raises(_lib.PbhcError, match="library_sweep"):
        env.state_dict()
    with pytest.raises(_lib.PbhcError, match="library_sweep"):
        env.load_state_dict({})
