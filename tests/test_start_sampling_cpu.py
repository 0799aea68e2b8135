"""env.config.start_statistics / start_sampling: the option resolver, the C ABI's argument checks, the crops refusal and the order of the
fold's all-reduce and update (no GPU)."""
import ctypes as C
import os
import re

import pytest
import torch

from pbhc_amd import _lib
from pbhc_amd import dist as pdist
from pbhc_amd.envs import env_config
from pbhc_amd.envs.motion_tracking import LeggedRobotMotionTracking
from pbhc_amd.motion_lib import MotionLib
from pbhc_amd.utils.config import load_config
from tests.helpers import GOLDEN

DEFAULTS = dict(bins=32, decay=0.9, prior_episodes=1.0, uniform_floor=0.1, lookahead_bins=4, lookahead_decay=0.8, update_every_rollouts=1)
EXPORTS = ("pbhc_start_stats", "pbhc_start_sampling_update", "pbhc_start_draw")


def _env_cfg(name, overrides=None):
    return load_config(os.path.join(GOLDEN, "configs", name), dict(overrides or {}), now="t").env.config


@pytest.mark.parametrize("name", ["v1_g1_23dof_walk.yaml", "v2_g1_29dof_teacher.yaml"])
def test_keys_absent_means_off(name):
    ec = _env_cfg(name)
    assert "start_statistics" not in ec and "start_sampling" not in ec
    o = env_config.start_options(ec)
    assert type(o) is dict and o == dict(statistics=False, sampling=False, **DEFAULTS)


def test_defaults_statistics_only_and_sampling_implies_statistics():
    assert env_config.START_SAMPLING_DEFAULTS == DEFAULTS
    o = env_config.start_options(_env_cfg("v1_g1_23dof_walk.yaml", {"env.config.start_statistics": True}))
    assert o["statistics"] is True and o["sampling"] is False
    o = env_config.start_options(_env_cfg("v1_g1_23dof_walk.yaml", {"env.config.start_sampling": {"enable": True}}))
    assert o == dict(statistics=True, sampling=True, **DEFAULTS)
    assert all(type(o[k]) is int for k in ("bins", "lookahead_bins", "update_every_rollouts"))
    given = {"enable": False, "bins": 128, "decay": 0.0, "prior_episodes": 3, "uniform_floor": 1.0, "lookahead_bins": 128, "lookahead_decay": 1.0,
             "update_every_rollouts": 7}
    o = env_config.start_options(_env_cfg("v2_g1_29dof_teacher.yaml", {"env.config.start_sampling": given}))
    assert o == dict(statistics=False, sampling=False, bins=128, decay=0.0, prior_episodes=3.0, uniform_floor=1.0, lookahead_bins=128,
                     lookahead_decay=1.0, update_every_rollouts=7)
    # the DEFAULT look-ahead follows a smaller bin count; a given one is held to it
    o = env_config.start_options(_env_cfg("v1_g1_23dof_walk.yaml", {"env.config.start_sampling": {"enable": True, "bins": 1}}))
    assert (o["bins"], o["lookahead_bins"]) == (1, 1)


@pytest.mark.parametrize("key,value", [("bins", 0), ("bins", 129), ("bins", 7.5), ("bins", float("nan")), ("decay", -0.01), ("decay", 1.01),
                                       ("decay", float("nan")), ("prior_episodes", 0.0), ("prior_episodes", -1.0), ("prior_episodes", float("inf")),
                                       ("uniform_floor", -0.1), ("uniform_floor", 1.5), ("lookahead_bins", 0), ("lookahead_bins", 33),
                                       ("lookahead_bins", 2.5), ("lookahead_decay", -0.5), ("lookahead_decay", 1.1), ("update_every_rollouts", 0),
                                       ("update_every_rollouts", 1.5), ("update_every_rollouts", float("inf")), ("decay", "fast"), ("bins", True)])
def test_out_of_range_values_are_refused_and_the_message_names_the_key(key, value):
    ec = _env_cfg("v1_g1_23dof_walk.yaml", {"env.config.start_sampling": {"enable": True, key: value}})
    with pytest.raises(_lib.PbhcError, match=r"env\.config\.start_sampling\." + key):
        env_config.start_options(ec)


def test_unknown_key_and_a_non_mapping_are_refused():
    with pytest.raises(_lib.PbhcError, match="floor"):
        env_config.start_options(_env_cfg("v1_g1_23dof_walk.yaml", {"env.config.start_sampling": {"enable": True, "floor": 0.1}}))
    with pytest.raises(_lib.PbhcError, match="start_sampling must be a mapping"):
        env_config.start_options(_env_cfg("v1_g1_23dof_walk.yaml", {"env.config.start_sampling": True}))


def test_a_library_of_crops_is_refused_and_the_message_names_both_keys():
    ml = MotionLib.__new__(MotionLib)
    ml.max_len = 8
    with pytest.raises(_lib.PbhcError, match=r"start_sampling.*motion_max_len"):
        ml.init_start_sampling(4)
    env = LeggedRobotMotionTracking.__new__(LeggedRobotMotionTracking)
    env.config, env._motion_lib = _env_cfg("v1_g1_23dof_walk.yaml", {"env.config.start_statistics": True}), ml
    with pytest.raises(_lib.PbhcError, match=r"start_sampling.*motion_max_len"):
        env._init_start_sampling()
    env.config = _env_cfg("v1_g1_23dof_walk.yaml")                # keys absent: nothing to refuse, nothing allocated
    env._init_start_sampling()
    assert env._start_window is None and env._start_time is None


def test_header_and_binding_agree_on_the_three_exports():
    text = _lib._strip_comments(open(_lib.HEADER).read())
    lib = _lib.lib()
    assert _lib.K["PBHC_START_MAX_BINS"] == 128
    for name in EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(getattr(lib, name).argtypes), name
    math_h = open(os.path.join(_lib.ROOT, "pbhc_amd", "csrc", "pbhc_math.h")).read()
    assert re.search(r"#define\s+PBHC_RNG_STREAM_START_SAMPLING\s+21u", math_h)


def test_null_and_bad_sizes_return_einval_without_a_gpu():
    lib, E = _lib.lib(), _lib.K["PBHC_EINVAL"]
    p = C.c_void_p(64)                 # never dereferenced: every call below is refused on the host
    # pbhc_start_stats(reset, tout, ratio, len, slot, clip_len, dt, N, M, K, window, stream)
    good = [p, p, p, p, p, p, 0.02, 4, 2, 8, p]
    for k in (0, 1, 2, 3, 4, 5, 10):   # each pointer on its own
        a = list(good)
        a[k] = None
        assert lib.pbhc_start_stats(*a, None) == E
        assert b"pbhc_start_stats" in lib.pbhc_last_error()
    for k, v in ((7, 0), (8, 0), (9, 0), (9, 129), (9, -1), (6, 0.0), (6, -0.02), (6, float("nan")), (6, float("inf"))):
        a = list(good)
        a[k] = v
        assert lib.pbhc_start_stats(*a, None) == E, (k, v)
    # pbhc_start_sampling_update(window, V, F, prob, cdf, M, K, decay, prior, floor, H, lambda, stream)
    good = [p, p, p, p, p, 3, 8, 0.9, 1.0, 0.1, 4, 0.8]
    for k in range(5):
        a = list(good)
        a[k] = None
        assert lib.pbhc_start_sampling_update(*a, None) == E
        assert b"pbhc_start_sampling_update" in lib.pbhc_last_error()
    for k, v in ((5, 0), (6, 0), (6, 129), (7, 1.5), (7, -0.1), (7, float("nan")), (8, 0.0), (8, -1.0), (8, float("nan")), (8, float("inf")),
                 (9, -0.1), (9, 1.1), (10, 0), (10, 9), (11, -0.1), (11, 1.1), (11, float("nan"))):
        a = list(good)
        a[k] = v
        assert lib.pbhc_start_sampling_update(*a, None) == E, (k, v)
    # pbhc_start_draw(cdf, clip_len, slot, reset (may be NULL), ovr_u (may be NULL), N, M, K, seed, counter, salt, start_time, stream)
    good = [p, p, p, None, None, 4, 2, 8, 1, p, 0, p]
    for k in (0, 1, 2, 9, 11):
        a = list(good)
        a[k] = None
        assert lib.pbhc_start_draw(*a, None) == E
        assert b"pbhc_start_draw" in lib.pbhc_last_error()
    for k, v in ((5, 0), (6, 0), (7, 0), (7, 129)):
        a = list(good)
        a[k] = v
        assert lib.pbhc_start_draw(*a, None) == E, (k, v)


class _FakeLib:
    """stands in for the motion library: records what the update is handed"""

    def __init__(self):
        self.calls = []

    def update_start_sampling_device(self, window, *rule):
        self.calls.append((window.clone(), rule))
        window.zero_()


def _fold_env(sampling):
    env = LeggedRobotMotionTracking.__new__(LeggedRobotMotionTracking)
    env._is_evaluating, env._start_suspended, env._fin_pending, env._start_time = False, False, False, None
    env._start = dict(statistics=True, sampling=sampling, **DEFAULTS)
    env._start_window = torch.arange(2 * 4 * 2, dtype=torch.int64).reshape(2, 4, 2).clone()
    env._motion_lib = _FakeLib()
    return env


def test_the_fold_sums_the_window_over_the_group_before_the_update(monkeypatch):
    other = torch.full((2, 4, 2), 100, dtype=torch.int64)
    seen = []

    def fake_all_reduce(t, group=None, **kw):
        seen.append((t.dtype, tuple(t.shape), group))
        t.add_(other)

    monkeypatch.setattr(pdist, "active", lambda group: group == "stats")
    monkeypatch.setattr(pdist, "all_reduce", fake_all_reduce)
    env = _fold_env(sampling=False)
    mine = env._start_window.clone()
    env._stat_group = "stats"
    assert env.update_start_sampling() is True
    assert seen == [(torch.int64, (2, 4, 2), "stats")]                       # ONE all-reduce, of the whole window
    (window, rule), = env._motion_lib.calls
    assert torch.equal(window, mine + other)                                 # the update is handed the SUM
    assert rule == (0.9, 1.0, 0.1, 4, 0.8)
    assert int(env._start_window.abs().sum()) == 0
    # no group: no collective, the update gets this rank's window
    env = _fold_env(sampling=False)
    mine = env._start_window.clone()
    env._stat_group = None
    seen.clear()
    env.update_start_sampling()
    assert seen == [] and torch.equal(env._motion_lib.calls[0][0], mine)
    # suspended by evaluation: nothing is folded
    env = _fold_env(sampling=False)
    env._stat_group, env._is_evaluating = "stats", True
    seen.clear()
    assert env.update_start_sampling() is False and seen == [] and env._motion_lib.calls == []


def test_public_calls_need_the_keys():
    env = LeggedRobotMotionTracking.__new__(LeggedRobotMotionTracking)
    env._start_window = None
    for call in (env.start_statistics, env.clear_start_statistics, env.update_start_sampling):
        with pytest.raises(_lib.PbhcError, match="start_statistics"):
            call()
