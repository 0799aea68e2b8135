"""env.config.clip_statistics / clip_sampling: the option resolver and the C ABI's argument checks (no GPU)."""
import ctypes as C
import os

import pytest

from pbhc_amd import _lib
from pbhc_amd.envs import env_config
from pbhc_amd.utils.config import load_config
from tests.helpers import GOLDEN


def _env_cfg(name, overrides=None):
    return load_config(os.path.join(GOLDEN, "configs", name), dict(overrides or {}), now="t").env.config


@pytest.mark.parametrize("name", ["v1_g1_23dof_walk.yaml", "v2_g1_29dof_teacher.yaml"])
def test_keys_absent_means_off(name):
    ec = _env_cfg(name)
    assert "clip_statistics" not in ec and "clip_sampling" not in ec
    o = env_config.clip_options(ec)
    assert o["statistics"] is False and o["sampling"] is False
    assert isinstance(o, dict) and type(o) is dict


def test_statistics_only_and_sampling_implies_statistics():
    o = env_config.clip_options(_env_cfg("v1_g1_23dof_walk.yaml", {"env.config.clip_statistics": True}))
    assert o["statistics"] is True and o["sampling"] is False
    o = env_config.clip_options(_env_cfg("v2_g1_29dof_teacher.yaml", {"env.config.clip_sampling": {"enable": True}}))
    assert o["statistics"] is True and o["sampling"] is True
    assert (o["decay"], o["prior_episodes"], o["uniform_floor"]) == (0.5, 1.0, 0.1)
    o = env_config.clip_options(_env_cfg("v2_g1_29dof_teacher.yaml", {"env.config.clip_sampling": {"enable": False, "decay": 0.0, "uniform_floor": 1.0,
                                                                                                   "prior_episodes": 3}}))
    assert o["statistics"] is False and o["sampling"] is False
    assert (o["decay"], o["prior_episodes"], o["uniform_floor"]) == (0.0, 3.0, 1.0)


@pytest.mark.parametrize("key,value", [("decay", -0.01), ("decay", 1.01), ("decay", float("nan")), ("prior_episodes", 0.0), ("prior_episodes", -1.0),
                                       ("prior_episodes", float("inf")), ("uniform_floor", -0.1), ("uniform_floor", 1.5), ("decay", "fast")])
def test_out_of_range_values_are_refused_and_the_message_names_the_key(key, value):
    ec = _env_cfg("v2_g1_29dof_teacher.yaml", {"env.config.clip_sampling": {"enable": True, key: value}})
    with pytest.raises(_lib.PbhcError, match=r"env\.config\.clip_sampling\." + key):
        env_config.clip_options(ec)


def test_unknown_key_is_refused():
    with pytest.raises(_lib.PbhcError, match="floor"):
        env_config.clip_options(_env_cfg("v2_g1_29dof_teacher.yaml", {"env.config.clip_sampling": {"enable": True, "floor": 0.1}}))


def test_null_and_bad_sizes_return_einval_without_a_gpu():
    lib, E = _lib.lib(), _lib.K["PBHC_EINVAL"]
    p = C.c_void_p(64)                 # never dereferenced: every call below is refused on the host
    assert lib.pbhc_clip_stats(None, None, None, None, None, 4, 1, None, None) == E
    assert b"pbhc_clip_stats" in lib.pbhc_last_error()
    for k in range(6):                 # each pointer on its own
        a = [p] * 5 + [4, 2] + [p]
        a[k if k < 5 else 7] = None
        assert lib.pbhc_clip_stats(*a, None) == E
    assert lib.pbhc_clip_stats(p, p, p, p, p, 0, 1, p, None) == E
    assert lib.pbhc_clip_stats(p, p, p, p, p, 4, 0, p, None) == E
    assert lib.pbhc_clip_sampling_update(None, None, None, None, None, None, 3, 0.5, 1.0, 0.1, None) == E
    for k in range(6):
        a = [p] * 6
        a[k] = None
        assert lib.pbhc_clip_sampling_update(*a, 3, 0.5, 1.0, 0.1, None) == E
    assert lib.pbhc_clip_sampling_update(p, p, p, p, p, p, 0, 0.5, 1.0, 0.1, None) == E
    for bad in ((1.5, 1.0, 0.1), (0.5, 0.0, 0.1), (0.5, 1.0, -0.1), (float("nan"), 1.0, 0.1)):
        assert lib.pbhc_clip_sampling_update(p, p, p, p, p, p, 3, *bad, None) == E
    assert lib.pbhc_clip_sample_slots(None, 3, 1, 0, None, 4, None) == E
    assert lib.pbhc_clip_sample_slots(None, 3, 1, 0, p, 4, None) == E
    assert lib.pbhc_clip_sample_slots(p, 3, 1, 0, None, 4, None) == E
    assert lib.pbhc_clip_sample_slots(p, 0, 1, 0, p, 4, None) == E
    assert lib.pbhc_clip_sample_slots(p, 3, 1, 0, p, 0, None) == E
