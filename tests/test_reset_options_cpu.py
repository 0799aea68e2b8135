"""termination.terminate_when_dof_far and noise_to_initial_level at the config level (no GPU): what env_config.build puts into the ABI."""
import numpy as np
import pytest

from pbhc_amd import _lib
from pbhc_amd.envs.motion_tracking import LeggedRobotMotionTracking
from tests.helpers import build_env_config

K = _lib.K
TC = "env.config.termination_curriculum.terminate_when_dof_far_curriculum."
DOF_FAR = {"env.config.termination.terminate_when_dof_far": True, TC + "enable": True, TC + "init": 2.0, TC + "degree": 0.05, TC + "min": 1.0,
           TC + "max": 2.5, TC + "level_down_threshold": 40, TC + "level_up_threshold": 42}
NOISE = {"env.config.noise_to_initial_level": 0.5}


def _build(cfgname, overrides, mode):
    cfg, _, c, L = build_env_config(cfgname, overrides, num_envs=64, seed=1, general=mode == 1, has_contact_mask=False)
    return cfg, (c, L)


def test_build_accepts_dof_far_and_reset_noise():
    cfg, (c, L) = _build("v1_g1_23dof_walk.yaml", dict(DOF_FAR, **NOISE), 0)
    assert c.terminate_when_dof_far == 1 and c.dof_far_curriculum == 1 and c.reset_noise == 1
    assert (c.dof_far_degree, c.dof_far_down, c.dof_far_up, c.dof_far_min, c.dof_far_max) == (np.float32(0.05), 40.0, 42.0, 1.0, 2.5)
    # the threshold starts at the curriculum's `init` (motion_tracking.py:128-130)
    assert L.globals0[K["PBHC_G_DOF_FAR_THR"]] == 2.0 and L.globals0[K["PBHC_G_DOF_FAR_HIT"]] == 0.0
    # scales x level, folded as the reference multiplies its python floats (float32 in the ABI)
    ns = cfg.env.config.init_noise_scale
    f = lambda x: float(np.float32(x))
    assert c.rn_root_pos == f(ns.root_pos * 0.5) and c.rn_root_vel == f(ns.root_vel * 0.5) and c.rn_root_ang_vel == f(ns.root_ang_vel * 0.5)
    assert c.rn_root_rot == f(ns.root_rot * 3.14 / 180 * 0.5)
    assert c.rn_dof_pos == f(ns.dof_pos * 0.5) and c.rn_dof_vel == f(ns.dof_vel * 0.5)
    assert _lib.lib().pbhc_env_config_lds_bytes(c) > 0                # the library accepts the config (ABI layout agrees)


def test_threshold_initialises_from_curriculum_init_when_curriculum_is_off():
    _, (c, L) = _build("v1_g1_23dof_walk.yaml", dict(DOF_FAR, **{TC + "enable": False, TC + "init": 1.7}), 0)
    assert c.terminate_when_dof_far == 1 and c.dof_far_curriculum == 0
    assert L.globals0[K["PBHC_G_DOF_FAR_THR"]] == 1.7


def test_switches_off_leave_the_config_as_it_was():
    _, (c, L) = _build("v1_g1_23dof_walk.yaml", {}, 0)
    assert c.terminate_when_dof_far == 0 and c.reset_noise == 0 and c.rn_dof_pos == 0.0
    assert L.globals0[K["PBHC_G_DOF_FAR_THR"]] == 0.0


def test_general_tracking_ignores_dof_far():
    """LeggedRobotGeneralTracking never reads termination.terminate_when_dof_far: accepted and ignored; its reset noise is configured"""
    _, (c, L) = _build("v2_g1_23dof_student.yaml", dict({"env.config.termination.terminate_when_dof_far": True}, **NOISE), 1)
    assert c.terminate_when_dof_far == 0 and c.reset_noise == 1


def test_data_parallel_dof_far_is_refused(monkeypatch):
    from pbhc_amd import dist as pdist

    class _Env:
        pass

    e = _Env()
    e._c = _lib.PbhcEnvConfig()
    e._c.terminate_when_dof_far = 1
    monkeypatch.setattr(pdist, "active", lambda group=None: True)
    with pytest.raises(NotImplementedError, match="collective"):
        LeggedRobotMotionTracking.enable_global_statistics(e, None)
