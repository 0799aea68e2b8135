"""obs.noise_process (OU IMU noise) and domain_rand.parallel_serial_pd / parallel_serial_tau at the config level (no GPU): what
env_config.build puts into the ABI, what it refuses, and that the switches off leave the config as it was."""
import ctypes as C

import numpy as np
import pytest

from pbhc_amd import _lib
from tests.helpers import build_env_config

K = _lib.K
OU = {"obs.noise_process.enable": True, "obs.noise_process.type": "ou", "obs.noise_process.kwargs.mu": 0.1,
      "obs.noise_process.kwargs.sigma": 2.0, "obs.noise_process.kwargs.theta": 0.5, "obs.noise_process.scale.rpy": 3.0,
      "obs.noise_process.scale.base_ang_vel": 0.4}
PS_PD = {"domain_rand.parallel_serial_pd.enable": True, "domain_rand.parallel_serial_pd.ratio": [0.8, 1.2],
         "domain_rand.parallel_serial_pd.joint_idx": [4, 5, 10, 11, 13, 14]}
PS_TAU = {"domain_rand.parallel_serial_tau.enable": True, "domain_rand.parallel_serial_tau.joint_idx": [5, 11, 4],
          "domain_rand.parallel_serial_tau.rao_lim": 0.03, "domain_rand.parallel_serial_tau.rfi_lim": 0.05}
NOISE_NAMES = ["base_ang_vel_noise", "projected_gravity_noise", "dof_pos_noise", "dof_vel_noise"]
NEW_FIELDS = {"noise_process", "ou_mu", "ou_theta", "ou_sigma", "ou_sqrt_dt", "ou_sqrt_2theta", "ou_scale_rpy", "ou_scale_ang_vel", "ps_pd",
              "ps_pd_num", "ps_pd_slot", "ps_pd_ratio", "ps_tau", "ps_tau_num", "ps_tau_slot", "ps_tau_rao_lim", "ps_tau_rfi_lim"}
CONFIGS = [("v1_g1_23dof_walk.yaml", 0), ("v2_g1_23dof_student.yaml", 1), ("v2_g1_23dof_teacher.yaml", 1), ("v2_g1_29dof_teacher.yaml", 1)]


def add_noise_names(cfg):
    """the four names in actor_obs (+ their dims / scales, as a yaml that uses them lists them)"""
    ob = cfg.obs
    ob.obs_dict.actor_obs = list(ob.obs_dict.actor_obs) + NOISE_NAMES
    D = len(cfg.robot.dof_names)
    ob.obs_dims = list(ob.obs_dims) + [{"base_ang_vel_noise": 3}, {"projected_gravity_noise": 3}, {"dof_pos_noise": D}, {"dof_vel_noise": D}]
    for k in NOISE_NAMES:
        ob.obs_scales[k] = 1.0
        ob.noise_scales[k] = 0.0


def _build(cfgname, overrides, mode, noise_names=False):
    cfg, _, c, L = build_env_config(cfgname, overrides, num_envs=64, seed=1, general=mode == 1, has_contact_mask=False,
                                    mutate=add_noise_names if noise_names else None)
    return cfg, (c, L)


def _fields(c):
    out = {}
    for name, ct in type(c)._fields_:
        v = getattr(c, name)
        if isinstance(v, C.Structure):
            out.update({name + "." + k: x for k, x in _fields(v).items()})
        elif isinstance(v, C.Array):
            out[name] = bytes(v) if not isinstance(v[0], C.Structure) else [_fields(x) for x in v]
        else:
            out[name] = v
    return out


@pytest.mark.parametrize("cfgname,mode", [CONFIGS[0], CONFIGS[1]])
def test_build_accepts_the_three_switches_and_the_four_names(cfgname, mode):
    cfg, (c, L) = _build(cfgname, dict(OU, **PS_PD, **PS_TAU), mode, noise_names=True)
    assert c.noise_process == 1
    f = lambda x: float(np.float32(x))
    assert (c.ou_mu, c.ou_sigma, c.ou_theta, c.ou_scale_rpy, c.ou_scale_ang_vel) == (f(0.1), 2.0, 0.5, 3.0, f(0.4))
    assert c.ou_sqrt_dt == f(np.sqrt(4 / 200)) and c.ou_sqrt_2theta == 1.0
    assert c.ps_pd == 1 and c.ps_pd_num == 6 and (c.ps_pd_ratio[0], c.ps_pd_ratio[1]) == (f(0.8), f(1.2))
    assert [c.ps_pd_slot[i] for i in range(16)] == [-1, -1, -1, -1, 0, 1, -1, -1, -1, -1, 2, 3, -1, 4, 5, -1]
    assert c.ps_tau == 1 and c.ps_tau_num == 3 and (c.ps_tau_rao_lim, c.ps_tau_rfi_lim) == (f(0.03), f(0.05))
    assert [c.ps_tau_slot[i] for i in (4, 5, 11, 0, 10)] == [2, 0, 1, -1, -1]           # the column of the [N, J] draws: the list's order
    assert L.ps_pd_idx == [4, 5, 10, 11, 13, 14] and L.ps_tau_idx == [5, 11, 4]
    # the two root-frame names read features of their own; dof_*_noise the clean joint values
    assert "BASE_ANG_VEL_NOISE" in L.feat_off and "PROJECTED_GRAVITY_NOISE" in L.feat_off
    assert c.feat_off[K["PBHC_F_BASE_ANG_VEL_NOISE"]] != c.feat_off[K["PBHC_F_BASE_ANG_VEL"]]
    assert _lib.lib().pbhc_env_config_lds_bytes(c) > 0                # the library accepts the config (ABI layout agrees)


@pytest.mark.parametrize("cfgname,mode", [CONFIGS[0], CONFIGS[1]])
def test_noise_names_without_the_process_read_the_clean_features(cfgname, mode):
    _, (c, L) = _build(cfgname, {}, mode, noise_names=True)
    assert c.noise_process == 0 and "BASE_ANG_VEL_NOISE" not in L.feat_off
    assert _lib.lib().pbhc_env_config_lds_bytes(c) > 0


@pytest.mark.parametrize("typ", ["white", "empty", "pink", "brown"])
def test_noise_process_types_other_than_ou_are_refused(typ):
    with pytest.raises(NotImplementedError, match="reset_part"):
        _build("v1_g1_23dof_walk.yaml", dict(OU, **{"obs.noise_process.type": typ}), 0)


@pytest.mark.parametrize("block,idx", [("parallel_serial_pd", [4, 23]), ("parallel_serial_tau", [40]), ("parallel_serial_pd", [-24])])
def test_out_of_range_joint_idx_is_refused(block, idx):
    ov = dict(PS_PD if block == "parallel_serial_pd" else PS_TAU, **{f"domain_rand.{block}.joint_idx": idx})
    with pytest.raises(IndexError, match="out of range"):
        _build("v1_g1_23dof_walk.yaml", ov, 0)


def test_negative_joint_idx_wraps_and_repeats_are_refused():
    _, (c, L) = _build("v1_g1_23dof_walk.yaml", dict(PS_PD, **{"domain_rand.parallel_serial_pd.joint_idx": [-1, 0]}), 0)
    assert L.ps_pd_idx == [22, 0] and c.ps_pd_slot[22] == 0
    with pytest.raises(ValueError, match="twice"):
        _build("v1_g1_23dof_walk.yaml", dict(PS_TAU, **{"domain_rand.parallel_serial_tau.joint_idx": [3, 3]}), 0)


@pytest.mark.parametrize("cfgname,mode", CONFIGS)
def test_switches_absent_or_disabled_leave_the_config_as_it_was(cfgname, mode):
    _, (a, La) = _build(cfgname, {}, mode)
    off = {k: v for k, v in dict(OU, **PS_PD, **PS_TAU).items() if not k.endswith(".enable")}
    off.update({"obs.noise_process.enable": False, "domain_rand.parallel_serial_pd.enable": False, "domain_rand.parallel_serial_tau.enable": False})
    _, (b, Lb) = _build(cfgname, off, mode)
    fa, fb = _fields(a), _fields(b)
    for k in fa:
        if k in ("map_image", "groups"):                               # device addresses / per-build pointers
            continue
        assert fa[k] == fb[k], k
    assert La.feat_off == Lb.feat_off and a.feat_dim == b.feat_dim and np.array_equal(La.globals0, Lb.globals0)
    # the new members hold their off values: no switch, no slot, and no feature of the process in the row
    assert a.noise_process == 0 and a.ps_pd == 0 and a.ps_tau == 0
    assert all(a.ps_pd_slot[i] == -1 and a.ps_tau_slot[i] == -1 for i in range(K["PBHC_MAX_DOF"]))
    assert "BASE_ANG_VEL_NOISE" not in La.feat_off and "PROJECTED_GRAVITY_NOISE" not in La.feat_off
    # the clean features' offsets and the row width are those of the feature table without the two new slots
    fo = {k: v for k, v in La.feat_off.items()}
    assert max(o + La.feat_dim_each[n] for n, o in fo.items()) == a.feat_dim
