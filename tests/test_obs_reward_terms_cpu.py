"""The reward terms teleop_radial_body_velocity_extend / teleop_radial_joint_velocity and the observation keys future_ref_dof_pos /
future_ref_dof_vel, local_ref_rigid_body_pos_relyaw, feet_contact_force, indicator_guider, indicator_learner, zero_vector: what
env_config.build resolves them to, what it refuses, that nothing moves when no such name is configured, and the conditions the reference
traces must meet to exercise them (tools/gen_obs_reward_terms_golden.py)."""
import hashlib

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, build_env_config
from tools.gen_obs_reward_terms_golden import FUTURE_REF_STEPS, RADIAL, V1_ACTOR, V1_CRITIC, V2_ACTOR, ZERO_VECTOR, overrides

WALK, HORSE, STUDENT, TEACHER = "v1_g1_23dof_walk.yaml", "v1_g1_23dof_horse_stance.yaml", "v2_g1_23dof_student.yaml", "v2_g1_29dof_teacher.yaml"


BASE = {"num_envs": 4, "simulator._target_": "pbhc_amd.simulator.replay_stub.ReplaySimStub"}


def _build(cfgname, general, ov=None, names=False):
    from pbhc_amd.utils.config import load_config

    o = dict(overrides(load_config(f"{GOLDEN}/configs/{cfgname}", dict(BASE), now="t"), general) if names else {}, **(ov or {}))
    return build_env_config(cfgname, o, num_envs=4, seed=1, general=general, has_contact_mask=True)


def _add_obs(cfgname, key, dim, group="actor_obs", extra=None):
    from pbhc_amd.utils.config import load_config

    cfg = load_config(f"{GOLDEN}/configs/{cfgname}", {"num_envs": 4}, now="t")
    ov = {"obs.obs_dict." + group: list(cfg.obs.obs_dict[group]) + [key], "obs.obs_dims": [dict(d) for d in cfg.obs.obs_dims] + [{key: dim}],
          "obs.obs_scales." + key: 1.0, "obs.noise_scales." + key: 0.0}
    return dict(ov, **(extra or {}))


def test_v1_names_resolve_to_ids_dims_and_sources():
    from pbhc_amd._lib import K

    cfg, skel, c, L = _build(WALK, False, names=True)
    D, Bx = skel.num_dof, skel.num_bodies_ext
    ids = [c.term_id[i] for i in range(c.num_terms)]
    assert K["PBHC_R_TELEOP_RADIAL_BODY_VELOCITY_EXTEND"] in ids and K["PBHC_R_TELEOP_RADIAL_JOINT_VELOCITY"] in ids
    assert c.radial_terms == 3 and c.obs_extra == 7 and c.future_ref_steps == FUTURE_REF_STEPS
    for n in RADIAL:
        assert abs(c.term_scale[L.reward_names.index(n)] - RADIAL[n] * L.dt) < 1e-9
    from pbhc_amd.envs.env_config import TERM_SIGMAS
    assert not set(RADIAL) & set(TERM_SIGMAS)
    fo, fd = L.feat_off, L.feat_dim_each
    assert fd["FUT_REF_DOF_POS"] == fd["FUT_REF_DOF_VEL"] == FUTURE_REF_STEPS * D and fd["REF_VEL_RELYAW"] == 3 * Bx and fd["FEET_CONTACT_FORCE"] == 6
    for f in ("ONE", "FEET_CONTACT_FORCE", "REF_VEL_RELYAW", "FUT_REF_DOF_POS", "FUT_REF_DOF_VEL", "RELYAW", "ZERO"):
        assert f in fo and c.feat_off[K["PBHC_F_" + f]] == fo[f]
    # source indices, in the reference's sorted-key order of each group
    def sources(group, key):
        keys = sorted(cfg.obs.obs_dict[group])
        from pbhc_amd.envs.env_config import flatten_obs_dims
        dims = flatten_obs_dims(cfg.obs)
        aux = {k: sum(dims[kk] * n for kk, n in a.items()) for k, a in cfg.obs.obs_auxiliary.items()}
        o = sum(dims[k] if k in dims else aux[k] for k in keys[:keys.index(key)])
        src = L.map_tensors[L.group_names.index(group)][1]
        return src[o:o + dims[key]].tolist()
    assert sources("actor_obs", "future_ref_dof_pos") == list(range(fo["FUT_REF_DOF_POS"], fo["FUT_REF_DOF_POS"] + FUTURE_REF_STEPS * D))
    assert sources("actor_obs", "future_ref_dof_vel") == list(range(fo["FUT_REF_DOF_VEL"], fo["FUT_REF_DOF_VEL"] + FUTURE_REF_STEPS * D))
    assert sources("actor_obs", "local_ref_rigid_body_pos_relyaw") == list(range(fo["REF_VEL_RELYAW"], fo["REF_VEL_RELYAW"] + 3 * Bx))
    assert sources("actor_obs", "indicator_guider") == [fo["ONE"]]
    assert sources("critic_obs", "indicator_learner") == [fo["ZERO"]]
    assert sources("critic_obs", "zero_vector") == [fo["ZERO"]] * ZERO_VECTOR
    assert sources("critic_obs", "feet_contact_force") == list(range(fo["FEET_CONTACT_FORCE"], fo["FEET_CONTACT_FORCE"] + 6))
    assert set(V1_ACTOR) <= set(cfg.obs.obs_dict.actor_obs) and set(V1_CRITIC) <= set(cfg.obs.obs_dict.critic_obs)


def test_v2_names_resolve():
    cfg, skel, c, L = _build(STUDENT, True, names=True)
    assert c.obs_extra == 6 and c.radial_terms == 0 and c.future_ref_steps == 0
    assert set(V2_ACTOR) <= set(cfg.obs.obs_dict.actor_obs) and "RELYAW" in L.feat_off


@pytest.mark.parametrize("key,dim", [("feet_contact_force", 6), ("local_ref_rigid_body_pos_relyaw", None), ("indicator_guider", 1), ("indicator_learner", 1),
                                     ("zero_vector", 5)])
def test_each_observation_name_alone_builds(key, dim):
    base = _build(WALK, False)[3]
    dim = dim if dim is not None else 3 * 27
    cfg, skel, c, L = _build(WALK, False, ov=_add_obs(WALK, key, dim))
    assert L.group_dims["actor_obs"] == base.group_dims["actor_obs"] + dim and L.group_dims["critic_obs"] == base.group_dims["critic_obs"]
    feat = {"feet_contact_force": "FEET_CONTACT_FORCE", "local_ref_rigid_body_pos_relyaw": "REF_VEL_RELYAW", "indicator_guider": "ONE",
            "indicator_learner": "ZERO", "zero_vector": "ZERO"}[key]
    src = L.map_tensors[L.group_names.index("actor_obs")][1].tolist()
    lo = L.feat_off[feat]
    assert sum(lo <= s_ < lo + L.feat_dim_each[feat] for s_ in src) >= (dim if feat != "ZERO" else dim)
    assert c.obs_extra == {"FEET_CONTACT_FORCE": 2, "REF_VEL_RELYAW": 4, "ONE": 1, "ZERO": 0}[feat]


def test_refusals():
    from pbhc_amd._lib import PbhcError

    for n in RADIAL:                                                     # general_tracking.py does not define the radial terms
        with pytest.raises(NotImplementedError, match="no HIP implementation"):
            _build(STUDENT, True, ov={"rewards.reward_scales." + n: 1.0})
    with pytest.raises(NotImplementedError, match="cannot run it"):      # the reference raises TypeError on its first evaluation
        _build(WALK, False, ov={"rewards.reward_scales.feet_max_height_for_this_air": -1.0})
    D = 23
    with pytest.raises(PbhcError, match="future_ref_steps"):
        _build(WALK, False, ov=_add_obs(WALK, "future_ref_dof_pos", 3 * D))
    with pytest.raises(PbhcError, match="future_ref_steps"):
        _build(WALK, False, ov=_add_obs(WALK, "future_ref_dof_vel", 3 * D, extra={"obs.future_ref_steps": 0}))
    with pytest.raises(PbhcError, match="does not match"):
        _build(WALK, False, ov=_add_obs(WALK, "future_ref_dof_pos", 2 * D, extra={"obs.future_ref_steps": 3}))
    for key in ("indicator_guider", "zero_vector", "future_ref_dof_pos"):  # v1 getters only
        with pytest.raises(NotImplementedError, match="no HIP implementation"):
            _build(STUDENT, True, ov=_add_obs(STUDENT, key, 1))


@pytest.mark.parametrize("name", ["history", "short_history", "long_history"])
def test_history_names_build(name):
    """an obs_auxiliary entry called history / short_history / long_history goes through the generic branch of key_sources: its elements
    read the HISTORY block, in sorted-key order, scaled by the key's own scale"""
    from pbhc_amd.utils.config import load_config

    cfg0 = load_config(f"{GOLDEN}/configs/{WALK}", dict(BASE), now="t")
    spec = {"dof_pos": 2, "actions": 3}
    ov = {"obs.obs_auxiliary." + name: spec, "obs.obs_dict.actor_obs": list(cfg0.obs.obs_dict.actor_obs) + [name],
          "obs.obs_scales." + name: 1.0, "obs.noise_scales." + name: 0.0}
    cfg, skel, c, L = _build(WALK, False, ov=ov)
    D = skel.num_dof
    keys = sorted(cfg.obs.obs_dict.actor_obs)
    from pbhc_amd.envs.env_config import flatten_obs_dims
    dims = flatten_obs_dims(cfg.obs)
    aux = {k: sum(dims[kk] * n for kk, n in a.items()) for k, a in cfg.obs.obs_auxiliary.items()}
    assert aux[name] == 5 * D
    o = sum(dims[k] if k in dims else aux[k] for k in keys[:keys.index(name)])
    src = L.map_tensors[L.group_names.index("actor_obs")][1][o:o + 5 * D].tolist()
    h = L.feat_off["HISTORY"]
    want = list(range(h + L.hist_off["actions"], h + L.hist_off["actions"] + 3 * D)) + list(range(h + L.hist_off["dof_pos"], h + L.hist_off["dof_pos"] + 2 * D))
    assert src == want and L.hist_len["actions"] >= 3 and L.hist_len["dof_pos"] >= 2


# the layout every fixture config resolves to with no new name configured, recorded on the parent commit: feat_dim, the offsets of the
# features in use, the reward ids, and a digest of the map images
def _digest(c, L):
    h = hashlib.sha256()
    h.update(np.asarray([c.feat_dim, c.hist_dim, c.num_terms] + [c.term_id[i] for i in range(c.num_terms)], dtype=np.int64).tobytes())
    h.update(repr(sorted(L.feat_off.items())).encode())
    h.update(L.map_image.cpu().numpy().tobytes() if L.map_image is not None else b"")
    return h.hexdigest()[:16]


PARENT_LAYOUT = {WALK: "10db9b3f52d1707b", HORSE: "de2048aec965cddc", STUDENT: "fb48f368a102c8bd", TEACHER: "b3465910cdf2ceac"}


@pytest.mark.parametrize("cfgname,general", [(WALK, False), (HORSE, False), (STUDENT, True), (TEACHER, True)])
def test_layout_without_new_names_is_the_parents(cfgname, general):
    cfg, skel, c, L = _build(cfgname, general)
    assert c.obs_extra == 0 and c.radial_terms == 0 and c.future_ref_steps == 0
    assert not {"ONE", "FEET_CONTACT_FORCE", "REF_VEL_RELYAW", "FUT_REF_DOF_POS", "FUT_REF_DOF_VEL"} & set(L.feat_off)
    assert _digest(c, L) == PARENT_LAYOUT[cfgname], _digest(c, L)


def test_golden_conditions():
    g = np.load(f"{GOLDEN}/env_v1_walk_terms.npz")
    names = list(g["reward_names"])
    T, N = g["step__rew_buf"].shape[:2]
    assert N == 16 and g["step__reset_buf_out"].sum() > 0
    for n in RADIAL:
        col = g["step__rew_buf"][..., names.index(n)]
        if names.index(n) == len(names) - 1:                 # (the last term's column also carries the termination reward)
            col = col[g["step__reset_buf_out"] == 0]
            assert np.isfinite(col).all() and col.std() > 0
        else:
            assert np.isfinite(col).all() and (col.std(axis=1) > 0).all(), n
    assert np.isfinite(g["step__rew_buf"]).all()
    t_last = (g["step__state__episode_length_buf"][0] + 1 + FUTURE_REF_STEPS) * float(g["dt"]) + g["state0__motion_start_times"]
    assert (t_last > g["state0__motion_len"]).any()
    # an env that resets inside the window shows look-ahead rows in that very step (its old episode's), not zeros
    cfg, skel, c, L = _build(WALK, False, names=True)
    from pbhc_amd.envs.env_config import flatten_obs_dims
    dims = flatten_obs_dims(cfg.obs)
    aux = {k: sum(dims[kk] * n for kk, n in a_.items()) for k, a_ in cfg.obs.obs_auxiliary.items()}
    keys = sorted(cfg.obs.obs_dict.actor_obs)
    o = sum(dims[k] if k in dims else aux[k] for k in keys[:keys.index("future_ref_dof_pos")])
    fut = g["step__obs__actor_obs"][..., o:o + dims["future_ref_dof_pos"]]
    k_, e_ = np.nonzero(g["step__reset_buf_out"])
    assert len(k_) > 0 and all(np.abs(fut[k, e]).max() > 0.05 for k, e in zip(k_, e_))
    g2 = np.load(f"{GOLDEN}/env_v2_student23_terms.npz")
    assert g2["step__reset_buf_out"].sum() > 0
