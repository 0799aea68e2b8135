"""Reference traces of the reward terms teleop_radial_body_velocity_extend and teleop_radial_joint_velocity and of the observation keys future_ref_dof_pos / future_ref_dof_vel, local_ref_rigid_body_pos_relyaw, feet_contact_force, indicator_guider,
indicator_learner and zero_vector (build machine only: it runs the unmodified reference on CPU through oracle/ref_harness).

  tests/golden/env_v1_walk_terms.npz         v1, walk clip, 16 envs x 6 steps: the two radial terms, future_ref_steps = 3, every new key in
                                             actor_obs / critic_obs
  tests/golden/env_v2_student23_terms.npz    v2 student23, 16 envs x 6 steps: local_ref_rigid_body_pos_relyaw, feet_contact_force

(feet_max_height_for_this_air has no trace: the reference raises TypeError on the term's first evaluation, legged_robot_base.py:68,1022.)
The scripted replay of oracle/ref_harness/gen_env_golden resets envs inside the window (the look-ahead rows of such a step are the old
episode's), and env 1 starts 3.5 steps before its clip's end, so its look-ahead times run past it.  The per-step intermediates, logs and
reference bodies of the older traces are not written.

    PYTHONPATH=<repo> python tools/gen_obs_reward_terms_golden.py [v1] [v2]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
G1 = G2 = None                      # oracle.ref_harness.gen_env_golden / gen_env_v2_golden: imported by main (the tests import the settings only)


def _harness():
    global G1, G2
    from oracle.ref_harness import gen_env_golden, gen_env_v2_golden
    G1, G2 = gen_env_golden, gen_env_v2_golden

FUTURE_REF_STEPS = 3
ZERO_VECTOR = 4
RADIAL = {"teleop_radial_body_velocity_extend": 0.5, "teleop_radial_joint_velocity": 0.75}
OBS_SCALES = {"future_ref_dof_pos": 1.0, "future_ref_dof_vel": 0.05, "local_ref_rigid_body_pos_relyaw": 0.5, "feet_contact_force": 0.01,
              "indicator_guider": 1.0, "indicator_learner": 1.0, "zero_vector": 1.0}
V1_ACTOR = ["future_ref_dof_pos", "future_ref_dof_vel", "local_ref_rigid_body_pos_relyaw", "indicator_guider"]
V1_CRITIC = ["feet_contact_force", "indicator_learner", "zero_vector"]
V2_ACTOR = ["local_ref_rigid_body_pos_relyaw", "feet_contact_force"]


def obs_dims(names, D, Bx):
    d = {"future_ref_dof_pos": FUTURE_REF_STEPS * D, "future_ref_dof_vel": FUTURE_REF_STEPS * D, "local_ref_rigid_body_pos_relyaw": 3 * Bx,
         "feet_contact_force": 6, "indicator_guider": 1, "indicator_learner": 1, "zero_vector": ZERO_VECTOR}
    return {n: d[n] for n in names}


def overrides(cfg, general):
    """the names as load_config overrides of a fixture config (the GPU tests apply the same: tests/test_gpu_obs_reward_terms.py)"""
    D, Bx = len(cfg.robot.dof_names), len(cfg.robot.body_names) + len(cfg.robot.motion.extend_config)
    groups = {"actor_obs": V2_ACTOR} if general else {"actor_obs": V1_ACTOR, "critic_obs": V1_CRITIC}
    names = [n for g in groups.values() for n in g]
    ov = {"obs.obs_dict." + g: list(cfg.obs.obs_dict[g]) + add for g, add in groups.items()}
    ov["obs.obs_dims"] = [dict(d) for d in cfg.obs.obs_dims] + [{n: v} for n, v in obs_dims(names, D, Bx).items()]
    for n in names:
        ov["obs.obs_scales." + n] = OBS_SCALES[n]
        ov["obs.noise_scales." + n] = 0.0
    if not general:
        ov["obs.future_ref_steps"] = FUTURE_REF_STEPS
    if not general:
        for n, v in RADIAL.items():
            ov["rewards.reward_scales." + n] = v
    return ov


def configure(cfg, general):
    from pbhc_amd.utils.config import _wrap

    for k, v in overrides(cfg, general).items():
        node, parts = cfg, k.split(".")
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = _wrap(v) if isinstance(v, (dict, list)) else v


def _run(module, run, general):
    orig_build, orig_save, orig_replay = module.build_env, G1.G.save, G1.make_replay

    def make_replay(env, ml, T, seed, script=True):
        # the older traces start env 8 on the clip's first frame, where the reference joint velocities are exactly zero: the radial
        # potential is NaN there (inf x 0).  This trace starts it half a second in, before the replay is derived from the start times
        if not general:
            env.motion_start_times[8] = 0.5
        return orig_replay(env, ml, T, seed, script=script)

    def build_env(cfg, seed=0):
        configure(cfg, general)
        return orig_build(cfg, seed)

    saved = {}

    def save(name, **arrs):
        arrs = {k: v for k, v in arrs.items() if not k.startswith(("step__x__", "step__ref_body_", "step__log__"))}
        name = name.replace(".npz", "") + ".npz"
        saved["name"] = name
        return orig_save(name, **arrs)

    # the reference reads config.obs.obs_dims.zero_vector by ATTRIBUTE (motion_tracking.py:984): with OmegaConf the dict pre_process_config
    # stores there is a DictConfig; the harness's config nodes keep a plain dict, so it is wrapped the same way after that call
    from humanoidverse.utils import helpers as H
    from pbhc_amd.utils.config import _wrap
    orig_pre = H.pre_process_config

    def pre_process_config(cfg):
        out = orig_pre(cfg)
        cfg.env.config.obs.obs_dims = _wrap(dict(cfg.env.config.obs.obs_dims))
        return out

    module.build_env, G1.G.save, H.pre_process_config, G1.make_replay = build_env, save, pre_process_config, make_replay
    try:
        run()
    finally:
        module.build_env, G1.G.save, H.pre_process_config, G1.make_replay = orig_build, orig_save, orig_pre, orig_replay
    return saved["name"]


def check(name, general):
    """the conditions a trace must meet to exercise the names (asserted again by tests/test_obs_reward_terms_cpu.py)"""
    g = np.load(os.path.join(G1.G.GOLD, name))
    names = list(g["reward_names"])
    resets = g["step__reset_buf_out"]
    print(name, "resets per step:", resets.sum(1), "size", os.path.getsize(os.path.join(G1.G.GOLD, name)))
    assert resets.sum() > 0
    if not general:
        rew = g["step__rew_buf"]
        for n in RADIAL:
            col = rew[..., names.index(n)]
            assert np.isfinite(col).all() and col.std(axis=1).min() > 0, n
        t_last = (g["step__state__episode_length_buf"][0] + 1 + FUTURE_REF_STEPS) * float(g["dt"]) + g["state0__motion_start_times"]
        assert (t_last > g["state0__motion_len"]).any(), "no look-ahead time runs past its clip's end"
    return g


def v1():
    name = _run(G1, lambda: G1.run_trace(G1.V1_CFG, "walk_terms", N=16, T=6, motion_file="motion_data/g1_walk_45cms_23dof.pkl", extra=G1.WALK_EXTRA, seed=43),
                False)
    check(name, False)


def v2():
    def run():
        cwd = os.getcwd()
        try:
            G2.run_trace("student23", "student23_terms", N=16, T=6, seed=44)
        finally:
            os.chdir(cwd)

    check(_run(G2, run, True), True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["v1", "v2"]
    _harness()
    if "v1" in which:
        v1()
    if "v2" in which:
        v2()
