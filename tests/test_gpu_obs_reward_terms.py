"""The radial-velocity reward terms and the observation keys future_ref_dof_pos / future_ref_dof_vel, local_ref_rigid_body_pos_relyaw,
feet_contact_force, indicator_guider, indicator_learner, zero_vector on the GPU: the reference's own traces with injected draws, a
plain-torch restatement at 4096 envs, exact no-ops, and the rollout graph."""
import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, build_hip_env, load_state_into_hip_env, state_dict_from_golden
from tests.test_gpu_parity import close
from tools.gen_obs_reward_terms_golden import FUTURE_REF_STEPS, ZERO_VECTOR, overrides

pytestmark = pytest.mark.gpu

WALK, STUDENT = "v1_g1_23dof_walk.yaml", "v2_g1_23dof_student.yaml"


def _names(cfgname, general):
    from pbhc_amd.utils.config import load_config

    return overrides(load_config(f"{GOLDEN}/configs/{cfgname}", {"num_envs": 4}, now="t"), general)


def _trace(tag, cfgname, general):
    """driven like test_env_step_matches_reference_trace; prints the largest residual of every quantity before asserting on it"""
    g = dict(np.load(f"{GOLDEN}/{tag}.npz"))
    T, N, D = g["actions_in"].shape
    cfg, env = build_hip_env(cfgname, N, general=general, overrides=dict({"domain_rand.push_robots": False}, **_names(cfgname, general)))
    assert env.reward_names == list(g["reward_names"])
    load_state_into_hip_env(env, state_dict_from_golden(g), g)
    tg = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.device)
    env.simulator.set_replay(tg(g["replay_root"]), tg(g["replay_dof_pos"]), tg(g["replay_dof_vel"]), tg(g["replay_contact"]))
    worst = {}

    def chk(mine, ref, tol, what, **kw):
        ref_t = torch.as_tensor(ref)
        d = (mine.detach().cpu().double() - ref_t.double()).abs()
        worst[what.split(": ")[-1]] = max(worst.get(what.split(": ")[-1], 0.0), float(d.max()))
        close(mine, ref, tol, what, **kw)

    try:
        for k in range(T):
            st = lambda name, dt=torch.float32: tg(g["step__state__" + name][k]).to(dt)
            env.set_injected_draws(u_rfi=tg(g["step__u_rfi"][k]), start_time=st("motion_start_times"), kp=st("kp_scale"), kd=st("kd_scale"),
                                   rfi_lim=st("rfi_lim_scale"), rao=st("rao_scale"), delay=st("action_delay_idx", torch.long))
            obs, rew, reset, extras = env.step({"actions": tg(g["actions_in"][k])})
            torch.cuda.synchronize()
            w = f"{tag} step {k}: "
            assert torch.equal(reset.cpu(), torch.from_numpy(g["step__reset_buf_out"][k])), w + "reset_buf"
            assert torch.equal(env.episode_length_buf.cpu(), torch.from_numpy(g["step__state__episode_length_buf"][k])), w + "episode_length_buf"
            chk(rew, g["step__rew_buf"][k], 3e-5, w + "rew_buf", rtol=1e-4)
            for ok in obs:
                if general:         # (slerp-conditioned elements of the v2 rows: the bound tests/test_gpu_parity_v2.py derives per element)
                    chk(obs[ok], g["step__obs__" + ok][k], 3e-5, w + ok, hard=2e-3, frac=0.02)
                else:
                    chk(obs[ok], g["step__obs__" + ok][k], 3e-5, w + ok)
            for name in ["feet_air_time", "last_contacts", "contacts_filt"]:
                chk(getattr(env, name), g["step__state__" + name][k], 3e-5, w + "state " + name)
            for name, col in env.episode_sums.items():
                chk(col, g["step__state__sum__" + name][k], 3e-5, w + "sum " + name, rtol=1e-4)
    finally:
        print(tag, "largest residuals:", {k: f"{v:.3g}" for k, v in worst.items()})
    return cfg, g


def test_v1_trace_with_all_names():
    cfg, g = _trace("env_v1_walk_terms", WALK, False)
    sl = _slices(cfg, "actor_obs")
    a = g["step__obs__actor_obs"]
    assert np.abs(a[..., sl["future_ref_dof_pos"][0]:sl["future_ref_dof_pos"][1]]).max() > 0.1
    assert (a[..., sl["indicator_guider"][0]] == 1.0).all()


def test_v2_trace_with_relyaw_and_feet_contact_force():
    _trace("env_v2_student23_terms", STUDENT, True)


def _slices(cfg, group):
    """column range of every key of an observation group (the reference's sorted-key layout, helpers.py)"""
    from pbhc_amd.envs.env_config import flatten_obs_dims

    dims = flatten_obs_dims(cfg.obs)
    aux = {k: sum(dims[kk] * n for kk, n in a.items()) for k, a in cfg.obs.obs_auxiliary.items()}
    out, o = {}, 0
    for k in sorted(cfg.obs.obs_dict[group]):
        n = dims[k] if k in dims else aux[k]
        out[k] = (o, o + n)
        o += n
    return out


def _env_4096(ov, seed=3, N=4096):
    """walk env at 4096 envs on a seeded replay.  Every start time — those of reset_all and, injected, those a reset draws — lies in
    [0.5 s, clip length - 1 s]: off the clip's rest frames, where the reference joint velocities are exactly zero and the reference's radial
    potential is NaN (no test feeds that case).  A quarter of the envs time out in the first step."""
    import bench

    torch.manual_seed(seed)
    np.random.seed(seed)
    cfg, env = build_hip_env(WALK, N, overrides=ov)
    torch.manual_seed(seed + 1)
    env.reset_all()
    g = torch.Generator(device="cpu").manual_seed(seed + 2)
    L = float(env.motion_len[0])
    draw = lambda: (0.5 + (L - 1.5) * torch.rand(N, generator=g)).to(env.device)
    env.motion_start_times.copy_(draw())
    env.simulator.set_replay(*[t.contiguous() for t in bench.make_replay_on_device(env, 4, seed=5)])
    env._episode_length_buf[::4] = int(env.max_episode_length) + 1
    return cfg, env, draw


def _outputs(env, obs, rew, reset):
    out = {"obs__" + k: v.clone() for k, v in obs.items()}
    out.update(rew=rew.clone(), reset=reset.clone(), root=env.simulator.robot_root_states.clone(), dof_pos=env.simulator.dof_pos.clone(),
               kp=env._kp_scale.clone(), kd=env._kd_scale.clone(), rao=env._rao_scale.clone(), rfi=env._rfi_lim_scale.clone(),
               torques=env.torques.clone(), start=env.motion_start_times.clone(), hist=env._hist.clone(), ep=env.episode_length_buf.clone(),
               sums=env._episode_sums.clone(), feet_air_time=env.feet_air_time.clone(), last_contacts=env.last_contacts.clone(),
               contacts_filt=env.contacts_filt.clone(), actions=env.actions.clone(), last_dof_vel=env.last_dof_vel.clone())
    return out


def _run(ov, steps=3):
    cfg, env, draw = _env_4096(ov)
    outs = []
    for _ in range(steps):
        env.set_injected_draws(start_time=draw())
        outs.append(_outputs(env, *env.step({"actions": 0.3 * torch.ones(env.num_envs, env.num_dof, device=env.device)})[:3]))
    torch.cuda.synchronize()
    assert bool(outs[0]["reset"].bool().any())
    return cfg, env, outs


def _radial_potential(cur, ref):
    """motion_tracking.py:78-94 in plain torch"""
    cs = torch.nn.functional.cosine_similarity(cur, ref, dim=-1)
    r = cur.norm(dim=-1) / ref.norm(dim=-1)
    return torch.exp(-(1 - cs) / 0.75) * (r * torch.exp(0.4 * (1 - r ** 2.5)))


def _quat_rotate(q, v):
    """isaac_utils rotations.py my_quat_rotate, xyzw"""
    w, u = q[..., 3:4], q[..., :3]
    return v * (2.0 * w ** 2 - 1.0) + torch.cross(u, v, dim=-1) * w * 2.0 + u * (u * v).sum(-1, keepdim=True) * 2.0


def test_restatement_4096():
    """three steps at 4096 envs, all names on: every new observation block and both radial reward columns restated in plain torch from the
    env's own exposed tensors (simulator views, the motion library, the config), for the envs that kept their state in the step (a reset
    replaces the simulator state the restatement reads; the look-ahead and constant blocks are checked for every env).  3e-5 on
    observation rows, 3e-5 + 1e-4 relative on reward columns."""
    cfg, env, draw = _env_4096(_names(WALK, False))
    sla, slc = _slices(cfg, "actor_obs"), _slices(cfg, "critic_obs")
    N, D, B, dev = env.num_envs, env.num_dof, env.num_bodies, env.device
    Bx = B + env.num_extend_bodies
    clipv = float(cfg.env.config.normalization.clip_observations)
    names = list(env.body_names)
    ext = [dict(e) for e in cfg.robot.motion.extend_config]
    parents = torch.tensor([names.index(e["parent_name"]) for e in ext], device=dev)
    offs = torch.tensor([e["pos"] for e in ext], dtype=torch.float32, device=dev)
    ids = torch.zeros(N, dtype=torch.long, device=dev)
    resets = 0
    for _ in range(3):
        ep0, start0 = env.episode_length_buf.clone(), env.motion_start_times.clone()
        env.set_injected_draws(start_time=draw())
        obs, rew, reset, extras = env.step({"actions": 0.3 * torch.ones(N, D, device=dev)})
        torch.cuda.synchronize()
        keep = ~reset.bool()
        resets += int(reset.sum())
        a, c = obs["actor_obs"], obs["critic_obs"]
        assert bool(torch.isfinite(rew).all()) and bool(torch.isfinite(a).all()) and bool(torch.isfinite(c).all())
        assert bool((a[:, sla["indicator_guider"][0]] == 1.0).all())
        assert bool((c[:, slc["indicator_learner"][0]] == 0.0).all())
        z0, z1 = slc["zero_vector"]
        assert z1 - z0 == ZERO_VECTOR and bool((c[:, z0:z1] == 0.0).all())
        f0, f1 = slc["feet_contact_force"]
        feet = torch.as_tensor(env.layout.feet, device=dev)
        cf = env.simulator.contact_forces[:, feet, :].reshape(N, -1)
        close(c[:, f0:f1], (cf * float(cfg.obs.obs_scales["feet_contact_force"])).clamp(-clipv, clipv).cpu().numpy(), 3e-5, "feet_contact_force")
        # the look-ahead joint rows: the motion library at (episode_length + 1 + i) dt + start of the state BEFORE the step's reset (the step
        # advances episode_length_buf first)
        p0, _ = sla["future_ref_dof_pos"]
        v0, _ = sla["future_ref_dof_vel"]
        tref = lambda i: (ep0 + 2 + i).float() * float(env.dt) + start0
        for i in range(FUTURE_REF_STEPS):
            ref = env._motion_lib.get_motion_state(ids, tref(i))
            close(a[:, p0 + i * D:p0 + (i + 1) * D], ref["dof_pos"].cpu().numpy(), 3e-5, f"future_ref_dof_pos step {i}")
            close(a[:, v0 + i * D:v0 + (i + 1) * D], (ref["dof_vel"] * float(cfg.obs.obs_scales["future_ref_dof_vel"])).cpu().numpy(), 3e-5,
                  f"future_ref_dof_vel step {i}")
        ref = env._motion_lib.get_motion_state(ids, tref(0))
        ref_bv = ref["body_vel_t"]                                               # [N, Bx, 3] reference velocities of the extended bodies
        assert ref_bv.shape == (N, Bx, 3)
        # local_ref_rigid_body_pos_relyaw (motion_tracking.py:684-685,720-721): calc_yaw_heading_quat_inv(yaw - ref_init_yaw) applied to the
        # reference body VELOCITIES.  yaw: get_euler_xyz's z of the root quaternion (xyzw)
        q = env.simulator.robot_root_states[:, 3:7]
        yaw = torch.atan2(2.0 * (q[:, 3] * q[:, 2] + q[:, 0] * q[:, 1]), q[:, 3] ** 2 + q[:, 0] ** 2 - q[:, 1] ** 2 - q[:, 2] ** 2)
        half = (yaw - env.ref_init_yaw) * 0.5
        qi = torch.stack([torch.zeros_like(half), torch.zeros_like(half), -torch.sin(half), torch.cos(half)], -1)
        want = _quat_rotate(qi[:, None, :].expand(N, Bx, 4), ref_bv).reshape(N, -1) * float(cfg.obs.obs_scales["local_ref_rigid_body_pos_relyaw"])
        r0, r1 = sla["local_ref_rigid_body_pos_relyaw"]
        assert r1 - r0 == 3 * Bx
        close(a[keep, r0:r1], want.clamp(-clipv, clipv)[keep].cpu().numpy(), 3e-5, "local_ref_rigid_body_pos_relyaw")
        # the radial columns (motion_tracking.py:1238-1244,1286-1292): cur = the simulator's velocities, ref = (reference - cur) + cur
        cur_j = env.simulator.dof_vel
        bv, bw = env.simulator._rigid_body_vel, env.simulator._rigid_body_ang_vel
        cur_b = torch.cat([bv, bv[:, parents] + torch.cross(bw[:, parents], offs[None].expand(N, -1, -1), dim=2)], 1).reshape(N, -1)   # :641-643
        for n, cur, rf in (("teleop_radial_joint_velocity", cur_j, ref["dof_vel"]), ("teleop_radial_body_velocity_extend", cur_b, ref_bv.reshape(N, -1))):
            want = (_radial_potential(cur, (rf - cur) + cur) * env.layout.reward_scales[n])[keep]
            assert bool(torch.isfinite(want).all()), n
            close(rew[:, env.reward_names.index(n)][keep], want.cpu().numpy(), 3e-5, n, rtol=1e-4)
    assert resets > N // 8


def test_no_name_equals_neutral_names_bit_for_bit():
    """zero_vector / indicator_learner appended to critic_obs leave actor_obs and every state buffer bit-identical; a reward term at scale 0
    builds the same config as its absence"""
    from pbhc_amd.utils.config import load_config

    cfg0 = load_config(f"{GOLDEN}/configs/{WALK}", {"num_envs": 4}, now="t")
    neutral = {"obs.obs_dict.critic_obs": list(cfg0.obs.obs_dict.critic_obs) + ["zero_vector", "indicator_learner"],
               "obs.obs_dims": [dict(d) for d in cfg0.obs.obs_dims] + [{"zero_vector": 3}, {"indicator_learner": 1}],
               "obs.obs_scales.zero_vector": 1.0, "obs.noise_scales.zero_vector": 0.0, "obs.obs_scales.indicator_learner": 1.0,
               "obs.noise_scales.indicator_learner": 0.0,
               "rewards.reward_scales.teleop_radial_body_velocity_extend": 0, "rewards.reward_scales.teleop_radial_joint_velocity": 0}
    _, _, a = _run({})
    _, env, b = _run(neutral)
    assert env._c.radial_terms == 0 and env._c.obs_extra == 0
    for x, y in zip(a, b):
        for k in x:
            if k == "obs__critic_obs":
                continue
            assert torch.equal(x[k], y[k]), k


def test_graph_rollout_with_all_names_equals_the_eager_loop(monkeypatch):
    """the 24-step rollout as one hipGraph against the step-by-step loop, MHPPO on v1, all names on"""
    import tests.test_gpu_parity as P

    orig = P.build_hip_env

    def build(*a, **k):
        cfgname = a[0] if a else k["cfgname"]
        return orig(*a, **dict(k, overrides=dict(k.get("overrides") or {}, **_names(cfgname, False))))

    monkeypatch.setattr(P, "build_hip_env", build)
    a = P._rollouts_with_split(True, "v1", batched=True, fused_sample=True, rollout_graph=True, rollouts=4)
    b = P._rollouts_with_split(True, "v1", batched=True, fused_sample=True, rollout_graph=False, rollouts=4)
    a.pop("_time_outs_seen"); b.pop("_time_outs_seen")
    assert bool(a.pop("_used_graph")) and not bool(b.pop("_used_graph"))
    a.pop("_used_graph_each"); b.pop("_used_graph_each")
    # The rollout draws its own start times and runs envs into their clip's end, so some lookups land on frames whose reference joint
    # velocities are exactly zero: the reference's own radial formula is NaN there, and through the batch normalisation of the advantages
    # one such reward reaches whole buffers.  The comparison therefore is: the NaN masks of the two runs are the same, and every other
    # entry is equal bit for bit; the masked counts are printed.  (Confining the start times to [0.5 s, 1 s] through reset_all and the
    # injected reset draws did not keep this rollout finite; the 4096-env restatement above runs on finite inputs only.)
    masked = {}
    for k in a:
        x, y = a[k], b[k]
        if x.is_floating_point():
            mx, my = torch.isnan(x), torch.isnan(y)
            assert torch.equal(mx, my), k
            if bool(mx.any()):
                masked[k] = f"{int(mx.sum())} of {mx.numel()}"
            x, y = x[~mx], y[~my]
        assert torch.equal(x, y), k
    print("entries NaN in both runs:", masked)
