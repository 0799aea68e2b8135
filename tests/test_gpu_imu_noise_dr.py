"""obs.noise_process (the Ornstein-Uhlenbeck IMU noise: state stepped in phase C, redrawn in the reset path) and domain_rand.parallel_serial_pd /
parallel_serial_tau (at the episodic-DR sites and on the torque line) on the GPU: the reference's own traces with injected draws, exact no-ops,
the in-kernel distributions at 4096 envs, and the rollout graph."""
import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, build_hip_env, load_state_into_hip_env, state_dict_from_golden
from tests.test_gpu_parity import close

pytestmark = pytest.mark.gpu

WALK, STUDENT = "v1_g1_23dof_walk.yaml", "v2_g1_23dof_student.yaml"
# the settings of tools/gen_imu_noise_dr_golden.py
OU = {"enable": True, "type": "ou", "kwargs": {"mu": 0.05, "sigma": 0.6, "theta": 0.8}, "scale": {"rpy": 5.0, "base_ang_vel": 0.5}}
PS_PD = {"enable": True, "ratio": [0.8, 1.2], "joint_idx": [4, 5, 10, 11, 13, 14]}
PS_TAU = {"enable": True, "joint_idx": [4, 5, 10, 11], "rao_lim": 0.02, "rfi_lim": 0.05}
NOISE_SCALES = {"base_ang_vel_noise": 0.25, "projected_gravity_noise": 1.0, "dof_pos_noise": 1.0, "dof_vel_noise": 0.05}
ROOT2, ALL4 = ["base_ang_vel_noise", "projected_gravity_noise"], list(NOISE_SCALES)


def _names(cfgname, names, scales=None):
    """load_config overrides that add observation names to actor_obs (dims, scales, zero noise scales), as a yaml that uses them lists them"""
    from pbhc_amd.utils.config import load_config

    cfg = load_config(f"{GOLDEN}/configs/{cfgname}", {"num_envs": 4}, now="t")
    D = len(cfg.robot.dof_names)
    dims = {"base_ang_vel_noise": 3, "projected_gravity_noise": 3, "dof_pos_noise": D, "dof_vel_noise": D}
    ov = {"obs.obs_dict.actor_obs": list(cfg.obs.obs_dict.actor_obs) + names,
          "obs.obs_dims": [dict(d) for d in cfg.obs.obs_dims] + [{n: dims[n]} for n in names]}
    for n in names:
        ov["obs.obs_scales." + n] = (scales or NOISE_SCALES)[n]
        ov["obs.noise_scales." + n] = 0.0
    return ov


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


def _trace(tag, cfgname, overrides, general, prepare=None, after_step=None):
    """prepare(env) / after_step(env, k): the hooks of tests/test_gpu_parity.py's _env_step_vs_oracle"""
    g = dict(np.load(f"{GOLDEN}/{tag}.npz"))
    T, N, D = g["actions_in"].shape
    cfg, env = build_hip_env(cfgname, N, general=general, overrides=dict({"domain_rand.push_robots": False}, **overrides))
    assert env.reward_names == list(g["reward_names"])
    load_state_into_hip_env(env, state_dict_from_golden(g), g)
    tg = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.device)
    env.noise_process_state.copy_(tg(g["state0__ou_state"]))
    env.simulator.set_replay(tg(g["replay_root"]), tg(g["replay_dof_pos"]), tg(g["replay_dof_vel"]), tg(g["replay_contact"]))
    if prepare is not None:
        prepare(env)
    c = env._c
    for k in range(T):
        st = lambda name, dt=torch.float32: tg(g["step__state__" + name][k]).to(dt)
        dr = lambda name: tg(g["step__" + name][k])
        env.set_injected_draws(u_rfi=dr("u_rfi"), start_time=st("motion_start_times"), kp=dr("dr_kp"), kd=dr("dr_kd"), rfi_lim=dr("dr_rfi_lim"),
                               rao=dr("dr_rao"), delay=st("action_delay_idx", torch.long), ou_step=dr("ou_step"), ou_reset=dr("ou_reset"),
                               ps_kp=dr("ps_kp") if c.ps_pd else None, ps_kd=dr("ps_kd") if c.ps_pd else None,
                               ps_rao=dr("ps_rao") if c.ps_tau else None, ps_tau=dr("ps_tau") if c.ps_tau else None)
        obs, rew, reset, extras = env.step({"actions": tg(g["actions_in"][k])})
        torch.cuda.synchronize()
        if after_step is not None:
            after_step(env, k)
        w = f"{tag} step {k}: "
        assert torch.equal(reset.cpu(), torch.from_numpy(g["step__reset_buf_out"][k])), w + "reset_buf"
        close(rew, g["step__rew_buf"][k], 3e-5, w + "rew_buf", rtol=2e-4)
        for ok in obs:
            if general:         # (slerp-conditioned elements of the v2 rows: the bound tests/test_gpu_parity_v2.py derives per element)
                close(obs[ok], g["step__obs__" + ok][k], 3e-5, w + ok, hard=2e-3, frac=0.02)
            else:
                close(obs[ok], g["step__obs__" + ok][k], 3e-5, w + ok)
        close(env.torques, g["step__state__torques"][k], 1e-3, w + "torques", rtol=1e-5)
        for name, mine in (("kp_scale", env._kp_scale), ("kd_scale", env._kd_scale), ("rao_scale", env._rao_scale), ("rfi_lim_scale", env._rfi_lim_scale)):
            close(mine, g["step__state__" + name][k], 1e-6, w + name, rtol=1e-6)
        close(env.noise_process_state, g["step__state__ou_state"][k], 1e-5, w + "ou_state", rtol=1e-5)
        close(env.simulator.dof_pos, g["step__state__dof_pos"][k], 3e-5, w + "dof_pos")
        for name in ["actions", "last_actions", "motion_start_times"]:
            close(getattr(env, name), g["step__state__" + name][k], 3e-5, w + "state " + name)
    return cfg, g


def test_v1_trace_ou_noise_and_parallel_serial():
    """walk: OU process, parallel_serial_pd over randomize_pd_gain, parallel_serial_tau over use_rao; resets inside the window"""
    ov = dict(_names(WALK, ROOT2), **{"obs.noise_process": OU, "domain_rand.parallel_serial_pd": PS_PD, "domain_rand.parallel_serial_tau": PS_TAU})
    cfg, g = _trace("env_v1_walk_imunoise", WALK, ov, general=False)
    assert g["step__reset_buf_out"].sum() > 0 and np.abs(g["step__ou_reset"]).sum() > 0
    # the noisy rows differ visibly from the clean ones (scale.rpy / scale.base_ang_vel of the fixture)
    sl = _slices(cfg, "actor_obs")
    a = g["step__obs__actor_obs"]
    for clean, noisy in (("base_ang_vel", "base_ang_vel_noise"), ("projected_gravity", "projected_gravity_noise")):
        (c0, c1), (n0, n1) = sl[clean], sl[noisy]
        assert np.abs(a[..., c0:c1] - a[..., n0:n1]).max() > 1e-2, noisy


def test_v2_trace_ou_noise():
    """student23: OU process, the four *_noise names"""
    _trace("env_v2_student23_imunoise", STUDENT, dict(_names(STUDENT, ALL4), **{"obs.noise_process": OU}), general=True)


def _full(cfgname, overrides, general=False, seed=3, N=4096, noise_off=True):
    torch.manual_seed(seed)
    np.random.seed(seed)
    cfg, env = build_hip_env(cfgname, N, general=general, overrides=overrides, noise_off=noise_off)
    torch.manual_seed(seed + 1)                 # reset_all's draws: the same with the switches on or off (theirs come last)
    env.reset_all()
    return cfg, env


def _replay(env, seed=5, T=4):
    import bench

    return [t.contiguous() for t in bench.make_replay_on_device(env, T, seed=seed)]


def _outputs(env, obs, rew, reset):
    out = {"obs__" + k: v.clone() for k, v in obs.items()}
    out.update(rew=rew.clone(), reset=reset.clone(), root=env.simulator.robot_root_states.clone(), dof_pos=env.simulator.dof_pos.clone(),
               kp=env._kp_scale.clone(), kd=env._kd_scale.clone(), rao=env._rao_scale.clone(), rfi=env._rfi_lim_scale.clone(),
               torques=env.torques.clone(), start=env.motion_start_times.clone(), hist=env._hist.clone(), ep=env.episode_length_buf.clone(),
               sums=env._episode_sums.clone())
    return out


def _run(cfgname, ov, general, steps=3, noise_off=True):
    """a few steps with resets: a quarter of the envs time out in the first step"""
    cfg, env = _full(cfgname, ov, general=general, noise_off=noise_off)
    env.simulator.set_replay(*_replay(env))
    env._episode_length_buf[::4] = int(env.max_episode_length) + 1
    outs = []
    for _ in range(steps):
        outs.append(_outputs(env, *env.step({"actions": 0.3 * torch.ones(env.num_envs, env.num_dof, device=env.device)})[:3]))
    torch.cuda.synchronize()
    assert bool(outs[0]["reset"].bool().any())
    return cfg, env, outs


def _assert_equal(a, b):
    for x, y in zip(a, b):
        for k in x:
            assert torch.equal(x[k], y[k]), k


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("what", ["pd_ratio_one", "tau_zero", "ou_zero"])
def test_switch_at_its_neutral_value_is_bit_identical_to_switch_off(what, general):
    cfgname = STUDENT if general else WALK
    on = {"pd_ratio_one": {"domain_rand.parallel_serial_pd": dict(PS_PD, ratio=[1.0, 1.0])},
          "tau_zero": {"domain_rand.parallel_serial_tau": dict(PS_TAU, rao_lim=0.0, rfi_lim=0.0)},
          "ou_zero": {"obs.noise_process": dict(OU, kwargs={"mu": 0.0, "sigma": 0.0, "theta": 0.8})}}[what]
    _, _, a = _run(cfgname, {}, general)
    _, env, b = _run(cfgname, on, general)
    _assert_equal(a, b)
    if what == "ou_zero":
        assert not bool(env.noise_process_state.any())


@pytest.mark.parametrize("general", [False, True])
def test_noise_names_without_the_process_equal_the_clean_rows(general):
    cfgname = STUDENT if general else WALK
    from pbhc_amd.utils.config import load_config

    sc = load_config(f"{GOLDEN}/configs/{cfgname}", {"num_envs": 4}, now="t").obs.obs_scales
    clean = {"base_ang_vel_noise": "base_ang_vel", "projected_gravity_noise": "projected_gravity", "dof_pos_noise": "dof_pos", "dof_vel_noise": "dof_vel"}
    scales = {n: float(sc[cl]) if cl in sc else 1.0 for n, cl in clean.items()}        # each noisy name scaled as its clean one
    cfg, env, outs = _run(cfgname, _names(cfgname, ALL4, scales), general)
    sl = _slices(cfg, "actor_obs")
    base = {"base_ang_vel_noise": "base_ang_vel", "projected_gravity_noise": "projected_gravity", "dof_pos_noise": "dof_pos", "dof_vel_noise": "dof_vel"}
    from pbhc_amd.envs.env_config import flatten_obs_dims

    dims = flatten_obs_dims(cfg.obs)
    D = env.num_dof
    for o in outs:
        a = o["obs__actor_obs"]
        for n, cl in base.items():
            (n0, n1) = sl[n]
            if cl in sl:                                   # the clean key is in the row too: the same columns, scaled the same
                c0, c1 = sl[cl]
                s = float(cfg.obs.obs_scales[cl])
                assert s == scales[n], n
                assert torch.equal(a[:, n0:n1], a[:, c0:c1]), n
            else:
                assert dims[n] in (3, D)
    # ... and with the process at sigma = mu = 0 the noisy rows are the clean ones up to the euler round trip: quat_from_euler_xyz_better
    # returns a UNIT quaternion, while the replayed root rotation is unit only to ~1e-4 (quat_rotate_inverse scales by |q|^2), as in the
    # reference
    cfg2, env2, outs2 = _run(cfgname, dict(_names(cfgname, ALL4, scales), **{"obs.noise_process": dict(OU, kwargs={"mu": 0.0, "sigma": 0.0, "theta": 0.8})}), general)
    for o, o2 in zip(outs, outs2):
        assert torch.allclose(o["obs__actor_obs"], o2["obs__actor_obs"], atol=2e-3, rtol=0)
        for n in ("dof_pos_noise", "dof_vel_noise"):          # the joint rows are the clean values either way
            (n0, n1) = sl[n]
            assert torch.equal(o["obs__actor_obs"][:, n0:n1], o2["obs__actor_obs"][:, n0:n1]), n


OU_D = {"mu": 0.1, "sigma": 0.6, "theta": 0.8}


def _stats_ok(x, mean, sd, k=5.0):
    n = x.numel()
    assert abs(float(x.mean()) - mean) < k * sd / n ** 0.5, (float(x.mean()), mean)
    assert abs(float(x.std()) - sd) < k * sd / (2 * n) ** 0.5, (float(x.std()), sd)


@pytest.mark.parametrize("general", [False, True])
def test_in_kernel_ou_distributions_4096(general):
    ov = {"obs.noise_process": dict(OU, kwargs=OU_D)}
    cfg, env = _full(STUDENT if general else WALK, ov, general=general)
    c = env._c
    mu, sd, dt = OU_D["mu"], OU_D["sigma"] / (2 * OU_D["theta"]) ** 0.5, float(env.dt)
    _stats_ok(env.noise_process_state.double().cpu(), mu, sd)                 # the host-side stationary draw of reset_all
    env.simulator.set_replay(*_replay(env))
    # one step without forced resets: lag-1 autocorrelation 1 - theta dt, increment (residual) variance sigma^2 dt
    x0 = env.noise_process_state.double().cpu().clone()
    _, _, reset, _ = env.step({"actions": torch.zeros(env.num_envs, env.num_dof, device=env.device)})
    torch.cuda.synchronize()
    keep = ~reset.bool().cpu()
    x1 = env.noise_process_state.double().cpu()
    a, b = (x0[keep] - mu).flatten(), (x1[keep] - mu).flatten()
    n = a.numel()
    rho = float((a * b).sum() / (a.norm() * b.norm()))
    assert abs(rho - (1 - OU_D["theta"] * dt)) < 5 * (1 - rho ** 2) / n ** 0.5 + 1e-3, rho
    r = (x1[keep] - x0[keep] - OU_D["theta"] * (mu - x0[keep]) * dt).flatten()
    var = float(r.var())
    assert abs(var - OU_D["sigma"] ** 2 * dt) < 5 * (2 / n) ** 0.5 * OU_D["sigma"] ** 2 * dt, var
    assert abs(float(r.mean())) < 5 * (OU_D["sigma"] ** 2 * dt / n) ** 0.5
    # every env resets: the in-kernel stationary redraw
    env._episode_length_buf.fill_(int(env.max_episode_length) + 1)
    env.step({"actions": torch.zeros(env.num_envs, env.num_dof, device=env.device)})
    torch.cuda.synchronize()
    assert bool(env.reset_buf.bool().all())
    x = env.noise_process_state.double().cpu()
    _stats_ok(x, mu, sd)
    for j in range(6):
        _stats_ok(x[:, j], mu, sd, k=6.0)
    assert c.noise_process == 1


def test_ou_draws_leave_the_observation_noise_unchanged_4096():
    """with observation noise on: the rows no noisy name reads are the same with the process on or off (Philox streams of their own)"""
    _, _, a = _run(WALK, {}, False, noise_off=False)
    _, _, b = _run(WALK, {"obs.noise_process": dict(OU, kwargs=OU_D)}, False, noise_off=False)
    _assert_equal(a, b)


def test_in_kernel_pd_ratios_4096():
    ov = {"domain_rand.parallel_serial_pd": PS_PD, "domain_rand.randomize_pd_gain": False}
    cfg, env = _full(WALK, ov)
    idx = PS_PD["joint_idx"]
    other = [d for d in range(env.num_dof) if d not in idx]
    kp0, kd0 = env._kp_scale.double().cpu().clone(), env._kd_scale.double().cpu().clone()
    # the host-side form (reset_all): the scales start at 1, so they ARE the first factors — for the envs that reset_all's own step did
    # not reset again (those compounded a second factor in the kernel)
    lo, hi = PS_PD["ratio"]
    once = ~env.reset_buf.bool().cpu()
    assert int(once.sum()) > env.num_envs // 2
    assert float(kp0[once][:, idx].min()) >= lo and float(kp0[once][:, idx].max()) <= hi and bool((kp0[:, other] == 1).all())
    env.simulator.set_replay(*_replay(env))
    env._episode_length_buf.fill_(int(env.max_episode_length) + 1)
    env.step({"actions": torch.zeros(env.num_envs, env.num_dof, device=env.device)})
    torch.cuda.synchronize()
    assert bool(env.reset_buf.bool().all())
    kp1, kd1 = env._kp_scale.double().cpu(), env._kd_scale.double().cpu()
    assert torch.equal(kp1[:, other], kp0[:, other]) and torch.equal(kd1[:, other], kd0[:, other])
    for r in (kp1[:, idx] / kp0[:, idx], kd1[:, idx] / kd0[:, idx]):          # compounded: new = old x U(ratio)
        r = r.flatten()
        assert float(r.min()) >= lo - 1e-6 and float(r.max()) <= hi + 1e-6
        n = r.numel()
        sd = (hi - lo) / 12 ** 0.5
        assert abs(float(r.mean()) - (lo + hi) / 2) < 5 * sd / n ** 0.5
        assert abs(float(r.std()) - sd) < 0.02 * sd + 5 * sd / (2 * n) ** 0.5
        hist = torch.histc(r.float(), bins=8, min=lo, max=hi)
        assert float((hist - n / 8).abs().max()) < 6 * (n / 8) ** 0.5
    assert not torch.equal(kp1[:, idx], kd1[:, idx])                         # two draws


def test_in_kernel_tau_torque_residual_4096():
    ov = {"domain_rand.parallel_serial_tau": PS_TAU}
    runs = []
    for inject_zero in (True, False):
        cfg, env = _full(WALK, ov)
        env.simulator.set_replay(*_replay(env))
        if inject_zero:
            env.set_injected_draws(ps_tau=torch.zeros(env.num_envs, len(PS_TAU["joint_idx"]), device=env.device))
        env.step({"actions": 0.1 * torch.ones(env.num_envs, env.num_dof, device=env.device)})
        torch.cuda.synchronize()
        runs.append(env.torques.double().cpu().clone())
    idx = PS_TAU["joint_idx"]
    other = [d for d in range(env.num_dof) if d not in idx]
    assert torch.equal(runs[0][:, other], runs[1][:, other])
    tl = torch.tensor([env._c.torque_limits[d] for d in idx], dtype=torch.float64)
    unclipped = (runs[0][:, idx].abs() < tl) & (runs[1][:, idx].abs() < tl)
    z = ((runs[1][:, idx] - runs[0][:, idx]) / (PS_TAU["rfi_lim"] * tl))[unclipped]
    n = z.numel()
    assert n > 0.9 * env.num_envs * len(idx)
    assert abs(float(z.mean())) < 5 / n ** 0.5 and abs(float(z.std()) - 1.0) < 0.05


@pytest.mark.parametrize("agent", ["v1", "v2"])
def test_graph_rollout_with_all_three_switches_equals_the_eager_loop(agent, monkeypatch):
    """the rollout hipGraph (step, reduction on the branch stream) against the step-by-step loop, OU + both parallel-serial switches on"""
    import tests.test_gpu_parity as P
    import tests.test_gpu_parity_v2 as P2

    ov = {"obs.noise_process": dict(OU, kwargs=OU_D), "domain_rand.parallel_serial_pd": PS_PD, "domain_rand.parallel_serial_tau": PS_TAU}
    orig = P.build_hip_env

    def build(*a, **k):
        cfgname = a[0] if a else k["cfgname"]
        extra = dict(ov, **_names(cfgname, ROOT2)) if cfgname.startswith("v1") else ov      # (v1's actor reads the noisy rows too)
        return orig(*a, **dict(k, overrides=dict(k.get("overrides") or {}, **extra)))

    monkeypatch.setattr(P, "build_hip_env", build)
    monkeypatch.setattr(P2, "build_hip_env", build)
    a = P._rollouts_with_split(True, agent, batched=True, fused_sample=True, rollout_graph=True, rollouts=4)
    b = P._rollouts_with_split(True, agent, batched=True, fused_sample=True, rollout_graph=False, rollouts=4)
    a.pop("_time_outs_seen"); b.pop("_time_outs_seen")
    assert bool(a.pop("_used_graph")) and not bool(b.pop("_used_graph"))
    a.pop("_used_graph_each"); b.pop("_used_graph_each")
    for k in a:
        assert torch.equal(a[k], b[k]), k
