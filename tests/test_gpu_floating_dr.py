"""FloatingBaseSim's per-env randomisation on the GPU (pbhc_amd/simulator/floating_sim.py `domain_rand`, csrc/pbhc_floating_sim.hip): the
per-env inertial rows and friction against ONE float64 model per env (tests/floating_model.py holds one robot's masses; the per-env models
and inputs are tests/floating_dr_inputs.py's), identity tables against no tables bit for bit, through the env one step at a time with the
critic's privileged columns, push_robots with injected and with the kernel's own draws, graph = eager, resume, memory edges.

Tolerances are tests/test_gpu_floating_sim.py's: gamma = 16 x 2^-24 on the per-element terms of floating_model.forward and the carried bound
of floating_model.carried_bound; the float32 restatement of the per-env models sits inside a quarter of it (tests/test_floating_dr_cpu.py).
"""
import os

import numpy as np
import pytest
import torch

from pbhc_amd import _lib
from pbhc_amd.simulator import floating_sim as fsim
from tests import floating_dr_inputs as di
from tests import floating_model as fm
from tests import joint_sim_model as jm
from tests import test_gpu_floating_sim as F
from tests.arena import POISON, arena
from tests.test_gpu_articulated_sim import _np, _prepare, _torque_params, scenario
from tests.test_gpu_imu_noise_dr import _slices

pytestmark = pytest.mark.gpu

DEV, H, GAMMA, EPS = F.DEV, F.H, F.GAMMA, F.EPS
TABLES = dict(link_mass=True, base_com=True, friction=True)
ALL = dict(TABLES, push=True)
SLIP = 0.6                                                   # the default 0.4 m/s does not pass the screen at friction_range[1] = 1.2
PUSH = {"domain_rand.push_robots": True, "domain_rand.push_interval_s": [1, 3], "domain_rand.max_push_vel_xy": 0.5}


def _with_tables(mjcf, N, identity=False):
    """F._setup's nominal params plus the per-env tables on the device -> sk, m, p, table [N,32,4], friction [N], what to keep alive"""
    sk, m, p, points = F._setup(mjcf)
    if identity:
        names = list(sk.body_names)[:sk.num_bodies][::2]
        table = fsim.FloatingBaseSim.inertial_table(sk, names, np.ones((N, len(names)), np.float32), np.zeros((N, 3), np.float32))
        friction = np.full(N, p.friction, np.float32)
    else:
        table, friction = di.tables(sk, N)
    dev = [torch.from_numpy(table).to(DEV).contiguous(), torch.from_numpy(friction).to(DEV).contiguous()]
    assert dev[0].data_ptr() % 16 == 0
    return sk, m, p, table, friction, [points] + dev


def _tensors(sk, p, root, q, v, tau, steps):
    """F._debug, and the five output TENSORS as the kernel left them"""
    outs = {}

    def place(name, t):
        if name.startswith("out_"):
            outs[name] = t
        return t

    got = F._debug(sk, p, root, q, v, tau, steps, place=place)
    return got, outs


@pytest.mark.parametrize("mjcf", [F.TREE, F.G1])
def test_one_substep_with_per_env_tables_equals_each_envs_own_model(mjcf):
    """N = 33 (four full workgroups of 8 envs and a ragged one), mass scales in [0.5, 2] on every second body, a centre-of-mass bias of up
    to +-5 cm on one body, friction in [0.2, 1.2], all per env; fm.random_states seed 5, no element skipped: every [a_0, alpha_0, q''] and
    every point's force within gamma x terms of THAT env's model — and the nominal model does not fit: more than half of the envs have an
    element outside its bound"""
    N = 33
    sk, m, p, table, friction, keep = _with_tables(mjcf, N)
    models = di.env_models(m, table, friction)
    root, q, v, tau = fm.random_states(m, N, 5, clear=1e-3)
    want, f, d = di.forward_each(models, root, q, v, tau, H)
    assert np.abs(m["ground_height"] - d["z"]).min() >= 1e-3 and (f[..., 2] > 0).any()
    tol, tol_f = GAMMA * d["terms"], GAMMA * d["f_abs"]
    p.env_inertial, p.env_friction = keep[1].data_ptr(), keep[2].data_ptr()
    got = F._debug(sk, p, root, q, v, tau, 1)
    gf = F._by_point(m, got["force"])
    err, ef = np.abs(got["acc0"] - want), np.abs(gf - f)
    on = f[..., 2] > 0
    print(f"{mjcf}: per-env tables: worst residual / bound accelerations {float((err / tol).max()):.3f}, forces {float((ef[on] / tol_f[on]).max()):.3f}")
    nom, fnom, dn = fm.forward(m, fm.state(root, q, v), tau, H)
    misfit = (np.abs(got["acc0"] - nom) > GAMMA * dn["terms"]).any(axis=1) | (np.abs(gf - fnom) > GAMMA * dn["f_abs"]).any(axis=(1, 2))
    print(f"the nominal model misses {int(misfit.sum())} of {N} envs")
    assert (ef <= tol_f).all(), (float((ef[on] / tol_f[on]).max()), np.argwhere(ef > tol_f)[:5].tolist())
    assert (err <= tol).all(), (float((err / tol).max()), np.argwhere(err > tol)[:5].tolist())
    assert misfit.sum() > N // 2, "the tables change too little for the test to show anything"


@pytest.mark.parametrize("mjcf", [F.TREE, F.G1])
def test_identity_tables_equal_no_tables_bit_for_bit(mjcf):
    """env_inertial from scale 1 / bias 0 and env_friction filled with the params' friction: all five outputs of 4 sub-steps are the
    NULL-pointer run's, bit for bit"""
    N = 33
    sk, m, p, table, friction, keep = _with_tables(mjcf, N, identity=True)
    root, q, v, tau = fm.random_states(m, N, 5, clear=1e-3)
    _, plain = _tensors(sk, p, root, q, v, tau, 4)
    p.env_inertial, p.env_friction = keep[1].data_ptr(), keep[2].data_ptr()
    _, ident = _tensors(sk, p, root, q, v, tau, 4)
    assert sorted(plain) == ["out_acc0", "out_force", "out_q", "out_root", "out_v"]
    for k in plain:
        assert bool(torch.isfinite(plain[k]).all()) and torch.equal(plain[k], ident[k]), k
    assert float(plain["out_force"].abs().max()) > 10.0


# ---- through the env ---------------------------------------------------------------------------------------------------------------------
def _build(N, flags, extra=None, seed=3, noise_off=True, spec=None):
    return F._build(F.WALK, N, False, extra=extra, seed=seed, noise_off=noise_off, spec=dict({"slip_velocity": SLIP, "domain_rand": dict(flags)}, **(spec or {})))


def _env_models(env):
    """one model per env from the tables the simulator uploaded (its float32 values); without a table the nominal value"""
    s, N = env.simulator, env.num_envs
    m = F._env_model(env)
    table = s._inertial_dev.cpu().numpy() if s._inertial_dev is not None else fsim.FloatingBaseSim.inertial_table(env.skeleton, [], None, np.zeros((N, 3)))
    friction = s._friction_dev.cpu().numpy() if s._friction_dev is not None else np.full(N, m["friction"], np.float32)
    return di.env_models(m, table, friction)


def _row(P, a_del, n, N):
    """env n's rows of the torque law's parameters (a batch of one)"""
    return {k: (x[n:n + 1] if isinstance(x, np.ndarray) and x.ndim == 2 and x.shape[0] == N else x) for k, x in P.items()}, a_del[n:n + 1]


def _model_step_each(models, root, q, v, a_del, P):
    """F._model_step of env n's model on env n's row, stacked -> dict(s, E, margin, touch)"""
    from concurrent.futures import ThreadPoolExecutor

    N = q.shape[0]

    def one(n):
        Pn, an = _row(P, a_del, n, N)
        return F._model_step(models[n], root[n:n + 1], q[n:n + 1], v[n:n + 1], an, Pn)

    with ThreadPoolExecutor(4) as pool:                      # (numpy releases the interpreter lock in its loops: about twice as fast)
        parts = list(pool.map(one, range(N)))
    out = {k: np.concatenate([r[k] for r in parts], 0) for k in ("E", "margin", "touch")}
    out["s"] = {k: np.concatenate([r["s"][k] for r in parts], 0) for k in parts[0]["s"]}
    return out


def _step(env, sc, k, zero_actions=False):
    """one env step of the scenario with its injected RFI draws -> what the comparison needs (F._run_case's record)"""
    s = env.simulator
    actions = np.zeros_like(sc["actions"][k]) if zero_actions else sc["actions"][k]
    env.set_injected_draws(u_rfi=torch.from_numpy(sc["u_rfi"][k]).to(env.device))
    P = _torque_params(env, sc["u_rfi"][k])
    pre = dict(q=_np(s.dof_pos), v=_np(s.dof_vel), root=_np(s.robot_root_states), queue=_np(env.action_queue), delay=env.action_delay_idx.cpu().numpy())
    a_del = jm.delayed_action(actions, float(env._c.action_clip_value), pre["queue"], pre["delay"], bool(env._c.randomize_ctrl_delay))
    obs, _, _, _ = env.step({"actions": torch.from_numpy(actions).to(env.device)})
    torch.cuda.synchronize()
    return dict(P=P, pre=pre, a_del=a_del, obs=obs, reset=env.reset_buf.bool().cpu().numpy(), frame_q=_np(s.replay["dof_pos"][0]),
                frame_v=_np(s.replay["dof_vel"][0]), frame_root=_np(s.replay["root"][0]),
                frames=[s.replay[k_][0].clone() for k_ in ("root", "dof_pos", "dof_vel", "contact")])


def test_frame_equals_each_envs_own_model_one_step_at_a_time():
    """the v1 walk config with link_mass, base_com and friction on, N = 33, the simulators' scenario: the frame step k consumed is each
    env's OWN model stepped from the state step k - 1 left, per element within the carried bound; the skip rule and its cap (1 % of the
    (env, step) pairs) are test_frame_equals_the_model_one_step_at_a_time's.  The uploaded tables are inertial_table of the tensors the
    critic observes, and the critic's dr_link_mass / dr_base_com / dr_friction columns hold those tensors."""
    N = 33
    cfg, env = _build(N, TABLES)
    D, s = env.num_dof, env.simulator
    sc = scenario(N, D, float(env._c.action_clip_value))
    _prepare(env, sc)
    dr = cfg.env.config.domain_rand
    names = list(dr.randomize_link_body_names)
    scale, bias, fric = s._link_mass_scale.cpu(), s._base_com_bias.cpu(), s.friction_coeffs.reshape(N).cpu()
    assert float(scale.min()) >= 0.9 - 1e-6 and float(scale.max()) <= 1.1 + 1e-6 and float(scale.std()) > 0.01 and float(bias.abs().max()) > 0.01
    assert float(fric.min()) >= 0.2 - 1e-6 and float(fric.max()) <= 1.2 + 1e-6 and float(fric.std()) > 0.05
    assert np.array_equal(s._inertial_dev.cpu().numpy(), fsim.FloatingBaseSim.inertial_table(env.skeleton, names, scale, bias))
    assert torch.equal(s._friction_dev.cpu(), fric)
    p = s._params
    assert p.env_inertial == s._inertial_dev.data_ptr() and p.env_friction == s._friction_dev.data_ptr() and not p.push_counter
    models = _env_models(env)
    skipped = total = 0
    worst = 0.0
    for k in range(sc["steps"]):
        r = _step(env, sc, k)
        mm = _model_step_each(models, r["pre"]["root"], r["pre"]["q"], r["pre"]["v"], r["a_del"], r["P"])
        err = fm.state_error(fm.state(r["frame_root"], r["frame_q"], r["frame_v"]), mm["s"], D)
        ok = (mm["margin"].min(axis=1) >= 1e-5) & (mm["touch"] >= 1e-6)
        skipped += int((~ok).sum()); total += N
        ratio = float((err / mm["E"])[ok].max())
        worst = max(worst, ratio)
        print(f"step {k}: worst residual / bound {ratio:.3f}, skipped {int((~ok).sum())}, resets {int(r['reset'].sum())}")
        assert not (err > mm["E"])[ok].any(), (k, ratio, np.argwhere((err > mm["E"]) & ok[:, None])[:5].tolist())
        if k == 0:
            # ... and the nominal robot is NOT what the kernel integrated
            nm = F._model_step(F._env_model(env), r["pre"]["root"], r["pre"]["q"], r["pre"]["v"], r["a_del"], r["P"])
            en = fm.state_error(fm.state(r["frame_root"], r["frame_q"], r["frame_v"]), nm["s"], D)
            assert (en > nm["E"]).any(axis=1).sum() > N // 2
        sl = _slices(cfg, "critic_obs")
        crit = r["obs"]["critic_obs"].cpu()
        for key, src in (("dr_link_mass", scale), ("dr_base_com", bias), ("dr_friction", fric[:, None])):
            a, b = sl[key]
            assert torch.equal(crit[:, a:b], src * float(cfg.obs.obs_scales[key])), (k, key)
    print(f"per-env tables through the env: worst residual / bound {worst:.3f}; {skipped} of {total} pairs skipped")
    assert skipped <= 0.01 * total, (skipped, total)


# ---- push_robots ------------------------------------------------------------------------------------------------------------------------------
def _threshold(interval, dt):
    """(int)((float)push_interval / dt) in float32, as the kernel and the reference's (push_interval_s / self.dt).int()"""
    return (np.asarray(interval, np.float32) / np.float32(dt)).astype(np.int32)


@pytest.mark.parametrize("fixed", [True, False])
def test_push_with_injected_draws(fixed):
    """N = 9, push_interval_s [1, 3]; the counters are preset so that envs 1, 4 and 7 fire on the next step, env 7 just reset
    (episode_length_buf 0 at the front), nobody else.  Envs 1 and 4: the frame is the model stepped from the PUSHED root (+= with
    _push_fixed, = without).  Env 7: not pushed — bit-identical to a run with push off — but its counter and interval are renewed.
    Everybody else: bit-identical to the run with push off.  Counters, intervals and push_vel as the header states them, the interval's
    cap at u0 -> 1 included."""
    N, fire, reset_env = 9, [1, 4, 7], 7
    extra = dict(PUSH, **{"domain_rand._push_fixed": fixed})
    cfg, env = _build(N, dict(push=True), extra=extra)
    D, s = env.num_dof, env.simulator
    sc = scenario(N, D, float(env._c.action_clip_value))
    _prepare(env, sc)
    p = s._params
    assert p.push_counter == s.push_counter.data_ptr() and (p.push_lo, p.push_hi, p.push_fixed) == (1, 3, int(fixed)) and abs(p.max_push_vel_xy - 0.5) < 1e-7
    assert not p.env_inertial and not p.env_friction
    assert s.push_interval.dtype == torch.int32 and s.push_counter.dtype == torch.int32 and set(s.push_interval.tolist()) <= {1, 2}
    c0 = s.push_counter.clone()                              # (control steps so far: reset_all's among them)
    _step(env, sc, 0)                                        # every env has an episode under way
    assert torch.equal(s.push_counter, c0 + 1) and int(c0.max()) <= 2
    dt = float(env._c.dt)
    interval = np.array([1, 2, 1, 2, 1, 2, 1, 2, 1], np.int32)
    counter = np.full(N, 3, np.int32)
    counter[fire] = _threshold(interval[fire], dt)
    assert counter[1] in (99, 100) and counter[4] in (49, 50)
    s.push_interval.copy_(torch.from_numpy(interval)); s.push_counter.copy_(torch.from_numpy(counter))
    env._episode_length_buf[reset_env] = 0                   # as a reset leaves it (the kernel's test; root_states is whatever the step left)
    u = np.random.default_rng(5).random((N, 3)).astype(np.float32)
    u[1, 0], u[4, 0] = 1.0, 0.25                             # lo + floor(1.0 x 2) = 3: capped at hi - 1 = 2;  lo + floor(0.5) = 1
    s.set_injected_push(torch.from_numpy(u).to(DEV))
    sd = env.state_dict()
    root0 = _np(s.robot_root_states)
    r = _step(env, sc, 1)
    # the state a run with push off leaves from the same state
    _, off = _build(N, dict(push=False), extra=extra)
    off.load_state_dict(sd)
    assert off.simulator.push_counter is None and not off.simulator._params.push_counter
    ro = _step(off, sc, 1)
    quiet = [e for e in range(N) if e not in (1, 4)]
    for a, b in zip(r["frames"], ro["frames"]):
        assert torch.equal(a[quiet], b[quiet])
    assert not torch.equal(r["frames"][0][[1, 4]], ro["frames"][0][[1, 4]])
    # the pushed envs against the model from the pushed root
    pv = (np.float32(2.0) * u[:, 1:3] - np.float32(1.0)) * np.float32(0.5)        # the kernel's float32 operations
    pushed = root0.copy()
    for e in (1, 4):
        pushed[e, 7:9] = (root0[e, 7:9].astype(np.float32) + pv[e] if fixed else pv[e]).astype(np.float64)
    assert np.array_equal(r["pre"]["root"], root0)
    m = F._env_model(env)
    mm = F._model_step(m, pushed, r["pre"]["q"], r["pre"]["v"], r["a_del"], r["P"])
    err = fm.state_error(fm.state(r["frame_root"], r["frame_q"], r["frame_v"]), mm["s"], D)
    ok = (mm["margin"].min(axis=1) >= 1e-5) & (mm["touch"] >= 1e-6)
    assert ok[[1, 4]].all(), "a pushed env sits on a discontinuity of the model: choose other envs"
    print(f"push ({'+=' if fixed else '='}): worst residual / bound of the pushed envs {float((err / mm['E'])[[1, 4]].max()):.3f}, of all {float((err / mm['E'])[ok].max()):.3f}")
    assert not (err > mm["E"])[ok].any(), float((err / mm["E"])[ok].max())
    unpushed = F._model_step(m, root0, r["pre"]["q"], r["pre"]["v"], r["a_del"], r["P"])
    eu = fm.state_error(fm.state(r["frame_root"], r["frame_q"], r["frame_v"]), unpushed["s"], D)
    assert (eu > unpushed["E"])[[1, 4]].any(axis=1).all(), "the push is too small to be seen"
    # counters, intervals, push_vel
    want_c = counter + 1
    want_c[fire] = 1
    want_i = interval.copy()
    want_i[1], want_i[4], want_i[7] = 2, 1, min(1 + int(np.floor(np.float32(u[7, 0]) * np.float32(2.0))), 2)
    assert s.push_counter.tolist() == want_c.tolist() and s.push_interval.tolist() == want_i.tolist()
    want_v = np.zeros((N, 2), np.float32)
    want_v[fire] = (np.float32(2.0) * u[fire, 1:3] - np.float32(1.0)) * np.float32(0.5)
    assert np.array_equal(s.push_vel.cpu().numpy(), want_v)
    with pytest.raises(_lib.PbhcError, match=r"floating_sim\.domain_rand\.push is off"):
        off.simulator.set_injected_push(torch.zeros(N, 3, device=DEV))


def _forced_push(seed):
    N = 1024
    extra = dict(PUSH, **{"domain_rand.push_interval_s": [1, 5]})
    cfg, env = _build(N, dict(push=True), extra=extra, seed=seed)
    s = env.simulator
    env.reset_all()
    zero = torch.zeros(N, env.num_dof, device=env.device)
    env.step({"actions": zero})
    s.push_counter.copy_(torch.from_numpy(_threshold(s.push_interval.cpu().numpy(), float(env._c.dt))).to(DEV))
    before = s.robot_root_states.clone()
    env.step({"actions": zero})
    torch.cuda.synchronize()
    return env, before, s.push_vel.clone(), s.push_interval.clone(), s.push_counter.clone()


def test_push_with_the_kernels_own_draws():
    """N = 1024, every env's counter at its threshold: one step and every env has fired — every component of push_vel in [-max, max] and not
    all alike, every interval of {lo .. hi - 1} drawn, mean and spread those of the uniform law (six sigma of 1024 draws), and the same
    seed gives the same draws twice"""
    env, before, pv, itv, cnt = _forced_push(3)
    N = env.num_envs
    assert cnt.tolist() == [1] * N
    assert float(pv.abs().max()) <= 0.5 and set(itv.tolist()) == {1, 2, 3, 4}
    assert not torch.equal(pv[0], pv[1]) and len(set(pv[:, 0].tolist())) > N // 2
    x = pv.double().cpu().numpy().ravel() / 0.5                  # U(-1, 1): mean 0 +- 1/sqrt(3 n), variance 1/3
    assert abs(x.mean()) < 6.0 / np.sqrt(3 * x.size) and abs(x.var() - 1.0 / 3.0) < 0.05
    assert np.bincount(itv.cpu().numpy(), minlength=5)[1:].min() > N // 8
    _, _, pv2, itv2, _ = _forced_push(3)
    assert torch.equal(pv, pv2) and torch.equal(itv, itv2)


def _rollouts(rollout_graph, rollouts=3):
    """F._rollouts with all four flags on and the push counters preset so that the envs fire during the second and third rollout"""
    from pbhc_amd.agents.mh_ppo import MHPPO

    flags = {"PBHC_ROLLOUT_GRAPH": "1" if rollout_graph else "0", "PBHC_ROLLOUT_SPLIT": "1", "PBHC_CRITIC_BATCHED": "1", "PBHC_FUSED_SAMPLE": "1"}
    os.environ.update(flags)
    try:
        cfg, env = _build(64, ALL, extra=dict(PUSH, **{"algo.config.num_steps_per_env": 8}), seed=11, noise_off=False)
        algo = MHPPO(env=env, config=cfg.algo.config, log_dir=None, device=DEV)
        algo.setup()
        algo._train_mode()
        obs = env.reset_all()
        s = env.simulator
        thr = _threshold(s.push_interval.cpu().numpy(), float(env._c.dt))
        s.push_counter.copy_(torch.from_numpy(thr - 10 - np.arange(64, dtype=np.int32) % 8).to(DEV))     # fires at step 10 .. 17 of 24
        used = []
        gperm = torch.Generator().manual_seed(23)
        for r in range(rollouts):
            algo.storage.clear()
            obs = algo._rollout_step(obs)
            used.append(bool(getattr(algo, "_rollout_used_graph", False)))
            n = algo.storage.num_envs * algo.storage.num_transitions_per_env
            algo._training_step(indices=torch.randperm(n, generator=gperm).to(DEV))
        torch.cuda.synchronize()
        out = {k: getattr(algo, k).clone() for k in ("_pflat", "_mflat", "_vflat")}
        out.update(dof_state=s.dof_state.clone(), root=s.robot_root_states.clone(), globals=env.globals.clone(), frame_root=s.replay["root"].clone(),
                   push_counter=s.push_counter.clone(), push_interval=s.push_interval.clone(), push_vel=s.push_vel.clone(),
                   actions=algo.storage.actions.clone(), rewards=algo.storage.rewards.clone())
        return out, used
    finally:
        for k in flags:
            os.environ.pop(k, None)


def test_captured_rollout_equals_the_eager_loop_with_all_four_flags():
    """all four flags on, 64 envs, 3 rollouts of 8 steps, every env's push firing inside the second or third rollout (the captured graph's
    replays): weights, Adam moments, root, dof_state and the push state bit-identical to the step-by-step loop"""
    a, used_a = _rollouts(True)
    b, used_b = _rollouts(False)
    assert used_a == [False, True, True] and not any(used_b)
    assert bool(torch.isfinite(a["dof_state"]).all()) and bool(torch.isfinite(a["root"]).all())
    assert bool((a["push_vel"].abs().sum(1) > 0).all()) and int(a["push_counter"].max()) <= 14, "a push did not fire inside the rollouts"
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_resume_is_bit_identical_with_all_four_flags():
    """six env steps in one run; in a second run three steps, state_dict(), a fresh env, load_state_dict(), three more — with a push firing
    on either side of the save.  A state dict saved with push off still loads into a simulator with push off."""
    N = 33
    sc = scenario(N, 23, 100.0)

    def fresh(flags=ALL):
        _, env = _build(N, flags, extra=PUSH, seed=5, noise_off=False)
        return env

    def start(env):
        _prepare(env, sc)
        s = env.simulator
        thr = _threshold(s.push_interval.cpu().numpy(), float(env._c.dt))
        s.push_counter.copy_(torch.from_numpy(thr - 1 - np.arange(N, dtype=np.int32) % 5).to(DEV))       # fires at step 1 .. 5

    def steps(env, ks):
        for k in ks:
            obs, _, _, _ = env.step({"actions": torch.from_numpy(sc["actions"][k]).to(env.device)})
        torch.cuda.synchronize()
        return obs

    env_a = fresh(); start(env_a)
    obs_a = steps(env_a, range(6))
    env_b = fresh(); start(env_b)
    steps(env_b, range(3))
    sd = env_b.state_dict()
    assert {"push_counter", "push_interval", "push_vel"} <= set(sd["simulator"])
    env_c = fresh()
    env_c.load_state_dict(sd)
    obs_c = steps(env_c, range(3, 6))
    for k in obs_a:
        assert torch.equal(obs_a[k], obs_c[k]), k
    sa, sc_ = env_a.simulator, env_c.simulator
    for name in ("dof_state", "robot_root_states", "push_counter", "push_interval", "push_vel", "_inertial_dev", "_friction_dev"):
        assert torch.equal(getattr(sa, name), getattr(sc_, name)), name
    assert torch.equal(sa.replay["root"], sc_.replay["root"]) and torch.equal(env_a.reset_buf, env_c.reset_buf)
    assert bool((sa.push_vel.abs().sum(1) > 0).all()) and int(sa.push_counter.max()) <= 5, "a push did not fire"
    assert not torch.equal(env_b.simulator.push_vel, sa.push_vel), "no push fired after the save"
    # push off: the state dict has no push state, and loads
    env_d = fresh(TABLES); _prepare(env_d, sc)
    steps(env_d, range(2))
    sd_d = env_d.state_dict()
    assert "push_counter" not in sd_d["simulator"]
    env_e = fresh(TABLES)
    env_e.load_state_dict(sd_d)
    assert torch.equal(steps(env_d, range(2, 4))["critic_obs"], steps(env_e, range(2, 4))["critic_obs"])
    assert torch.equal(env_d.simulator.robot_root_states, env_e.simulator.robot_root_states)


def test_the_new_operands_in_arenas():
    """N = 9 (one full workgroup and a ragged one), all four flags: env_inertial, env_friction, push_counter, push_interval, push_vel and
    u_push each in a poisoned arena (env_inertial on its 16-byte boundary, the others one float off theirs).  The step's results are finite
    and those of the plain run from the same state, every byte outside the operands is intact — so nothing is stored for an env beyond N,
    whose loads are clamped onto env N - 1 — and push_vel is written for the envs that fire only."""
    N, fire = 9, [0, 3, 8]
    cfg, env = _build(N, ALL, extra=PUSH)
    D, s = env.num_dof, env.simulator
    sc = scenario(N, D, float(env._c.action_clip_value))
    _prepare(env, sc)
    _step(env, sc, 0)
    counter = np.full(N, 3, np.int32)
    counter[fire] = _threshold(s.push_interval.cpu().numpy(), float(env._c.dt))[fire]
    s.push_counter.copy_(torch.from_numpy(counter))
    u = torch.from_numpy(np.random.default_rng(8).random((N, 3)).astype(np.float32)).to(DEV)
    s.set_injected_push(u)
    sd = env.state_dict()
    plain = _step(env, sc, 1)
    plain_state = {k: getattr(s, k).clone() for k in ("push_counter", "push_interval", "push_vel")}
    assert set(np.flatnonzero(plain_state["push_vel"].abs().sum(1).cpu().numpy())) == set(fire)
    env.load_state_dict(sd)
    p, reg = s._params, {}

    def rehome(attr, field, fill, offset):
        t = getattr(s, attr)
        rows, cols = t.shape[0], t.numel() // t.shape[0]
        reg[field] = arena(rows, cols, offset=offset, fill=fill, data=t.reshape(rows, cols), device=DEV, dtype=t.dtype, name=field)
        setattr(s, attr, reg[field].view.reshape(t.shape))
        setattr(p, field, reg[field].ptr())

    rehome("_inertial_dev", "env_inertial", POISON, 0)
    rehome("_friction_dev", "env_friction", POISON, 1)
    rehome("push_counter", "push_counter", 7, 1)             # (int32 fills: harmless as data — a count, a whole second — and no value the run produces)
    rehome("push_interval", "push_interval", 9, 1)
    rehome("push_vel", "push_vel", POISON, 1)
    rehome("_u_push", "u_push", POISON, 1)
    assert reg["env_inertial"].ptr() % 16 == 0 and all(reg[k].ptr() % 16 == 4 for k in reg if k != "env_inertial")
    got = _step(env, sc, 1)
    for a in reg.values():
        assert a.intact(), a.damage()
    for x, y in zip(got["frames"], plain["frames"]):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)
    for k, v in plain_state.items():
        assert torch.equal(getattr(s, k), v), k
    # push_vel of the envs that did not fire was never stored: it still holds what the state dict restored
    assert set(np.flatnonzero(s.push_vel.abs().sum(1).cpu().numpy())) == set(fire)
    # a misaligned env_inertial is refused without a launch: no byte of any arena changes
    import ctypes as C

    snap = {k: a.buf.clone() for k, a in reg.items()}
    p.env_inertial = reg["env_inertial"].ptr() + 4
    rc = _lib.lib().pbhc_floating_sim_step(env._env, C.byref(env._io), C.byref(p), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == _lib.K["PBHC_EINVAL"] and b"env_inertial" in _lib.lib().pbhc_last_error()
    for k, a in reg.items():
        assert torch.equal(a.buf.view(torch.int32), snap[k].view(torch.int32)), k
