"""JointSpaceSim on the GPU (pbhc_amd/simulator/joint_sim.py, csrc/pbhc_joint_sim.hip k_joint_sim): the integrator against the float64 model
of tests/joint_sim_model.py one control step at a time, the first sub-step's torque against the step's own `torques`, the root / contact
frame, the closed loop, graph = eager, resume, and the ordering against the dof-far pre-pass.

The scenario (`scenario`, `case_overrides`): v1 walk at N = 70 and v2 student at N = 33 — both leave a partial workgroup (8 envs each) and an
odd env in a wave —, control delay, PD-gain DR, RAO and RFI on, observation noise off, six control steps of seeded N(0,1) actions with about
5 % of them at 3x the clip value, three joints started 0.05 rad beyond a hard limit, two joints whose torque limit is lowered to 1 N m (the
clip binds under ordinary actions), start times that make envs run off their clip's end inside the six steps."""
import os
import random

import numpy as np
import pytest
import torch

from tests import joint_sim_model as model
from tests.helpers import GOLDEN, build_hip_env
from pbhc_amd.utils.config import load_config

pytestmark = pytest.mark.gpu

SIM = "pbhc_amd.simulator.joint_sim.JointSpaceSim"
WALK, STUDENT = "v1_g1_23dof_walk.yaml", "v2_g1_23dof_student.yaml"
CASES = [(WALK, 70, False), (STUDENT, 33, True)]
LOWERED = (2, 10)                                          # dofs whose torque limit is lowered
EPS = 2.0 ** -24
DEV = "cuda:0"


def scenario(N, D, clip, seed=7, steps=6):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((steps, N, D))
    big = rng.random((steps, N, D)) < 0.05
    a = np.where(big, np.sign(a) * 3.0 * clip, a).astype(np.float32)
    return dict(steps=steps, actions=a, big_share=float(big.mean()), u_rfi=rng.random((steps, N, D)).astype(np.float32),
                beyond_limit=[(1, 3, 1), (N - 1, 0, 0), (N // 2, D - 1, 1)],          # (env, dof, 0 below the lower / 1 above the upper limit)
                ending=[0, 9, N - 2],                                                 # envs placed three steps before their clip's end
                inertia=lambda D_: np.linspace(0.04, 0.3, D_), damping=0.05)


def case_overrides(cfgname, dr=True, extra=None):
    base = load_config(os.path.join(GOLDEN, "configs", cfgname), {}, now="test")
    D = len(base.robot.dof_names)
    lim = [float(x) for x in base.robot.dof_effort_limit_list]
    if dr:
        for d in LOWERED:
            lim[d] = 1.0
    sc = scenario(4, D, 1.0)
    ov = {"simulator._target_": SIM, "domain_rand.push_robots": False, "robot.dof_effort_limit_list": lim,
          "simulator.config.joint_sim": {"inertia": [float(x) for x in sc["inertia"](D)], "damping": sc["damping"]},
          "domain_rand.randomize_ctrl_delay": dr, "domain_rand.ctrl_delay_step_range": [0, 2], "domain_rand.randomize_pd_gain": dr,
          "domain_rand.use_rao": dr, "domain_rand.randomize_torque_rfi": dr, "domain_rand.randomize_rfi_lim": dr}
    ov.update(extra or {})
    return ov


def _seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def _build(cfgname, N, general, dr=True, extra=None, seed=3, noise_off=True):
    _seed_all(seed)
    cfg, env = build_hip_env(cfgname, N, general=general, overrides=case_overrides(cfgname, dr, extra), noise_off=noise_off)
    return cfg, env


def _np(t):
    return t.detach().double().cpu().numpy()


def _model_params(env, u_rfi=None):
    """the float64 model's parameters from the env's own float32 values (config struct, DR scales as they stand NOW)"""
    c, D, N = env._c, env.num_dof, env.num_envs
    f = lambda a: np.array([a[d] for d in range(D)], np.float64)
    p = env.simulator._params
    return dict(control_type=int(c.control_type), Kp=f(c.p_gains), Kd=f(c.d_gains), action_scale=f(c.action_scale), torque_limit=f(c.torque_limits),
                lo=np.array([c.hard_dof_pos_limits[d][0] for d in range(D)], np.float64), hi=np.array([c.hard_dof_pos_limits[d][1] for d in range(D)], np.float64),
                inertia=f(p.inertia), damping=f(p.damping), default=_np(env.default_dof_pos) if c.randomize_default_dof_pos else f(c.default_dof_pos),
                kp=_np(env._kp_scale), kd=_np(env._kd_scale), rfi_scale=_np(env._rfi_lim_scale), rao_scale=_np(env._rao_scale),
                u_rfi=None if (u_rfi is None or not c.randomize_torque_rfi) else np.asarray(u_rfi, np.float64), rfi_lim=float(c.rfi_lim), n_ps=None,
                ps_rfi_lim=0.0, use_rao=bool(c.use_rao), clip_torques=bool(c.clip_torques), enforce_limits=bool(p.enforce_limits),
                h=float(c.sim_dt), decimation=int(p.decimation))


def _prepare(env, sc):
    """reset, then the scenario's initial state: joints beyond a limit, envs about to run off their clip"""
    env.reset_all()
    s = env.simulator
    lim = s.hard_dof_pos_limits
    for e, d, side in sc["beyond_limit"]:
        s.dof_pos[e, d] = lim[d, side] + (0.05 if side else -0.05)
    for e in sc["ending"]:
        env.motion_start_times[e] = env.motion_len[e] - 3.5 * env.dt - env._episode_length_buf[e].float() * env.dt
    torch.cuda.synchronize()


def _run_case(cfgname, N, general, inject, prepare=None, after_step=None):
    """prepare(env) / after_step(env, k): the hooks of tests/test_gpu_parity.py's _env_step_vs_oracle.
    six steps; per step the kernel's frame, tau0 and the step's torques, next to the model's prediction from the kernel's OWN pre-step state"""
    cfg, env = _build(cfgname, N, general)
    D = env.num_dof
    sc = scenario(N, D, float(env._c.action_clip_value))
    assert 0.03 < sc["big_share"] < 0.07
    _prepare(env, sc)
    s = env.simulator
    s.set_debug_torques(True)
    if prepare is not None:
        prepare(env)
    out = []
    for k in range(sc["steps"]):
        u = torch.from_numpy(sc["u_rfi"][k]).to(env.device) if inject else None
        env.set_injected_draws(u_rfi=u)
        P = _model_params(env, sc["u_rfi"][k] if inject else None)
        pre = dict(q=_np(s.dof_pos), v=_np(s.dof_vel), queue=_np(env.action_queue), delay=env.action_delay_idx.cpu().numpy(),
                   ep=env._episode_length_buf.clone(), start=env.motion_start_times.clone(), ids=env.motion_ids.clone())
        a_del = model.delayed_action(sc["actions"][k], float(env._c.action_clip_value), pre["queue"], pre["delay"], bool(env._c.randomize_ctrl_delay))
        m = model.substeps(pre["q"], pre["v"], a_del, P)
        terms = model.torque_terms(pre["q"], pre["v"], a_del, P)
        env.step({"actions": torch.from_numpy(sc["actions"][k]).to(env.device)})
        torch.cuda.synchronize()
        if after_step is not None:
            after_step(env, k)
        out.append(dict(P=P, pre=pre, model=m, terms=terms, a_del=a_del, reset=env.reset_buf.bool().cpu().numpy(), time_outs=int(env.time_out_buf.sum()),
                        frame_q=_np(s.replay["dof_pos"][0]), frame_v=_np(s.replay["dof_vel"][0]), frame_root=s.replay["root"][0].clone(),
                        frame_contact=s.replay["contact"][0].clone(), dof_pos=_np(s.dof_pos), dof_vel=_np(s.dof_vel), root=s.robot_root_states.clone(),
                        tau0=_np(s.tau0), torques=_np(env.torques)))
    return env, sc, out


_RUNS = {}


def _case(cfgname, N, general, inject=True):
    key = (cfgname, N, general, inject)
    if key not in _RUNS:
        _RUNS[key] = _run_case(cfgname, N, general, inject)
    return _RUNS[key]


@pytest.mark.parametrize("cfgname,N,general", CASES)
def test_integrator_equals_the_model_one_step_at_a_time(cfgname, N, general):
    """From the kernel's own post-step state of step k - 1 (resets included), the queue peeked before step k and the scales, the model's (q, v)
    after the sub-steps is the frame step k consumed.  Per element, in float64 from magnitudes:
        v: 32 eps (max_s |v_s| + h tau_lim / I)          q: that x decimation h + 8 eps |q|          eps = 2^-24
    An element whose float64 pre-clamp position lies within 1e-5 rad of a limit is skipped (the outward-velocity zeroing is discontinuous
    there); the skipped share stays <= 0.5 %."""
    env, sc, steps = _case(cfgname, N, general)
    skipped = total = time_outs = clipped = limited = 0
    for k, r in enumerate(steps):
        P, m = r["P"], r["model"]
        tol_v = 32 * EPS * (m["vmax"] + P["h"] * P["torque_limit"] / P["inertia"])
        tol_q = tol_v * P["decimation"] * P["h"] + 8 * EPS * np.abs(m["q"])
        ok = m["margin"] >= 1e-5
        skipped += int((~ok).sum()); total += ok.size
        ev, eq = np.abs(r["frame_v"] - m["v"]), np.abs(r["frame_q"] - m["q"])
        print(f"{cfgname} step {k}: worst |dv| / tol {float((ev / tol_v)[ok].max()):.3f}, worst |dq| / tol {float((eq / tol_q)[ok].max()):.3f}, "
              f"skipped {int((~ok).sum())}, resets {int(r['reset'].sum())}, time-outs {r['time_outs']}")
        assert not (ev > tol_v)[ok].any(), (k, float((ev / tol_v)[ok].max()), np.argwhere((ev > tol_v) & ok)[:5].tolist())
        assert not (eq > tol_q)[ok].any(), (k, float((eq / tol_q)[ok].max()), np.argwhere((eq > tol_q) & ok)[:5].tolist())
        # ... and the step consumed that frame: the state it left for the envs that did not reset IS the frame
        keep = ~r["reset"]
        assert np.array_equal(r["dof_pos"][keep], r["frame_q"][keep]) and np.array_equal(r["dof_vel"][keep], r["frame_v"][keep])
        time_outs += r["time_outs"]
        tl = P["torque_limit"]
        clipped += int((np.abs(r["terms"][3]) > tl)[:, list(LOWERED)].sum())
        limited += int(((m["q"] == P["lo"]) | (m["q"] == P["hi"])).sum())
    assert skipped <= 0.005 * total, (skipped, total)
    assert time_outs > 0, "no env timed out inside the six steps"
    assert clipped > 0 and limited > 0, "the torque clip / the joint limits never bound"
    assert sum(int(r["reset"].sum()) for r in steps) < len(steps) * N, "every env reset in every step: nothing was compared"


@pytest.mark.parametrize("inject", [True, False])
@pytest.mark.parametrize("cfgname,N,general", CASES)
def test_first_substep_torque_is_the_steps_torque(cfgname, N, general, inject):
    """tau0 of the simulator's launch against the `torques` the step itself computed, per element within
    8 eps (|kp term| + |kd term| + tau_lim (|rfi| + |ps_tau| + |rao|)); with the in-kernel draw (inject False) this holds only if both
    launches key Philox with the same (seed, env, step counter, stream, dof)."""
    env, sc, steps = _case(cfgname, N, general, inject)
    c = env._c
    for k, r in enumerate(steps):
        P = r["P"]
        t_p, t_d, noise, _ = r["terms"]
        tl = P["torque_limit"]
        rfi = (np.abs(np.asarray(P["u_rfi"]) * 2 - 1) if P["u_rfi"] is not None else np.ones_like(t_p)) * P["rfi_lim"] * P["rfi_scale"] * bool(c.randomize_torque_rfi)
        bound = 8 * EPS * (np.abs(t_p) + np.abs(t_d) + tl * (rfi + np.abs(P["rao_scale"]) * bool(c.use_rao)))
        keep = ~r["reset"]
        err = np.abs(r["tau0"] - r["torques"])
        print(f"{cfgname} inject {inject} step {k}: worst |tau0 - torques| / bound {float((err / np.maximum(bound, 1e-30))[keep].max()):.3f}")
        assert not (err > bound)[keep].any(), (k, float(err[keep].max()))
        if inject and P["control_type"] == 0:
            # the float64 model's torque too, from the same draws.  Against float64 the bound needs one more term: the float32 sum
            # (a scale + default - q) inside the kp term is rounded twice at the magnitude of its operands, not of its (cancelling) result,
            # and that error is multiplied by kp Kp: 4 eps kp Kp (|a scale| + |default| + |q|)
            inner = np.abs(r["a_del"] * P["action_scale"]) + np.abs(P["default"]) + np.abs(r["pre"]["q"])
            bound_m = bound + 4 * EPS * P["kp"] * P["Kp"] * inner
            errm = np.abs(r["tau0"] - r["model"]["tau0"])
            print(f"   against the float64 model: worst / bound {float((errm / bound_m).max()):.3f}")
            assert not (errm > bound_m).any(), (k, float(errm.max()))
    assert bool(c.randomize_torque_rfi) and float(c.rfi_lim) > 0


@pytest.mark.parametrize("cfgname,N,general", CASES)
def test_root_and_contact_of_the_frame(cfgname, N, general):
    """the root the step consumed = the library's root body at (episode_length + 2) dt + start (pre-step values) + env origin; the contact frame
    holds contact_force or 0 on the feet's z and 0 everywhere else"""
    from tests.test_gpu_parity import close

    env, sc, steps = _case(cfgname, N, general)
    feet = env.feet_indices.cpu().tolist()
    cf = env.simulator.contact_force
    on = 0
    for k, r in enumerate(steps):
        pre = r["pre"]
        t = (pre["ep"] + 2).float() * env.dt + pre["start"]
        ref = env._motion_lib.get_motion_state(pre["ids"], t, offset=env.env_origins)
        want = torch.cat([ref["root_pos"], ref["root_rot"], ref["root_vel"], ref["root_ang_vel"]], dim=1)
        keep = torch.from_numpy(~r["reset"])
        tol = torch.full((N, 13), 3e-5)
        tol[:, 3:7] = 2e-4
        close(r["root"].cpu()[keep], want.cpu()[keep], tol[keep], f"{cfgname} step {k} root", rtol=3e-5)
        close(r["frame_root"].cpu(), want.cpu(), tol, f"{cfgname} step {k} frame root", rtol=3e-5)
        c = r["frame_contact"].cpu()
        z = c[:, feet, 2]
        assert bool(((z == cf) | (z == 0)).all())
        on += int((z == cf).sum())
        rest = c.clone()
        rest[:, feet, 2] = 0
        assert float(rest.abs().max()) == 0.0
        if "contact_mask" in ref:
            assert torch.equal(z.bool(), (ref["contact_mask"] > 0.5).cpu())
    assert on > 0, "no foot was ever in contact"


def test_the_loop_is_closed():
    """20 steps at N = 64, DR and noise off: with a* = (q_ref(next) - q_default) / action_scale the final mean |dif_joint_angles| is smaller
    than with zero actions — asserted only after the float64 model shows that ordering for the same inputs.
    Measured (v1 walk, inertia 0.04 .. 0.3, damping 0.05): see DESIGN.md §8."""
    N, T = 64, 20
    res = {}
    for policy in ("track", "zero"):
        cfg, env = _build(WALK, N, False, dr=False)
        env.reset_all()
        s, D = env.simulator, env.num_dof
        env.motion_start_times.zero_()
        env._episode_length_buf.zero_()
        torch.cuda.synchronize()
        P = _model_params(env)
        qm, vm = _np(s.dof_pos), _np(s.dof_vel)
        scale = torch.tensor(P["action_scale"], dtype=torch.float32, device=env.device)
        qdef = torch.tensor(P["default"], dtype=torch.float32, device=env.device)
        resets = 0
        for k in range(T):
            t = (env._episode_length_buf + 2).float() * env.dt + env.motion_start_times
            qref = env._motion_lib.get_motion_state(env.motion_ids, t, offset=env.env_origins)["dof_pos"]
            a = ((qref - qdef) / scale).contiguous() if policy == "track" else torch.zeros(N, D, device=env.device)
            r = model.substeps(qm, vm, model.delayed_action(_np(a), float(env._c.action_clip_value), None, None, False), P)
            qm, vm = r["q"], r["v"]
            env.step({"actions": a})
            torch.cuda.synchronize()
            resets += int(env.reset_buf.sum())
        assert resets == 0, "an env reset inside the 20 steps: the model below does not follow resets"
        res[policy] = (float(np.linalg.norm(_np(qref) - qm, axis=1).mean()), float((qref - s.dof_pos).norm(dim=1).mean()))
    print(f"closed loop, final mean |dif_joint_angles|: track model {res['track'][0]:.5f} kernel {res['track'][1]:.5f}; "
          f"zero actions model {res['zero'][0]:.5f} kernel {res['zero'][1]:.5f}")
    assert res["track"][0] < res["zero"][0], ("the float64 model does not show the ordering", res)
    assert res["track"][1] < res["zero"][1], res


def _rollouts(rollout_graph, rollouts=3):
    """MHPPO at 64 envs, 8 steps per rollout, `_training_step` after every rollout (a fixed permutation per iteration), through the agents'
    rollout driver; in the style of tests/test_gpu_parity.py _rollouts_with_split"""
    from pbhc_amd.agents.mh_ppo import MHPPO

    flags = {"PBHC_ROLLOUT_GRAPH": "1" if rollout_graph else "0", "PBHC_ROLLOUT_SPLIT": "1", "PBHC_CRITIC_BATCHED": "1", "PBHC_FUSED_SAMPLE": "1"}
    os.environ.update(flags)
    try:
        cfg, env = _build(WALK, 64, False, extra={"algo.config.num_steps_per_env": 8}, seed=11, noise_off=False)
        algo = MHPPO(env=env, config=cfg.algo.config, log_dir=None, device=DEV)
        algo.setup()
        algo._train_mode()
        obs = env.reset_all()
        used = []
        gperm = torch.Generator().manual_seed(23)
        start = algo._pflat.clone()
        for r in range(rollouts):
            algo.storage.clear()
            obs = algo._rollout_step(obs)
            used.append(bool(getattr(algo, "_rollout_used_graph", False)))
            n = algo.storage.num_envs * algo.storage.num_transitions_per_env
            algo._training_step(indices=torch.randperm(n, generator=gperm).to(DEV))
        torch.cuda.synchronize()
        out = {k: getattr(algo, k).clone() for k in ("_pflat", "_mflat", "_vflat", "_lr", "_adam_step")}
        out.update(dof_state=env.simulator.dof_state.clone(), root=env.simulator.robot_root_states.clone(), globals=env.globals.clone(),
                   frame_q=env.simulator.replay["dof_pos"].clone(), actions=algo.storage.actions.clone(), rewards=algo.storage.rewards.clone())
        return out, used, start
    finally:
        for k in flags:
            os.environ.pop(k, None)


def test_captured_rollout_equals_the_eager_loop():
    """the simulator's launch inside the rollout hipGraph (one frame, device cursor % 1): weights, Adam moments and dof_state bit-identical to
    the step-by-step loop"""
    a, used_a, start = _rollouts(True)
    b, used_b, _ = _rollouts(False)
    assert used_a == [False, True, True] and not any(used_b)
    assert not torch.equal(a["_pflat"], start)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_resume_is_bit_identical():
    """six env steps in one run; in a second run three steps, state_dict(), a fresh env, load_state_dict(), three more"""
    N = 70
    sc = scenario(N, 23, 100.0)

    def steps(env, ks):
        for k in ks:
            obs, _, _, _ = env.step({"actions": torch.from_numpy(sc["actions"][k]).to(env.device)})
        torch.cuda.synchronize()
        return obs

    _, env_a = _build(WALK, N, False, seed=5, noise_off=False)
    _prepare(env_a, sc)
    obs_a = steps(env_a, range(6))
    _, env_b = _build(WALK, N, False, seed=5, noise_off=False)
    _prepare(env_b, sc)
    steps(env_b, range(3))
    sd = env_b.state_dict()
    _, env_c = _build(WALK, N, False, seed=5, noise_off=False)
    env_c.load_state_dict(sd)
    obs_c = steps(env_c, range(3, 6))
    for k in obs_a:
        assert torch.equal(obs_a[k], obs_c[k]), k
    assert torch.equal(env_a.simulator.dof_state, env_c.simulator.dof_state)
    assert torch.equal(env_a.reset_buf, env_c.reset_buf)
    assert torch.equal(env_a.simulator.robot_root_states, env_c.simulator.robot_root_states)
    assert int(env_a._episode_length_buf.min()) < 6, "no env reset inside the six steps"


def test_dof_far_pre_pass_reads_the_frame_the_simulator_just_wrote():
    """terminate_when_dof_far with the simulator: the pre-pass's decision is norm(dif_joint_angles) > threshold of the step's OWN frame — it
    would see the previous step's frame if the simulator's launch came after it"""
    from pbhc_amd import _lib

    K = _lib.K
    N = 70
    TC = "env.config.termination_curriculum.terminate_when_dof_far_curriculum."
    cfg, env = _build(WALK, N, False, extra={"env.config.termination.terminate_when_dof_far": True, TC + "enable": False})
    sc = scenario(N, env.num_dof, float(env._c.action_clip_value))
    env.reset_all()
    s = env.simulator
    fired = []
    for k in range(sc["steps"]):
        t = (env._episode_length_buf + 2).float() * env.dt + env.motion_start_times
        qref = env._motion_lib.get_motion_state(env.motion_ids, t, offset=env.env_origins)["dof_pos"]
        # the threshold of this step: 5 % above / below the largest norm the PREVIOUS frame would give, alternating — a pre-pass that read the
        # old frame would fire on every odd step and on no even one
        norm_prev = (qref - s.replay["dof_pos"][0]).norm(dim=1)
        thr = float(norm_prev.max()) * (1.05 if k % 2 == 0 else 0.95)
        env.globals[K["PBHC_G_DOF_FAR_THR"]] = thr
        env.step({"actions": torch.from_numpy(sc["actions"][k]).to(env.device)})
        torch.cuda.synchronize()
        norm_new = (qref - s.replay["dof_pos"][0]).norm(dim=1)
        want = bool((norm_new > thr).any())
        got = float(env.read_log()["terminate_by_dof_far"]) > 0
        fired.append((want, k % 2 == 1, got))
        print(f"dof-far step {k}: threshold {thr:.4f}, largest norm of the new frame {float(norm_new.max()):.4f}, of the old one {float(norm_prev.max()):.4f}, fired {got}")
        assert got == want, (k, fired, float(norm_new.max()), thr)
        if want:
            assert bool(env.reset_buf.all())
    assert any(f[0] for f in fired) and not all(f[0] for f in fired), fired
    assert any(f[0] != f[1] for f in fired), ("the old frame would have given the same decisions: the test shows no ordering", fired)


def test_subtree_inertia_through_bind_and_its_refusal():
    """`inertia: "subtree"` end to end: the skeleton from the G1 MJCF, the default pose through pbhc_sim_fk on one env inside bind(), against
    the same formula on the CPU oracle's FK.  Bound: the two FKs are float32 chains of at most 8 links, so a link origin differs by < 1e-6 m;
    with all 35 kg at a lever of at most 1 m that moves an inertia by at most 2 r dp sum(m) = 7e-5 kg m^2 -> 1e-4.  Without link masses (the
    fixture's skeleton JSON) the env's construction refuses by name."""
    from oracle.fk import sim_fk
    from pbhc_amd import _lib
    from pbhc_amd.simulator import joint_sim as js

    mj = {"robot.motion.asset.assetFileName": "mjcf/g1_23dof_lock_wrist_fitmotionONLY.xml",
          "simulator.config.joint_sim": {"inertia": "subtree", "armature": 0.02, "damping": 0.05}}
    cfg, env = _build(WALK, 8, False, dr=False, extra=mj)
    sk = env.skeleton
    assert float(sk.body_mass.sum()) < 36.0
    rc = cfg.robot
    q0 = torch.tensor([[float(rc.init_state.default_joint_angles[n]) for n in rc.dof_names]])
    root = torch.zeros(1, 13)
    root[0, 6] = 1.0
    d = dict(parents=sk.parents, offsets=sk.offsets, local_rot_wxyz=sk.local_rot_wxyz, dof_axis=sk.dof_axis, num_bodies=sk.num_bodies)
    pos, rot, _, _ = sim_fk(d, root, q0, torch.zeros_like(q0))
    want = js.subtree_inertia(sk, pos[0].numpy(), rot[0].numpy(), 0.02)
    got = env.simulator.inertia
    print("subtree inertia, worst difference", float(np.abs(got - want).max()), "largest", float(want.max()), "smallest", float(want.min()))
    assert np.abs(got - want).max() < 1e-4
    assert want.max() > 0.3 and abs(want.min() - 0.02) < 1e-3            # the hips carry a leg; the last link of a chain carries nothing
    env.reset_all()
    env.step({"actions": torch.zeros(8, env.num_dof, device=env.device)})
    torch.cuda.synchronize()
    assert bool(torch.isfinite(env.simulator.dof_state).all())
    with pytest.raises(_lib.PbhcError, match=r'joint_sim\.inertia: "subtree" needs the link masses'):
        _build(WALK, 8, False, dr=False, extra={"simulator.config.joint_sim": {"armature": 0.02}})
