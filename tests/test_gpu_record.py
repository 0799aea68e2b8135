"""The evaluation recorder on the GPU (env.config.save_motion: k_record_motion after every fused step, device-resident [N, T, ...] buffers)
and the batched scoring of its recordings: the reference's own saved_motion_dict, the drop-3 / stop semantics of the device-side counter,
graph == eager, off == absent, the .pkl file, eval_batch_traj_device == eval_batch_traj, MHPPO.evaluate_policy."""
import os

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from tests.helpers import GOLDEN, build_hip_env, clip_from_env_golden, load_state_into_hip_env, skel_from_golden, state_dict_from_golden
from tests.test_gpu_parity import angvel_tol, close, trace_slerp_bounds
from tests.test_record_cpu import ROTVEC_TOL

pytestmark = pytest.mark.gpu

WALK = "v1_g1_23dof_walk.yaml"
DEV = "cuda:0"
KEYS = ("root_trans_offset", "pose_aa", "dof", "root_rot", "actor_obs", "action", "terminate", "root_lin_vel", "root_ang_vel", "dof_vel",
        "contact_mask", "motion_times")
EPS32 = float(np.finfo(np.float32).eps)


def _record(tmp, T=8, **more):
    ov = {"env.config.save_motion": True, "env.config.save_total_steps": T, "env.config.save_note": "note", "env.config.eval_timestamp": "stamp",
          "env.config.ckpt_dir": str(tmp)}
    ov.update(more)
    return ov


def _skeleton():
    from pbhc_amd.skeleton import Skeleton

    return Skeleton.from_json(os.path.join(GOLDEN, "skeleton_g1_23dof_lock_wrist_fitmotionONLY.json"))


def test_recording_matches_the_reference_trace(tmp_path):
    """Replay of tests/golden/env_v1_walk_record.npz (tools/gen_record_golden.py): env.saved_motion_dict against the reference's, key by key.
    The reference's reset_all() before the trace recorded one step of its own, so its dict holds trace steps 2..9 and is complete after
    trace step 9; the HIP env's counter starts the trace at 1 likewise."""
    g = dict(np.load(f"{GOLDEN}/env_v1_walk_record.npz"))
    S, N, D = g["actions_in"].shape
    T = int(g["save_total_steps"])
    cfg, env = build_hip_env(WALK, N, overrides=_record(tmp_path, T))
    env._write_to_file = False
    assert env.save_motion
    load_state_into_hip_env(env, state_dict_from_golden(g), g)
    env._rec_counter[0] = 1                                               # the step of the reference's reset_all() (see above)
    env._rec_steps = 1
    tg = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.device)
    env.simulator.set_replay(tg(g["replay_root"]), tg(g["replay_dof_pos"]), tg(g["replay_dof_vel"]), tg(g["replay_contact"]))
    assert env.rollout_graph_safe(24) is True                             # the recorder does not keep the steps out of a graph
    from oracle.motion_lib import MotionLib as OML

    oml = OML(skel_from_golden(), [clip_from_env_golden(g)])
    first = 2                                                             # trace step of recorded frame 0
    root_tols, done_at, snap = [], None, None
    for k in range(S):
        st = lambda name, dt=torch.float32: tg(g["step__state__" + name][k]).to(dt)
        env.set_injected_draws(u_rfi=tg(g["step__u_rfi"][k]), start_time=st("motion_start_times"), kp=st("kp_scale"), kd=st("kd_scale"),
                               rfi_lim=st("rfi_lim_scale"), rao=st("rao_scale"), delay=st("action_delay_idx", torch.long))
        obs, rew, reset, extras = env.step({"actions": tg(g["actions_in"][k])})
        torch.cuda.synchronize()
        assert torch.equal(reset.cpu(), torch.from_numpy(g["step__reset_buf_out"][k])), f"step {k}: reset_buf"
        gs = lambda name, j: torch.from_numpy(g["state0__" + name] if j < 0 else g["step__state__" + name][j])
        _, root_tol = trace_slerp_bounds(oml, gs("episode_length_buf", k - 1), gs("motion_start_times", k - 1), gs("episode_length_buf", k),
                                         gs("motion_start_times", k), torch.from_numpy(g["step__reset_buf_out"][k]), float(env.dt), 2e-5)
        root_tols.append(root_tol)
        recorder_steps = k + 2                                            # reset_all's + trace steps 0..k
        # drop-3 and stop: complete after T + 3 recorder steps, not one earlier; later steps leave it alone
        assert env.motion_recorded == (recorder_steps >= T + 3) and hasattr(env, "saved_motion_dict") == (recorder_steps >= T + 3), k
        if recorder_steps == T + 3:
            done_at = k
            snap = {key: v.clone() for key, v in env.recorded_motion_device().items() if torch.is_tensor(v)}
    assert done_at == first + T - 1 and int(env._rec_counter[0]) == T + 3 and not bool(env._rec_counter[1:].any())
    assert env._record_launches == S
    for key, v in env.recorded_motion_device().items():
        if torch.is_tensor(v):
            assert torch.equal(v, snap[key]), f"{key} changed after the recording was complete"
    d = env.saved_motion_dict
    assert d is env.saved_motion_dict                                     # one host copy
    assert set(d) == set(KEYS)
    ref = {k: g["saved__" + k] for k in KEYS}
    for k in KEYS:
        assert d[k].shape == ref[k].shape and d[k].dtype == ref[k].dtype, (k, d[k].shape, ref[k].shape, d[k].dtype, ref[k].dtype)
    term = torch.from_numpy(ref["terminate"]).bool()                      # [N, T]
    assert term.any() and (ref["root_rot"][..., 3] < 0).any() and (~term).any()
    assert np.array_equal(d["terminate"], ref["terminate"])
    # copies of replayed state: equal for the envs that did not reset in the step; for those that did, the bounds the reset-trace tests
    # apply to the same state (tests/test_gpu_parity.py test_env_step_matches_reference_trace)
    keep = ~term
    for k in ("root_trans_offset", "root_rot", "dof", "dof_vel", "root_lin_vel", "root_ang_vel"):
        a, b = torch.from_numpy(d[k]), torch.from_numpy(ref[k])
        print(f"{k}: max |dev| surviving envs {float((a - b)[keep].abs().max()):.3e}, reset envs {float((a - b)[term].abs().max()):.3e}")
        assert torch.equal(a[keep], b[keep]), k
    a, b = torch.from_numpy(d["contact_mask"]), torch.from_numpy(ref["contact_mask"])
    print(f"contact_mask: max |dev| {float((a - b).abs().max()):.3e}")
    close(a, b, 3e-5, "contact_mask")
    for f in range(T):
        k = first + f
        w = f"frame {f} (trace step {k}): "
        close(d["root_trans_offset"][:, f], ref["root_trans_offset"][:, f], 3e-5, w + "root_trans_offset", rtol=3e-5)
        close(d["root_rot"][:, f], ref["root_rot"][:, f], (root_tols[k] + 1e-5).expand(-1, 4), w + "root_rot", rtol=3e-5)
        close(d["root_lin_vel"][:, f], ref["root_lin_vel"][:, f], 3e-5, w + "root_lin_vel", rtol=3e-5)
        rw = torch.from_numpy(ref["root_ang_vel"][:, f])
        close(d["root_ang_vel"][:, f], rw, angvel_tol(rw, float(env._motion_lib._motion_dt[0]), k=32.0, base=3e-5), w + "root_ang_vel", rtol=3e-5)
        close(d["dof"][:, f], ref["dof"][:, f], 3e-5, w + "dof")
        close(d["dof_vel"][:, f], ref["dof_vel"][:, f], 3e-5, w + "dof_vel", rtol=1e-4)
        close(d["action"][:, f], ref["action"][:, f], 3e-5, w + "action")
        close(d["actor_obs"][:, f], ref["actor_obs"][:, f], 3e-5, w + "actor_obs")
    # motion_times = episode_length_buf * dt + motion_start_times (post-reset): to one float ulp of T x dt
    mt_err = np.abs(d["motion_times"].astype(np.float64) - ref["motion_times"].astype(np.float64)).max()
    print(f"motion_times: max |dev| {mt_err:.3e} (bound {float(np.spacing(np.float32(T * env.dt))):.3e})")
    assert mt_err <= float(np.spacing(np.float32(T * env.dt)))
    # pose_aa: rows 1..D are the exact products dof_axis * dof of the recorded dof, the extended bodies are zero, row 0 is the rotation
    # vector of the recorded root quaternion (scipy float64 on that quaternion; ROTVEC_TOL: tests/test_record_cpu.py)
    axis = np.asarray(skel_from_golden()["dof_axis"], np.float32)
    assert np.array_equal(d["pose_aa"][:, :, 1:D + 1], axis[None, None] * d["dof"][..., None])
    assert not d["pose_aa"][:, :, D + 1:].any() and d["pose_aa"].shape[2] == D + 1 + env.num_extend_bodies
    rv = Rotation.from_quat(d["root_rot"].reshape(-1, 4).astype(np.float64)).as_rotvec().reshape(N, T, 3)
    rv_err = np.abs(d["pose_aa"][:, :, 0].astype(np.float64) - rv).max()
    print(f"pose_aa row 0 vs scipy float64: max |dev| {rv_err:.3e} (bound {ROTVEC_TOL:.3e})")
    assert rv_err <= ROTVEC_TOL
    # ... and against the reference's own rows, through the bounds of the state they are made from (|d rotvec| <= 2 |dq| + ROTVEC_TOL away from
    # angle pi; the golden's angles stay below 2.5 rad)
    assert float(np.linalg.norm(ref["pose_aa"][:, :, 0], axis=-1).max()) < 2.5
    for f in range(T):
        close(d["pose_aa"][:, f, 0], ref["pose_aa"][:, f, 0], (4 * (root_tols[first + f] + 1e-5) + 2 * ROTVEC_TOL).expand(-1, 3), f"frame {f}: pose_aa row 0", rtol=3e-5)
        close(d["pose_aa"][:, f, 1:], ref["pose_aa"][:, f, 1:], 3e-5, f"frame {f}: pose_aa rows 1..")


def _rollout(env, actions, graph):
    """reset_all + len(actions) steps on a replay window, eagerly or as ONE captured graph"""
    import bench

    env.reset_all()
    env.simulator.set_replay(*bench.make_replay_on_device(env, len(actions) + 2, seed=5))
    outs = []
    if not graph:
        for a in actions:
            obs, rew, reset, _ = env.step({"actions": a})
            outs.append((obs["actor_obs"].clone(), rew.clone(), reset.clone(), env.simulator.robot_root_states.clone()))
        torch.cuda.synchronize()
        return outs
    assert env.rollout_graph_safe(len(actions))
    env.simulator.use_device_cursor()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=env.device)
    c0 = env.common_step_counter
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            for a in actions:
                env.step({"actions": a})
    torch.cuda.current_stream().wait_stream(side)
    env.common_step_counter = c0
    g.replay()
    env.after_graph_steps(len(actions))
    torch.cuda.synchronize()
    return outs


def _twin(tmp_path, overrides, N=512):
    torch.manual_seed(3)
    np.random.seed(3)
    return build_hip_env(WALK, N, noise_off=False, overrides=overrides)[1]


def test_recorder_inside_a_graph_equals_the_eager_loop(tmp_path):
    T, N = 12, 512
    recs = []
    for graph in (False, True):
        env = _twin(tmp_path, _record(tmp_path, T))
        env._write_to_file = False
        actions = 0.5 * torch.randn(T + 2, N, env.num_dof, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        _rollout(env, list(actions), graph)
        assert env.motion_recorded and env._record_launches == T + 3
        recs.append({k: v.clone() for k, v in env.recorded_motion_device().items() if torch.is_tensor(v)})
        assert int(env._rec_counter[0]) == T + 3
    assert recs[0]["terminate"].any(), "no env reset inside the window"
    for k in recs[0]:
        assert torch.equal(recs[0][k], recs[1][k]), k


def test_recorder_off_changes_nothing_and_launches_nothing(tmp_path):
    outs = {}
    for tag, ov in (("absent", {}), ("false", {"env.config.save_motion": False}), ("on", _record(tmp_path, 4))):
        env = _twin(tmp_path, ov, N=256)
        if tag == "on":
            env._write_to_file = False
        actions = 0.5 * torch.randn(6, 256, env.num_dof, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
        outs[tag] = _rollout(env, list(actions), graph=False)
        if tag != "on":
            assert env.save_motion is False and env._rec is None and env._record_launches == 0 and env.layout.record is None
            with pytest.raises(AttributeError):
                env.saved_motion_dict
        else:
            assert env._record_launches == 7
    for tag in ("false", "on"):             # (on: the recorder only reads what the step left)
        for s, (a, b) in enumerate(zip(outs["absent"], outs[tag])):
            for x, y in zip(a, b):
                assert torch.equal(x, y), (tag, s)


def test_recording_file(tmp_path):
    """{ckpt_dir}/motions/{save_note}_{eval_timestamp}_{N}x{T}-{motion_episode_length}.pkl, written by the step that completes the recording"""
    import joblib

    from pbhc_amd.eval import metrics as M

    T, N = 8, 16
    env = _twin(tmp_path, _record(tmp_path, T), N=N)
    actions = 0.5 * torch.randn(T + 2, N, env.num_dof, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    mel = int(env._motion_episode_length)
    assert mel == int(np.load(f"{GOLDEN}/env_v1_walk_record.npz")["motion_episode_length"])          # the same clip: the reference's 202
    path = tmp_path / "motions" / f"note_stamp_{N}x{T}-{mel}.pkl"
    _rollout(env, list(actions[:-1]), graph=False)
    assert not path.exists()
    env.step({"actions": actions[-1]})
    assert path.exists() and env.saved_motion_path == str(path)
    data = joblib.load(path)
    assert sorted(data) == sorted(f"motion{i}" for i in range(N))
    D, Bx, obs_dim = env.num_dof, env.skeleton.num_bodies_ext, env.obs_buf_dict["actor_obs"].shape[1]
    shapes = dict(root_trans_offset=(T, 3), pose_aa=(T, Bx, 3), dof=(T, D), root_rot=(T, 4), actor_obs=(T, obs_dim), action=(T, D), terminate=(T,),
                  root_lin_vel=(T, 3), root_ang_vel=(T, 3), dof_vel=(T, D), contact_mask=(T, 2), motion_times=(T,))
    for i in (0, N - 1):
        m = data[f"motion{i}"]
        assert set(m) == set(KEYS) | {"fps"} and m["fps"] == 1 / env.dt
        for k, shape in shapes.items():
            assert m[k].shape == shape and m[k].dtype == (np.int64 if k == "terminate" else np.float32), (k, m[k].shape, m[k].dtype)
            assert np.array_equal(m[k], env.saved_motion_dict[k][i])
    clip = env._motion_lib._clips[0]
    res = M.eval_batch_traj(_skeleton(), env.saved_motion_dict, clip, motion_len=T, device=DEV)
    assert len(res["_raw"]) == N and np.isfinite(res["accuracy"]["E_mpjpe"]["mean"])


def test_recorder_refuses_buffers_that_do_not_fit(tmp_path):
    from pbhc_amd import _lib

    with pytest.raises(_lib.PbhcError, match=r"bytes \(\d+\.\d+ GiB\)"):
        build_hip_env(WALK, 16, overrides=_record(tmp_path, 2_000_000_000))


# ---- batched scoring ---------------------------------------------------------------------------------------------------------------------
def _assert_same_table(dev_res, loop_res, N, T, B, D):
    """Both tables hold float means of non-negative float norms (x 1e3 in double).  Per episode the loop and the batch add the same terms
    in a different order: a sum of n non-negative floats carries a relative error of at most (n - 1) eps in ANY order, so two orders differ
    by at most 2 (n - 1) eps of the value; n <= T * B terms of the outer means + the D (or 3) squares inside a norm.  The means over
    episodes are formed in double from those values (same bound); std is 1-Lipschitz in the sup norm of its inputs, so it moves by at most
    the largest per-episode difference."""
    rel = 2.0 * (T * B + D) * EPS32
    worst = 0.0
    for part in ("accuracy", "smoothness"):
        assert set(dev_res[part]) == set(loop_res[part])
        big = 0.0
        for key in loop_res[part]:
            a = np.array([dev_res["_raw"][i][part][key] for i in range(N)])
            b = np.array([loop_res["_raw"][i][part][key] for i in range(N)])
            lim = rel * np.abs(b)
            worst = max(worst, float((np.abs(a - b) / np.maximum(lim, 1e-300)).max()) if (lim > 0).any() else 0.0)
            assert (np.abs(a - b) <= lim).all(), (part, key, float(np.abs(a - b).max()), float(lim.max()))
            big = float(np.abs(a - b).max())
            assert abs(dev_res[part][key]["mean"] - loop_res[part][key]["mean"]) <= rel * abs(loop_res[part][key]["mean"]), (part, key)
            assert abs(dev_res[part][key]["std"] - loop_res[part][key]["std"]) <= big + 1e-12 * abs(loop_res[part][key]["mean"]), (part, key)
    print(f"eval_batch_traj_device vs eval_batch_traj: worst difference / bound {worst:.3f} (relative bound {rel:.2e})")


def _synthetic_recording(clip, N, T, D, seed):
    rng = np.random.default_rng(seed)
    pose = np.asarray(clip["pose_aa"], np.float32)
    trans = np.asarray(clip["root_trans_offset"], np.float32)
    F = pose.shape[0]
    start = rng.integers(0, F - T, size=N)
    idx = start[:, None] + np.arange(T)[None]
    fps = int(clip["fps"])
    rec = dict(pose_aa=(pose[idx] + 0.02 * rng.standard_normal((N, T) + pose.shape[1:])).astype(np.float32),
               root_trans_offset=(trans[idx] + 0.02 * rng.standard_normal((N, T, 3))).astype(np.float32),
               motion_times=(idx / fps).astype(np.float32), contact_mask=(rng.random((N, T, 2)) < 0.5).astype(np.float32),
               terminate=np.zeros((N, T), np.int64))
    rec["dof"] = rec["pose_aa"][:, :, 1:D + 1].sum(-1).astype(np.float32)      # (single-axis hinges: the angle up to the axis' sign)
    return rec


@pytest.mark.parametrize("case", ["golden", "synthetic64"])
def test_batched_scoring_equals_the_loop(case):
    from pbhc_amd.eval import metrics as M

    sk = _skeleton()
    g = dict(np.load(f"{GOLDEN}/env_v1_walk_record.npz"))
    clip = clip_from_env_golden(g)
    if case == "golden":
        saved = {k: g["saved__" + k] for k in KEYS}
    else:
        saved = _synthetic_recording(clip, 64, 40, sk.num_dof, seed=6)
    N, T = saved["pose_aa"].shape[:2]
    loop = M.eval_batch_traj(sk, saved, clip, motion_len=T, device=DEV)
    rec = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in saved.items()}
    dev = M.eval_batch_traj_device(sk, rec, clip, motion_len=T)
    assert len(dev["_raw"]) == N
    _assert_same_table(dev, loop, N, T, sk.num_bodies, sk.num_dof)


def test_evaluate_policy_records_and_scores(tmp_path):
    import bench
    from pbhc_amd.agents.mh_ppo import MHPPO
    from pbhc_amd.eval import metrics as M

    torch.manual_seed(5)
    np.random.seed(5)
    T, N = 40, 64
    cfg, env = build_hip_env(WALK, N, noise_off=False, overrides=_record(tmp_path, T))
    algo = MHPPO(env=env, config=cfg.algo.config, log_dir=None, device=DEV)
    algo.setup()
    env.simulator.set_replay(*bench.make_replay_on_device(env, T + 8, seed=7))
    obs = algo.evaluate_policy()
    assert set(obs) == set(env.obs_buf_dict) and env.motion_recorded and env._rec_steps == T + 3
    assert algo._eval_used_graph
    em = algo.eval_metrics
    assert len(em["_raw"]) == N and {"accuracy", "smoothness", "first_termination_ratio"} <= set(em)
    assert em["first_termination_ratio"] == M.first_termination_ratio(env.saved_motion_dict["terminate"])
    assert all(np.isfinite(v["mean"]) for v in em["accuracy"].values())
    assert os.path.exists(env.saved_motion_path)
    # the same numbers from the host copy through the yardstick loop
    loop = M.eval_batch_traj(env.skeleton, env.saved_motion_dict, env._motion_lib._clips[0], motion_len=T, device=DEV)
    _assert_same_table(em, loop, N, T, env.skeleton.num_bodies, env.skeleton.num_dof)
