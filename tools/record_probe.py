"""The evaluation recorder under the profiler, and the wall time of the batched scoring.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/record_probe.py steps ENVS
        reset_all + 20 control steps of the v1 walk config with env.config.save_motion on (save_total_steps 16): one k_env_step,
        one k_env_finalize and one k_record_motion dispatch per step; the recorder writes a frame in 16 of them
  python3 tools/record_probe.py summary DIR [DIR ...]
        per directory: median (minimum) of the dispatches of the three kernels, microseconds, and the recorder's algorithmic bytes / bandwidth
  python3 tools/record_probe.py score EPISODES [FRAMES]
        records EPISODES envs x FRAMES steps, then times metrics.eval_batch_traj_device (device buffers) against metrics.eval_batch_traj
        (the Python loop over episodes, fed the host copy)
"""
import csv
import glob
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T_PROBE = 16


def _env(num_envs, total_steps):
    import torch

    from pbhc_amd.envs.motion_tracking import LeggedRobotMotionTracking
    from pbhc_amd.utils.config import load_config

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ov = {"num_envs": num_envs, "simulator._target_": "pbhc_amd.simulator.replay_stub.ReplaySimStub", "env.config.save_motion": True,
          "env.config.save_total_steps": total_steps, "env.config.save_note": "probe", "env.config.eval_timestamp": "probe",
          "env.config.ckpt_dir": tempfile.mkdtemp(prefix="record_probe_")}
    cfg = load_config(os.path.join(root, "tests", "golden", "configs", "v1_g1_23dof_walk.yaml"), ov, now="probe")
    torch.manual_seed(0)
    env = LeggedRobotMotionTracking(cfg.env.config, "cuda:0")
    env._write_to_file = False
    return env


def frame_bytes(env):
    """algorithmic bytes of one recorded frame of one env: (read, written)"""
    rows = env.layout.record["rows"]
    written = sum((8 if k == "terminate" else 4) * int(__import__("numpy").prod(s, dtype="int64")) for k, s in rows.items())
    D = env.num_dof
    read = 4 * (rows["actor_obs"][0] + 13 + 2 * D + D + 2 + 3 + 1) + 8 + 8          # obs row, root state, dof state, actions, contacts, origin, start, 2 x int64
    return read, written


def steps(num_envs):
    import torch

    import bench

    env = _env(num_envs, T_PROBE)
    env.reset_all()
    env.simulator.set_replay(*bench.make_replay_on_device(env, 24, seed=1))
    a = torch.zeros(num_envs, env.num_dof, device="cuda:0")
    for _ in range(20):
        env.step({"actions": a})
    torch.cuda.synchronize()
    r, w = frame_bytes(env)
    print(f"envs {num_envs}: recorder frame {r} B read + {w} B written per env, specialised={env.is_specialised}, recorded={env.motion_recorded}")


def summary(dirs):
    for d in dirs:
        f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
        rows = list(csv.DictReader(open(f)))
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        print(d)
        for name in ("k_env_step", "k_env_finalize", "k_record_motion"):
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
            if name == "k_record_motion":            # dispatches 3 .. 3 + T_PROBE - 1 write a frame, the others only advance / read the counter
                wr, idle = us[3:3 + T_PROBE], us[:3] + us[3 + T_PROBE:]
                print(f"  {name:16s} writing a frame: median {statistics.median(wr):7.2f} (min {min(wr):7.2f}) us over {len(wr)}; "
                      f"not writing: median {statistics.median(idle):6.2f} us over {len(idle)}")
            else:
                print(f"  {name:16s} median {statistics.median(us[2:]):7.2f} (min {min(us[2:]):7.2f}) us over {len(us[2:])} of {len(us)} dispatches")


def score(episodes, frames):
    import torch

    import bench
    from pbhc_amd.eval import metrics as M

    env = _env(episodes, frames)
    env.reset_all()
    env.simulator.set_replay(*bench.make_replay_on_device(env, frames + 8, seed=1))
    a = torch.zeros(episodes, env.num_dof, device="cuda:0")
    while not env.motion_recorded:
        env.step({"actions": a})
    rec, clip = env.recorded_motion_device(), env._motion_lib._clips[0]
    M.eval_batch_traj_device(env.skeleton, rec, clip)                 # warm-up (library load, first launches)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev = M.eval_batch_traj_device(env.skeleton, rec, clip)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    saved = env.saved_motion_dict
    t2 = time.perf_counter()
    loop = M.eval_batch_traj(env.skeleton, saved, clip, device="cuda:0")
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    same = all(dev["_raw"][i][p][k] == loop["_raw"][i][p][k] for i in range(episodes) for p in ("accuracy", "smoothness") for k in loop["_raw"][i][p])
    print(f"{episodes} episodes x {frames} frames: eval_batch_traj_device {1e3 * (t1 - t0):.1f} ms, eval_batch_traj {1e3 * (t3 - t2):.1f} ms "
          f"(+ {1e3 * (t2 - t1):.1f} ms device -> host copy), ratio {(t3 - t2) / (t1 - t0):.1f}x, tables identical: {same}")


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "steps":
        steps(int(sys.argv[2]))
    elif mode == "summary":
        summary(sys.argv[2:])
    else:
        score(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 200)
