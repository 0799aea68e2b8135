"""k_joint_sim / k_articulated_sim / k_floating_sim under the profiler, next to the two kernels of the same mapping (k_dof_far_any, k_clip_stats).

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/joint_sim_probe.py steps ENVS [joint|articulated|both|replay|floating|floating-dr]
        reset_all + 20 control steps of the v1 walk config on one stream with terminate_when_dof_far and clip_statistics on: per step one
        k_joint_sim (joint) or k_articulated_sim (articulated: the G1 MJCF, armature 0.02, damping 0.05), one k_dof_far_any, one k_env_step,
        one k_env_finalize and one k_clip_stats dispatch; `both` runs the two simulators one after the other in ONE trace;
        floating: FloatingBaseSim (the G1 MJCF, armature 0.02, damping 0.05, eight sole points, slip velocity 0.6 m/s), floating-dr: the same
        with all four floating_sim.domain_rand flags on and push_robots as the config has it (floating: push_robots off)
  python3 tools/joint_sim_probe.py summary DIR [DIR ...]
        per directory: dispatches, median and minimum (microseconds) of those kernels
"""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SOLE = [[0.132, 0.026, -0.035], [0.132, -0.026, -0.035], [-0.054, 0.026, -0.035], [-0.054, -0.026, -0.035]]
KERNELS = ("k_joint_sim", "k_articulated_sim", "k_floating_sim", "k_dof_far_any", "k_clip_stats", "k_env_step", "k_env_finalize")


def steps(num_envs, sim):
    import torch

    import bench
    from pbhc_amd.envs.motion_tracking import LeggedRobotMotionTracking
    from pbhc_amd.utils.config import load_config

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ov = {"num_envs": num_envs, "env.config.clip_statistics": True, "env.config.termination.terminate_when_dof_far": True}
    if sim == "joint":
        ov.update({"simulator._target_": "pbhc_amd.simulator.joint_sim.JointSpaceSim",
                   "simulator.config.joint_sim": {"inertia": 0.1, "damping": 0.05}})
    elif sim == "articulated":
        ov.update({"simulator._target_": "pbhc_amd.simulator.articulated_sim.ArticulatedSim",
                   "simulator.config.articulated_sim": {"armature": 0.02, "damping": 0.05},
                   "robot.motion.asset.assetFileName": "mjcf/g1_23dof_lock_wrist_fitmotionONLY.xml"})
    elif sim in ("floating", "floating-dr"):
        spec = {"armature": 0.02, "damping": 0.05, "slip_velocity": 0.6, "contact_points": {"left_ankle_roll_link": SOLE, "right_ankle_roll_link": SOLE}}
        if sim == "floating-dr":
            spec["domain_rand"] = dict.fromkeys(("link_mass", "base_com", "friction", "push"), True)
        else:
            ov["domain_rand.push_robots"] = False
        ov.update({"simulator._target_": "pbhc_amd.simulator.floating_sim.FloatingBaseSim", "simulator.config.floating_sim": spec,
                   "robot.motion.asset.assetFileName": "mjcf/g1_23dof_lock_wrist_fitmotionONLY.xml"})
    else:
        ov["simulator._target_"] = "pbhc_amd.simulator.replay_stub.ReplaySimStub"
    cfg = load_config(os.path.join(root, "tests", "golden", "configs", "v1_g1_23dof_walk.yaml"), ov, now="probe")
    torch.manual_seed(0)
    env = LeggedRobotMotionTracking(cfg.env.config, "cuda:0")
    env.reset_all()
    if sim == "replay":
        env.simulator.set_replay(*bench.make_replay_on_device(env, 24, seed=1))
    g = torch.Generator(device="cuda:0").manual_seed(1)
    for _ in range(20):
        env.step({"actions": torch.randn(num_envs, env.num_dof, device="cuda:0", generator=g)})
    torch.cuda.synchronize()
    print(f"envs {num_envs}, sim {sim}: specialised={env.is_specialised}, joint_pos_diff_norm {float(env.read_log()['joint_pos_diff_norm']):.4f}")


def summary(dirs):
    for d in dirs:
        rows = {k: [] for k in KERNELS}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    name = r["Kernel_Name"]
                    for k in KERNELS:
                        if k in name:
                            rows[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
        print(d)
        for k in KERNELS:
            v = rows[k]
            if v:
                print(f"  {k:16s} dispatches {len(v):4d}  median {statistics.median(v):7.2f} us  min {min(v):7.2f} us")
            else:
                print(f"  {k:16s} dispatches    0")


if __name__ == "__main__":
    if sys.argv[1] == "steps":
        which = sys.argv[3] if len(sys.argv) > 3 else "joint"
        for sim in (("joint", "articulated") if which == "both" else (which,)):
            steps(int(sys.argv[2]), sim)
    elif sys.argv[1] == "summary":
        summary(sys.argv[2:])
    else:
        raise SystemExit(__doc__)
