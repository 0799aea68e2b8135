#!/usr/bin/env python
"""Train MHPPO in the closed loop of JointSpaceSim (pbhc_amd/simulator/joint_sim.py), ArticulatedSim (pbhc_amd/simulator/articulated_sim.py)
or FloatingBaseSim (pbhc_amd/simulator/floating_sim.py) and print whether the tracking error moves.

    python tools/closed_loop_train.py --config tests/golden/configs/v1_g1_23dof_walk.yaml --envs 1024 --iters 300 --sim joint

Its own loop, not bench.py: rollout (timed with an event pair) -> update, and per iteration one line with
    joint_diff   the batch mean of |dif_joint_angles| (rad) of the rollout's last step, as the step kernel logs it (joint_pos_diff_norm)
    r_joint_pos  the batch mean of the joint-position reward term exp(-mean(dif^2) / sigma) of that step, over the envs that did not reset in
                 it, recomputed here from the state the step left and the adaptive sigma it used
    rollout_ms   the rollout's time on the device
`--sim replay` runs the same loop on ReplaySimStub with a synthetic replay window, where actions do not move the state: the reference point
for rollout_ms, and the control for the two tracking figures (they must NOT move there).

The joint simulator is no physics engine (no gravity, no coupling between joints, no contact dynamics; the root rides the clip): a falling
error here shows that the loop action -> torque -> joint state -> observation -> reward is closed and that PPO can use it, nothing more.
`--sim articulated` runs the robot's tree with the MJCF's masses and inertia tensors under gravity and the gantry's accelerations (armature and
damping from the same flags; --inertia is not used): still no free root, no contact dynamics, no balance.
`--sim floating` frees the root and lets the ground push back at the four corners of each sole of the G1 (the corners of the footprint of the
foot's collision capsules, friction 0.8): the robot can fall, and the loop prints per iteration, after the columns above,
    ended_by     the share of the episodes that ended in the rollout's last step by gravity / motion-far / time-out / motion-end (the step
                 kernel's batch means of its termination flags, normalised to their sum; "-" when no episode ended in that step)
The contact defaults (stiffness 10000 N/m and normal damping 100 N s/m per point, slip velocity 0.4 m/s) pass the stability screen at the
config's 200 Hz with a static sink of 0.39 cm; `--sim-fps F` raises sim.fps to F and the decimation with it (F must be a multiple
of the config's fps), which a stiffer ground or a smaller slip velocity needs, and says so.
`--randomize` (with --sim floating) turns on simulator.config.floating_sim.domain_rand.{link_mass, base_com, friction}: every env integrates
its own link masses, torso centre of mass and friction coefficient, the ones the critic observes; the stability screen is then taken at
friction_range[1] = 1.2, which the default slip velocity does not pass at 200 Hz, so the default becomes 0.6 m/s (and is printed).
`--push` turns on domain_rand.push and leaves the config's push_robots as it is; without it push_robots is switched off.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build(args):
    from pbhc_amd.agents.mh_ppo import MHPPO
    from pbhc_amd.envs.motion_tracking import LeggedRobotMotionTracking
    from pbhc_amd.utils.config import load_config

    ov = {"num_envs": args.envs}
    if args.sim == "joint":
        ov["simulator._target_"] = "pbhc_amd.simulator.joint_sim.JointSpaceSim"
        inertia = "subtree" if args.inertia == "subtree" else float(args.inertia)
        ov["simulator.config.joint_sim"] = {"inertia": inertia, "armature": args.armature, "damping": args.damping}
        if args.mjcf:                                         # "subtree" needs the link masses: the skeleton from the MJCF
            ov["robot.motion.asset.assetFileName"] = args.mjcf
    elif args.sim == "articulated":
        ov["simulator._target_"] = "pbhc_amd.simulator.articulated_sim.ArticulatedSim"
        ov["simulator.config.articulated_sim"] = {"armature": args.armature, "damping": args.damping}
        if args.mjcf:                                         # the masses and inertia tensors: the skeleton from the MJCF
            ov["robot.motion.asset.assetFileName"] = args.mjcf
    elif args.sim == "floating":
        ov["simulator._target_"] = "pbhc_amd.simulator.floating_sim.FloatingBaseSim"
        slip = args.slip_velocity if args.slip_velocity is not None else (0.6 if args.randomize else 0.4)
        flags = dict.fromkeys(("link_mass", "base_com", "friction"), bool(args.randomize))
        flags["push"] = bool(args.push)
        ov["simulator.config.floating_sim"] = {"armature": args.armature, "damping": args.damping, "stiffness": args.stiffness,
                                               "normal_damping": args.normal_damping, "friction": args.friction, "slip_velocity": slip,
                                               "contact_points": {"left_ankle_roll_link": G1_SOLE, "right_ankle_roll_link": G1_SOLE},
                                               "domain_rand": flags}
        if not args.push:
            ov["domain_rand.push_robots"] = False             # (without --push the simulator does not push)
        print(f"# floating_sim: slip_velocity {slip} m/s, domain_rand " + " ".join(f"{k}={int(v)}" for k, v in flags.items()))
        if args.mjcf:
            ov["robot.motion.asset.assetFileName"] = args.mjcf
        if args.sim_fps:
            base = load_config(args.config, {}, now="closed_loop").simulator.config.sim
            if args.sim_fps % int(base.fps) != 0:
                raise SystemExit(f"--sim-fps {args.sim_fps}: not a multiple of the config's sim.fps {base.fps}")
            ratio = args.sim_fps // int(base.fps)
            ov["simulator.config.sim.fps"] = args.sim_fps
            ov["simulator.config.sim.control_decimation"] = int(base.control_decimation) * ratio
            print(f"# sim.fps {base.fps} -> {args.sim_fps}, control_decimation {base.control_decimation} -> {int(base.control_decimation) * ratio} "
                  "(the control step stays what it was)")
    else:
        ov["simulator._target_"] = "pbhc_amd.simulator.replay_stub.ReplaySimStub"
    cfg = load_config(args.config, ov, now="closed_loop")
    torch.manual_seed(args.seed)
    env = LeggedRobotMotionTracking(cfg.env.config, args.device)
    algo = MHPPO(env=env, config=cfg.algo.config, log_dir=None, device=args.device)
    algo.setup()
    return cfg, env, algo


# the corners of the footprint of the G1's foot collision capsules (x from -0.054 to 0.132, y +-0.026, 0.025 + the 0.01 radius below the
# ankle-roll link's origin), in that link's frame
G1_SOLE = [[0.132, 0.026, -0.035], [0.132, -0.026, -0.035], [-0.054, 0.026, -0.035], [-0.054, -0.026, -0.035]]


def ended_by(log):
    parts = [float(log[k]) for k in ("terminate_by_gravity", "terminate_by_motion_far", "terminate_by_time_out", "terminate_by_motion_end")]
    total = sum(parts)
    return "-" if total <= 0 else "/".join(f"{p / total:.2f}" for p in parts)


def tracking_figures(env):
    log = env.read_log()
    keep = env.reset_buf == 0
    qref = env._motion_lib.get_motion_state(env.motion_ids, env._ref_time, offset=env.env_origins)["dof_pos"]
    err = ((qref - env.simulator.dof_pos) ** 2).mean(dim=1)
    r = torch.exp(-err / float(log["adp_sigma_teleop_joint_pos"]))
    r = float(r[keep].mean()) if bool(keep.any()) else float("nan")
    return float(log["joint_pos_diff_norm"]), r, float(log["average_episode_length"]), ended_by(log)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default=os.path.join(ROOT, "tests", "golden", "configs", "v1_g1_23dof_walk.yaml"))
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--sim", choices=("joint", "articulated", "floating", "replay"), default="joint")
    ap.add_argument("--inertia", default="subtree", help='"subtree" or one number (kg m^2) for every joint')
    ap.add_argument("--armature", type=float, default=0.02)
    ap.add_argument("--damping", type=float, default=0.05)
    ap.add_argument("--mjcf", default="mjcf/g1_23dof_lock_wrist_fitmotionONLY.xml", help="robot.motion.asset.assetFileName for --sim joint ('' keeps the config's)")
    ap.add_argument("--stiffness", type=float, default=10000.0, help="--sim floating: N/m per contact point")
    ap.add_argument("--normal-damping", type=float, default=100.0, help="--sim floating: N s/m per contact point")
    ap.add_argument("--friction", type=float, default=0.8)
    ap.add_argument("--slip-velocity", type=float, default=None, help="--sim floating: m/s below which the friction is linear (default 0.4; 0.6 with --randomize)")
    ap.add_argument("--randomize", action="store_true", help="--sim floating: per-env link masses, torso centre of mass and friction (floating_sim.domain_rand)")
    ap.add_argument("--push", action="store_true", help="--sim floating: push_robots as the config has it (floating_sim.domain_rand.push)")
    ap.add_argument("--sim-fps", type=int, default=0, help="--sim floating: raise sim.fps to this multiple of the config's, and the decimation with it")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--print-every", type=int, default=1)
    args = ap.parse_args()

    if (args.randomize or args.push) and args.sim != "floating":
        raise SystemExit("--randomize and --push belong to --sim floating")
    cfg, env, algo = build(args)
    algo._train_mode()
    obs = env.reset_all()
    if args.sim == "replay":
        import bench

        env.simulator.set_replay(*bench.make_replay_on_device(env, algo.num_steps_per_env * 8 + 3, seed=99))
    elif args.sim == "joint":
        print("# inertia (kg m^2): " + " ".join(f"{v:.4f}" for v in env.simulator.inertia))
    print(f"# sim {args.sim}, {args.envs} envs, {algo.num_steps_per_env} steps per rollout, {args.iters} iterations")
    print("# iter joint_diff r_joint_pos avg_ep_len rollout_ms graph" + (" ended_by(gravity/motion_far/time_out/motion_end)" if args.sim == "floating" else ""))
    times, first, last = [], None, None
    for it in range(args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        algo.storage.clear()
        e0.record()
        obs = algo._rollout_step(obs)
        e1.record()
        algo._training_step()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        jd, rj, epl, ended = tracking_figures(env)
        if it >= 2:
            times.append(ms)
        first = (jd, rj) if first is None else first
        last = (jd, rj)
        if it % args.print_every == 0 or it == args.iters - 1:
            print(f"{it:5d} {jd:.5f} {rj:.5f} {epl:8.2f} {ms:8.3f} {int(bool(getattr(algo, '_rollout_used_graph', False)))}"
                  + (f" {ended}" if args.sim == "floating" else ""), flush=True)
    if times:
        print(f"# rollout_ms median {statistics.median(times):.3f} min {min(times):.3f} max {max(times):.3f} over {len(times)} iterations")
    print(f"# joint_diff {first[0]:.5f} -> {last[0]:.5f}   r_joint_pos {first[1]:.5f} -> {last[1]:.5f}")


if __name__ == "__main__":
    main()
