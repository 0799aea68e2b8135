"""Reference trace of the evaluation recorder (build machine only: it runs the unmodified reference on CPU through oracle/ref_harness).

  tests/golden/env_v1_walk_record.npz   v1, walk clip, 16 envs, save_motion on with save_total_steps = 8 (opt/record.yaml's keys) and
                                        _write_to_file off (motion_tracking.py:140-170, 861-938).

The reference records every control step — the one inside reset_all() included, which run_trace calls before the trace — drops its first
three records and builds `saved_motion_dict` at the START of the step that finds save_total_steps + 3 records in its lists.  With
reset_all's record that is trace step 10 (0-based), and the dict holds trace steps 2..9; the trace runs 12 steps, so the last one also shows
that later steps leave the dict alone.  It is stored under `saved__<key>` next to the usual replay inputs (actions, replay frames, the
per-step draws and states of gen_env_golden.run_trace).  The default scripted replay already resets an env inside the recorded window (env 3
tips over from step 2 on and is reset in every step); on top of it env 11's root quaternion is negated from step 4 on — the same rotation
with w < 0 — so that the rotation vector's sign branch is exercised.  The per-step intermediates and reference bodies of the older traces
(step__x__*, step__ref_body_*) are not written.

The recorder keeps `tensor.cpu()` of live env buffers in its lists.  On the device the reference runs on that is a copy — a snapshot of the
step; on this CPU harness `.cpu()` would return the live tensor itself and every list entry would end up showing the last step.  While the
trace runs, torch.Tensor.cpu therefore returns a clone (a run-time substitution in the harness, like the wrappers of the other generators;
the reference's files are not touched).  main() checks the result: `terminate` and `dof` of the dict are the per-step values of the trace.

    PYTHONPATH=<repo> python tools/gen_record_golden.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_harness import gen_env_golden as G1      # noqa: E402

SAVE_TOTAL_STEPS = 8
KEYS = ("root_trans_offset", "pose_aa", "dof", "root_rot", "actor_obs", "action", "terminate", "root_lin_vel", "root_ang_vel", "dof_vel",
        "contact_mask", "motion_times")
_MAKE_REPLAY = G1.make_replay


def _negated_quat_replay(env, ml, T, seed, script=True):
    root, qp, qv, cf = _MAKE_REPLAY(env, ml, T, seed, script=script)
    root[4:, 11, 3:7] *= -1.0
    return root, qp, qv, cf


def main():
    ckpt = tempfile.mkdtemp(prefix="record_golden_")
    record = {"env.config.save_motion": True, "env.config.save_total_steps": SAVE_TOTAL_STEPS, "env.config.save_note": "golden",
              "env.config.eval_timestamp": "golden", "env.config.ckpt_dir": ckpt}
    held = {}
    orig_build, orig_replay, orig_save = G1.build_env, G1.make_replay, G1.G.save

    def build_env(cfg, seed=0):
        env = orig_build(cfg, seed)
        assert env.save_motion
        env._write_to_file = False
        held["env"] = env
        return env

    def save(name, **arrs):
        env = held["env"]
        arrs = {k: v for k, v in arrs.items() if not k.startswith(("step__x__", "step__ref_body_"))}
        for k in KEYS:
            arrs["saved__" + k] = np.asarray(env.saved_motion_dict[k])
        arrs["save_total_steps"] = np.int64(SAVE_TOTAL_STEPS)
        arrs["motion_episode_length"] = np.int64(int(env._motion_episode_length))
        return orig_save(name, **arrs)

    G1.build_env, G1.make_replay, G1.G.save = build_env, _negated_quat_replay, save
    orig_cpu = torch.Tensor.cpu
    torch.Tensor.cpu = lambda self, *a, **k: orig_cpu(self, *a, **k).clone()          # device -> host copy semantics (see above)
    try:
        G1.run_trace(G1.V1_CFG, "walk_record", N=16, T=SAVE_TOTAL_STEPS + 4, motion_file="motion_data/g1_walk_45cms_23dof.pkl",
                     extra=dict(G1.WALK_EXTRA, **record), seed=41)
    finally:
        G1.build_env, G1.make_replay, G1.G.save = orig_build, orig_replay, orig_save
        torch.Tensor.cpu = orig_cpu
    g = np.load(os.path.join(G1.G.GOLD, "env_v1_walk_record.npz"))
    term, rot = g["saved__terminate"], g["saved__root_rot"]
    print("resets inside the recorded window per env:", term.sum(1))
    print("root quaternions with w < 0 in the window:", int((rot[..., 3] < 0).sum()))
    assert term.sum() > 0 and (rot[..., 3] < 0).any()
    T = SAVE_TOTAL_STEPS
    assert np.array_equal(term, g["step__reset_buf_out"][2:2 + T].T), "terminate is not the per-step reset_buf of trace steps 2..9"
    assert np.array_equal(g["saved__dof"], g["step__state__dof_pos"][2:2 + T].transpose(1, 0, 2)), "dof is not the per-step state"
    for k in KEYS:
        print(k, g["saved__" + k].shape, g["saved__" + k].dtype)


if __name__ == "__main__":
    main()
