"""Reference traces of the two reset options (build machine only: it runs the unmodified reference on CPU through oracle/ref_harness).

  tests/golden/env_v1_walk_doffar.npz   v1, walk clip, 16 envs x 5 steps: termination.terminate_when_dof_far with its curriculum (a degree
                                        that moves the threshold) and noise_to_initial_level = 1 (motion_tracking.py:128-130,283-306,343-349,
                                        470-545).  The default scripted replay bends env 6's knee to 3.1 rad on steps 1-4, which would fire
                                        the batch-global test on every one of them: here it stays bent on step 2 only, so dof-far fires on
                                        exactly one step (and resets all 16 envs, with noise).
  tests/golden/env_v2_student23_resetnoise.npz   v2 student23, 16 envs x 5 steps, noise_to_initial_level = 1 (general_tracking.py:405-485:
                                        the dof offsets are rand_like, one-sided).

The reset-noise draws are recorded without touching the reference's arithmetic: the env's _reset_dofs / _reset_root_states are wrapped at
run time to reseed the global generator, draw what the method is about to draw (same shapes, same order), and reseed again — the way
gen_env_golden.py records the torque-noise uniforms.  The draws land in step__reset_root [T,N,13] (randn pos 3, randn axis 3, rand angle 1,
randn lin vel 3, randn ang vel 3), step__reset_dof_pos / step__reset_dof_vel [T,N,D]; rows of envs that did not reset are zero.  The per-step
intermediates and reference bodies the older traces carry (step__x__*, step__ref_body_*) are not written: no test of these switches reads them.

    PYTHONPATH=<repo> python tools/gen_reset_options_golden.py [v1] [v2]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_harness import gen_env_golden as G1      # noqa: E402
from oracle.ref_harness import gen_env_v2_golden as G2   # noqa: E402

_TC = "env.config.termination_curriculum.terminate_when_dof_far_curriculum."
DOF_FAR = {"env.config.termination.terminate_when_dof_far": True, _TC + "enable": True, _TC + "init": 2.0, _TC + "degree": 0.05,
           _TC + "min": 1.0, _TC + "max": 2.5, _TC + "level_down_threshold": 40, _TC + "level_up_threshold": 42}
NOISE = {"env.config.noise_to_initial_level": 1.0}
_MAKE_REPLAY = G1.make_replay


class _Recorder:
    """Wraps an env's _reset_dofs / _reset_root_states; `begin_step()` starts a fresh [N, ...] record (zeros for envs that do not reset)."""

    def __init__(self, env, uniform_dofs):
        self.env, self.n = env, 0
        self.active = False
        self.draw_dof = torch.rand if uniform_dofs else torch.randn
        self.steps = {"reset_root": [], "reset_dof_pos": [], "reset_dof_vel": []}
        od, orr = env._reset_dofs, env._reset_root_states

        def reset_dofs(env_ids, *a, **k):
            if self.active:
                s = self._seed()
                n, D = len(env_ids), env.num_dof
                p, v = self.draw_dof(n, D), self.draw_dof(n, D)
                torch.manual_seed(s)
                self.cur["reset_dof_pos"][env_ids] = p
                self.cur["reset_dof_vel"][env_ids] = v
            return od(env_ids, *a, **k)

        def reset_root(env_ids, *a, **k):
            if self.active:
                s = self._seed()
                n = len(env_ids)
                z = torch.cat([torch.randn(n, 3), torch.randn(n, 3), torch.rand(n, 1), torch.randn(n, 3), torch.randn(n, 3)], dim=1)
                torch.manual_seed(s)
                self.cur["reset_root"][env_ids] = z
            return orr(env_ids, *a, **k)

        env._reset_dofs, env._reset_root_states = reset_dofs, reset_root

    def _seed(self):
        s = 5000 + self.n
        self.n += 1
        torch.manual_seed(s)
        return s

    def begin_step(self):
        N, D = self.env.num_envs, self.env.num_dof
        self.active = True
        self.cur = {"reset_root": torch.zeros(N, 13), "reset_dof_pos": torch.zeros(N, D), "reset_dof_vel": torch.zeros(N, D)}
        for k in self.steps:
            self.steps[k].append(self.cur[k])


def _run(module, run, uniform_dofs, replay_fn=None):
    """run the module's run_trace with build_env / make_replay / env.step substituted at run time; returns (recorder, saved file name)"""
    rec = {}
    orig_build, orig_replay = module.build_env, G1.make_replay

    def build_env(cfg, seed=0):
        env = orig_build(cfg, seed)
        r = _Recorder(env, uniform_dofs)
        rec["r"] = r
        ostep = env.step

        def step(actor_state):
            r.begin_step()
            return ostep(actor_state)

        env.step = step
        return env

    module.build_env = build_env
    if replay_fn is not None:
        G1.make_replay = replay_fn
    saved = {}
    orig_save = G1.G.save

    def save(name, **arrs):
        # the per-step intermediates (step__x__*) and reference bodies are diagnostics of the older traces that no test of these switches
        # reads: left out to keep the fixtures small
        arrs = {k: v for k, v in arrs.items() if not k.startswith(("step__x__", "step__ref_body_"))}
        T = arrs["actions_in"].shape[0]
        for k, v in rec["r"].steps.items():            # (the first record is reset_all's own step, before the trace)
            arrs["step__" + k] = np.stack([t.numpy() for t in v[-T:]]).astype(np.float32)
        saved["name"] = name
        return orig_save(name, **arrs)

    G1.G.save = save
    try:
        run()
    finally:
        module.build_env, G1.make_replay, G1.G.save = orig_build, orig_replay, orig_save
    return saved["name"]


def _one_bend_replay(env, ml, T, seed, script=True):
    """the default scripted replay with env 6's bent knee / ankle kept on step 2 only (dof-far fires on exactly one step)"""
    root, qp, qv, cf = _MAKE_REPLAY(env, ml, T, seed, script=script)
    _, qp0, _, _ = _MAKE_REPLAY(env, ml, T, seed, script=False)
    for k in range(T):
        if k != 2:
            qp[k, 6, 3], qp[k, 6, 5] = qp0[k, 6, 3], qp0[k, 6, 5]
    return root, qp, qv, cf


def v1():
    name = _run(G1, lambda: G1.run_trace(G1.V1_CFG, "walk_doffar", N=16, T=5, motion_file="motion_data/g1_walk_45cms_23dof.pkl",
                                         extra=dict(G1.WALK_EXTRA, **DOF_FAR, **NOISE), seed=31), uniform_dofs=False, replay_fn=_one_bend_replay)
    g = np.load(os.path.join(G1.G.GOLD, name))
    fired = g["step__log__terminate_by_dof_far"]
    print(name, "terminate_by_dof_far per step:", fired, "threshold:", g["step__log__terminate_when_dof_far_threshold"])
    assert (fired > 0).sum() == 1, "dof-far must fire on exactly one step"


def v2():
    def run():
        cwd = os.getcwd()
        try:
            G2.run_trace("student23", "student23_resetnoise", N=16, T=5, extra=NOISE, seed=32)
        finally:
            os.chdir(cwd)

    name = _run(G2, run, uniform_dofs=True)
    g = np.load(os.path.join(G1.G.GOLD, name))
    print(name, "resets per step:", g["step__reset_buf_out"].sum(1))


if __name__ == "__main__":
    which = sys.argv[1:] or ["v1", "v2"]
    if "v1" in which:
        v1()
    if "v2" in which:
        v2()
