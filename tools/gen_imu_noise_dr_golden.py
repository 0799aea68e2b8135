"""Reference traces of obs.noise_process (the Ornstein-Uhlenbeck IMU noise) and domain_rand.parallel_serial_pd / parallel_serial_tau (build
machine only: it runs the unmodified reference on CPU through oracle/ref_harness).

  tests/golden/env_v1_walk_imunoise.npz        v1, walk clip, 16 envs x 5 steps: the OU process (scale.rpy / scale.base_ang_vel large enough
                                               that the noisy rows differ visibly from the clean ones), parallel_serial_pd with
                                               randomize_pd_gain, parallel_serial_tau with use_rao; actor_obs names base_ang_vel_noise and
                                               projected_gravity_noise.  The scripted replay terminates envs inside the window, so the
                                               stationary redraw and the compounding of the scales are exercised.
  tests/golden/env_v2_student23_imunoise.npz   v2 student23, 16 envs x 5 steps: the OU process, the four *_noise names in actor_obs.

The draws are recorded without touching the reference's arithmetic: noise_process.step / reset_part, _episodic_domain_randomization and
_compute_torques are wrapped at run time to save the global generator's state, draw what the method is about to draw (same shapes, same
order) and restore the state.  Per step [T, N, ...], rows of envs that did not draw are zero:
  step__ou_step [N,6]        the OU step's normals (every env)          step__ou_reset [N,6]   the stationary redraw's normals (reset envs)
  step__dr_kp / dr_kd / dr_rfi_lim / dr_rao [N,D]   the episodic draws as values (randomize_pd_gain, randomize_rfi_lim, use_rao)
  step__ps_kp / ps_kd [N,J]  parallel_serial_pd's U(ratio) factors      step__ps_rao [N,J]     parallel_serial_tau's episodic normals
  step__ps_tau [N,J]         parallel_serial_tau's torque normals of the control step's last physics sub-step (as step__u_rfi)
  state0__ou_state / step__state__ou_state [N,6]    env.noise_process.x before the trace / after each step
The per-step intermediates and reference bodies of the older traces (step__x__*, step__ref_body_*) are not written.

    PYTHONPATH=<repo> python tools/gen_imu_noise_dr_golden.py [v1] [v2]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_harness import gen_env_golden as G1      # noqa: E402
from oracle.ref_harness import gen_env_v2_golden as G2   # noqa: E402

OU = {"enable": True, "type": "ou", "kwargs": {"mu": 0.05, "sigma": 0.6, "theta": 0.8}, "scale": {"rpy": 5.0, "base_ang_vel": 0.5}}
PS_PD = {"enable": True, "ratio": [0.8, 1.2], "joint_idx": [4, 5, 10, 11, 13, 14]}
PS_TAU = {"enable": True, "joint_idx": [4, 5, 10, 11], "rao_lim": 0.02, "rfi_lim": 0.05}
NOISE_SCALES = {"base_ang_vel_noise": 0.25, "projected_gravity_noise": 1.0, "dof_pos_noise": 1.0, "dof_vel_noise": 0.05}


def configure(cfg, names, dr):
    """the switches and the *_noise observation names on a resolved config tree (the GPU tests apply the same as load_config overrides:
    tests/test_gpu_imu_noise_dr.py)"""
    from pbhc_amd.utils.config import _wrap

    D = len(cfg.robot.dof_names)
    cfg.obs.noise_process = _wrap(OU)
    cfg.obs.obs_dict.actor_obs = list(cfg.obs.obs_dict.actor_obs) + names
    dims = {"base_ang_vel_noise": 3, "projected_gravity_noise": 3, "dof_pos_noise": D, "dof_vel_noise": D}
    cfg.obs.obs_dims = list(cfg.obs.obs_dims) + [_wrap({n: dims[n]}) for n in names]
    for n in names:
        cfg.obs.obs_scales[n] = NOISE_SCALES[n]
        cfg.obs.noise_scales[n] = 0.0
    if dr:
        cfg.domain_rand.parallel_serial_pd = _wrap(PS_PD)
        cfg.domain_rand.parallel_serial_tau = _wrap(PS_TAU)


class _Recorder:
    """Wraps the reference env's random draws of the three switches; `begin_step()` starts a fresh [N, ...] record per step."""

    def __init__(self, env):
        self.env, self.cur = env, None
        N, D = env.num_envs, env.num_dof
        dr = env.config.domain_rand
        self.pd = dr.parallel_serial_pd.joint_idx if "parallel_serial_pd" in dr and dr.parallel_serial_pd.enable else []
        self.tau = dr.parallel_serial_tau.joint_idx if "parallel_serial_tau" in dr and dr.parallel_serial_tau.enable else []
        self.shapes = {"ou_step": (N, 6), "ou_reset": (N, 6), "dr_kp": (N, D), "dr_kd": (N, D), "dr_rfi_lim": (N, D), "dr_rao": (N, D),
                       "ps_kp": (N, max(len(self.pd), 1)), "ps_kd": (N, max(len(self.pd), 1)), "ps_rao": (N, max(len(self.tau), 1)),
                       "ps_tau": (N, max(len(self.tau), 1)), "state__ou_state": (N, 6)}
        self.steps = {k: [] for k in self.shapes}
        self.x0 = env.noise_process.x.clone()
        np_, oe, oc = env.noise_process, env._episodic_domain_randomization, env._compute_torques
        ostep, oreset = np_.step, np_.reset_part

        def peek(fn):
            s = torch.get_rng_state()
            try:
                return fn()
            finally:
                torch.set_rng_state(s)

        def step():
            if self.cur is not None:
                self.cur["ou_step"][:] = peek(lambda: torch.randn(*np_.shape))
            return ostep()

        def reset_part(mask):
            if self.cur is not None:
                z = peek(lambda: torch.randn(int(torch.sum(mask))))
                self.cur["ou_reset"][mask] = z
            return oreset(mask)

        def episodic(env_ids):
            if self.cur is not None and len(env_ids) > 0:
                n, c = len(env_ids), env.config.domain_rand
                u = lambda lo, hi, m: (hi - lo) * torch.rand(n, m) + lo

                def draw():
                    d = {}
                    if c.randomize_pd_gain:
                        d["dr_kp"], d["dr_kd"] = u(c.kp_range[0], c.kp_range[1], D), u(c.kd_range[0], c.kd_range[1], D)
                    if self.pd:
                        r = c.parallel_serial_pd.ratio
                        d["ps_kp"], d["ps_kd"] = u(r[0], r[1], len(self.pd)), u(r[0], r[1], len(self.pd))
                    if c.randomize_rfi_lim:
                        d["dr_rfi_lim"] = u(c.rfi_lim_range[0], c.rfi_lim_range[1], D)
                    if c.use_rao:
                        d["dr_rao"] = u(-c.rao_lim, c.rao_lim, D)
                    if self.tau:
                        d["ps_rao"] = torch.randn(n, len(self.tau))
                    return d

                for k, v in peek(draw).items():
                    self.cur[k][env_ids] = v
            return oe(env_ids)

        def compute_torques(a):
            if self.cur is not None and self.tau:
                def draw():
                    if env.config.domain_rand.randomize_torque_rfi:
                        torch.rand(N, D)
                    return torch.randn(N, len(self.tau))
                self.cur["ps_tau"][:] = peek(draw)              # every sub-step overwrites: the last one's is what the trace keeps
            return oc(a)

        np_.step, np_.reset_part = step, reset_part
        env._episodic_domain_randomization, env._compute_torques = episodic, compute_torques

    def begin_step(self):
        self.cur = {k: torch.zeros(*s) for k, s in self.shapes.items()}
        for k in self.steps:
            self.steps[k].append(self.cur[k])

    def end_step(self):
        self.cur["state__ou_state"][:] = self.env.noise_process.x


def _run(module, run, names, dr):
    """run the module's run_trace with build_env / env.step / save substituted at run time; returns the saved file name"""
    rec = {}
    orig_build = module.build_env

    def build_env(cfg, seed=0):
        configure(cfg, names, dr)
        env = orig_build(cfg, seed)
        ostep = env.step

        def step(actor_state):
            if "r" in rec:
                rec["r"].begin_step()
            out = ostep(actor_state)
            if "r" in rec:
                rec["r"].end_step()
            return out

        env.step = step
        orig_reset_all = env.reset_all

        def reset_all():
            out = orig_reset_all()
            rec["r"] = _Recorder(env)           # after reset_all: the trace's steps only (and the OU state they start from)
            return out

        env.reset_all = reset_all
        return env

    module.build_env = build_env
    saved = {}
    orig_save = G1.G.save

    def save(name, **arrs):
        arrs = {k: v for k, v in arrs.items() if not k.startswith(("step__x__", "step__ref_body_"))}
        r = rec["r"]
        T = arrs["actions_in"].shape[0]
        for k, v in r.steps.items():
            arrs["step__" + k] = np.stack([t.numpy() for t in v[-T:]]).astype(np.float32)
        arrs["state0__ou_state"] = r.x0.numpy().astype(np.float32)
        name = name.replace(".npz", "") + ".npz"
        saved["name"] = name
        return orig_save(name, **arrs)

    G1.G.save = save
    try:
        run()
    finally:
        module.build_env, G1.G.save = orig_build, orig_save
    return saved["name"]


def _report(name):
    g = np.load(os.path.join(G1.G.GOLD, name))
    print(name, "resets per step:", g["step__reset_buf_out"].sum(1))
    assert g["step__reset_buf_out"].sum() > 0 and np.abs(g["step__ou_reset"]).sum() > 0, "the window holds no reset"


def v1():
    name = _run(G1, lambda: G1.run_trace(G1.V1_CFG, "walk_imunoise", N=16, T=5, motion_file="motion_data/g1_walk_45cms_23dof.pkl",
                                         extra=G1.WALK_EXTRA, seed=41), ["base_ang_vel_noise", "projected_gravity_noise"], dr=True)
    _report(name)


def v2():
    def run():
        cwd = os.getcwd()
        try:
            G2.run_trace("student23", "student23_imunoise", N=16, T=5, seed=42)
        finally:
            os.chdir(cwd)

    name = _run(G2, run, ["base_ang_vel_noise", "projected_gravity_noise", "dof_pos_noise", "dof_vel_noise"], dr=False)
    _report(name)


if __name__ == "__main__":
    which = sys.argv[1:] or ["v1", "v2"]
    if "v1" in which:
        v1()
    if "v2" in which:
        v2()
