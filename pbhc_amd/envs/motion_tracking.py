"""LeggedRobotMotionTracking — drop-in for the reference's KungfuBot (v1) env, running the whole
`step()` as one fused HIP launch.

Same constructor, methods, attributes and return values as the reference class
(reference: humanoidverse/envs/motion_tracking/motion_tracking.py:97-135 on top of
legged_robot_base.py:29-37,239-265 and base_task.py:19-93), selected the same way:
`env._target_: pbhc_amd.envs.motion_tracking.LeggedRobotMotionTracking`.
`step(actor_state)` returns `(obs_dict, rew_buf, reset_buf, extras)` with env-owned tensors that
are overwritten by the next step, as in the reference.  There is no eager / CPU path: every step
goes through `pbhc_env_step`; construction fails if libpbhc_hip.so is missing.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import importlib
import os
import sys
from collections.abc import Mapping

import numpy as np
import torch

from .. import _lib
from .. import dist as pdist
from ..motion_lib import MotionLib
from ..utils import resume, rng_state
from . import env_config

K = _lib.K


class EpisodeExtras(Mapping):
    """`extras["episode"]` of a step (legged_robot_base.py:510-515): `rew_<term>` = the finished episodes' reward sums / max_episode_length_s
    and `end_epis_length`, one entry per env reset in that step.  Their shape depends on how many envs reset, which the reference learns with
    a host synchronisation every step (`nonzero`); here the kernel leaves the per-env values on the device and this mapping gathers them on
    first access.  It reads env-owned buffers of ITS step: `env.step()` materialises a mapping somebody still holds before it launches the
    next step, so a consumer may keep it (the reference's agents append it to `ep_infos` and read it at logging time)."""

    def __init__(self, env):
        self._env, self._data = env, None

    def materialise(self):
        if self._data is None:
            e = self._env
            ids = e.reset_buf.nonzero(as_tuple=False).flatten()
            d = {"rew_" + k: e._episode_rew_out[ids, i] for i, k in enumerate(e.layout.sum_names)}
            d["end_epis_length"] = e.last_episode_length_buf[ids]
            self._data, self._env = d, None
        return self._data

    def __getitem__(self, k):
        return self.materialise()[k]

    def __iter__(self):
        return iter(self.materialise())

    def __len__(self):
        return len(self.materialise())


class StepExtras(dict):
    """The env's `extras` mapping (one object, refilled every step, like the reference's `self.extras`).  `ref_body_pos_extend` /
    `ref_body_rot_extend` — the reference motion's extended body poses of the last step (motion_tracking.py:645-650) — are read by
    evaluation callbacks only, so the fused step does not store them: the kernel leaves the motion time of its lookup (4 B per env instead
    of 756) and the two tensors are rebuilt by the same lerp / slerp (pbhc_motion_state) when one of them is read — valid until the next
    `step()`, exactly as long as the reference's env-owned tensors are."""
    LAZY = {"ref_body_pos_extend": 0, "ref_body_rot_extend": 1}

    def __init__(self, env):
        super().__init__()
        self._env = env

    def _fill(self):
        pos, rot = self._env._reference_bodies()
        dict.__setitem__(self, "ref_body_pos_extend", pos)
        dict.__setitem__(self, "ref_body_rot_extend", rot)

    def invalidate(self):
        for k in self.LAZY:
            dict.__setitem__(self, k, None)

    def __getitem__(self, k):
        if k in self.LAZY and dict.get(self, k) is None:
            self._fill()
        return dict.__getitem__(self, k)

    def get(self, k, default=None):
        return self[k] if k in self else default

    def __iter__(self):
        # (an overridden __iter__ takes `dict(extras)` / `{**extras}` / `other.update(extras)` off CPython's storage-level fast path: they
        # then read through keys() + __getitem__, i.e. they see the lazy members materialised, not None)
        return iter(list(dict.keys(self)))

    def __reduce__(self):
        self._fill()
        return (dict, (dict(dict.items(self)),))

    def items(self):
        self._fill()
        return dict.items(self)

    def values(self):
        self._fill()
        return dict.values(self)

    def copy(self):
        self._fill()
        return dict(self)


class ReinitSchedule:
    """domain_rand.reinit_epis_rand > 0: the episodic domain randomisation of EVERY env is re-drawn at exponentially distributed intervals
    (legged_robot_base.py:142,390-395): the counter starts at 0 — the first re-draw fires in the very first step — and every firing draws
    the next interval with ONE np.random.rand.  Host logic only (tests/test_reinit_schedule.py replays the reference's lines)."""

    def __init__(self, mean_interval):
        self.mean = float(mean_interval)
        self.counter = 0.0 if self.mean > 0 else float("inf")

    def due(self, common_step_counter):
        """`common_step_counter`: the value AFTER this step's increment (the reference tests it in `_update_tasks_callback`, behind
        `_update_counters_each_step`)."""
        if common_step_counter >= self.counter:
            self.counter = common_step_counter + float(-np.log(np.random.rand(1))[0] * self.mean)
            return True
        return False


def get_class(path):
    mod, name = path.rsplit(".", 1)
    return getattr(importlib.import_module(mod), name)


class LeggedRobotMotionTracking:
    TRACKING_MODE = 0          # selects the kernel instantiation (see PbhcEnvConfig.tracking_mode)
    _fin_deferred = _fin_owed = False            # set_finalize_deferred(): per instance once it is used

    def __init__(self, config, device):
        """config = cfg.env.config (with .robot/.obs/.rewards/.domain_rand/.terrain/.simulator aliased
        to the top-level nodes, as Hydra composes it)."""
        self.init_done = False
        self.config = config
        self._lib = _lib.lib()
        self._is_evaluating = False
        # ---- BaseTask.__init__ (base_task.py:20-64)
        self.simulator = get_class(config.simulator._target_)(config=config, device=device)
        self.headless = config.headless
        self.simulator.set_headless(self.headless)
        self.simulator.setup()
        self.device = torch.device(self.simulator.sim_device)
        self.sim_dt = self.simulator.sim_dt
        self.up_axis_idx = 2
        self.dt = config.simulator.config.sim.control_decimation * self.sim_dt
        self.max_episode_length_s = config.max_episode_length_s
        self.max_episode_length = np.ceil(self.max_episode_length_s / self.dt)
        self.num_envs = N = config.num_envs
        self.dim_actions = config.robot.actions_dim
        self.simulator.setup_terrain(config.terrain.mesh_type)
        self.num_dof, self.num_bodies, self.dof_names, self.body_names = self.simulator.load_assets()
        assert self.num_dof == self.dim_actions, "Number of DOFs must be equal to number of actions"
        self.num_dofs = self.num_dof
        dev = self.device
        rc = config.robot
        base = list(rc.init_state.pos) + list(rc.init_state.rot) + list(rc.init_state.lin_vel) + list(rc.init_state.ang_vel)
        self.base_init_state = torch.tensor(base, dtype=torch.float, device=dev)
        self._get_env_origins()
        self.simulator.create_envs(N, self.env_origins, self.base_init_state)
        self.dof_pos_limits, self.dof_vel_limits, self.torque_limits = self.simulator.get_dof_limits_properties()
        self.simulator.prepare_sim()
        self.viewer = None
        # ---- motion library (motion_tracking.py:171-199)
        self.skeleton = self.simulator.skeleton
        rc.motion.step_dt = self.dt
        self.max_len = int(getattr(rc.motion, "motion_max_len", -1)) if self.TRACKING_MODE == 1 else -1     # general_tracking.py:60
        self._motion_lib = MotionLib.from_config(rc.motion, self.skeleton, N, dev, max_len=self.max_len, robot=rc)
        # host-side draws (slot -> clip sampling, start phases and episodic DR of reset_all): the torch global generator on rank 0 — as the
        # reference — and a rank-keyed generator on the other ranks of a data-parallel run, so that equal seeds do not replicate envs
        self._gen = pdist.host_generator(dev)
        self._motion_lib.generator = self._gen
        if self._gen is not None:
            import random

            self._motion_lib.pyrand = random.Random(self._gen.initial_seed())
        self._load_motions_initial()
        for e in rc.motion.get("extend_config", []):
            self.simulator._body_list.append(e["joint_name"])           # motion_tracking.py:226
        self.num_extend_bodies = len(rc.motion.get("extend_config", []))
        # ---- static config -> device
        # Philox key of this env shard: the torch-seeded draw, with the rank mixed in (same config.seed on every rank must not replicate streams)
        self._seed = pdist.rank_seed(int(torch.randint(0, 2**31 - 1, (1,)).item()), bits=31)
        self._c, self.layout = env_config.build(_TopView(config), self.skeleton, self._motion_lib, N, dev, self.simulator._link_mass_scale.shape[1],
                                                seed=self._seed, mode=self.TRACKING_MODE)
        L = self.layout
        self.reward_names = L.reward_names
        self.reward_scales = L.reward_scales
        self.feet_indices = torch.tensor(L.feet, dtype=torch.long, device=dev)
        self.penalised_contact_indices = torch.tensor(L.penalised, dtype=torch.long, device=dev)
        self.motion_tracking_id, self.lower_body_id, self.upper_body_id = L.track, L.lower, L.upper
        self.globals = torch.tensor(L.globals0, dtype=torch.float64, device=dev)
        # reference yaw of env 0 at t = dt (motion_tracking.py:186-187); host-side, once
        ref0 = self._motion_lib.get_motion_state(torch.zeros(1, dtype=torch.long, device=dev), torch.full((1,), self.dt, device=dev), offset=self.env_origins[:1])
        q = ref0["root_rot"][0].tolist()
        self.ref_init_yaw = float(np.arctan2(2.0 * (q[3] * q[2] + q[0] * q[1]), q[3] * q[3] + q[0] * q[0] - q[1] * q[1] - q[2] * q[2]))
        self._c.ref_init_yaw = self.ref_init_yaw
        self._env = C.c_void_p()
        _lib.check(self._lib.pbhc_env_create(C.byref(self._c), C.byref(self._motion_lib.table), self.globals.data_ptr(), C.byref(self._env)), "pbhc_env_create")
        # the step kernel specialised to this config (a ~3 s hipcc build on the first env of a config, cached in pbhc_amd/_spec):
        # PBHC_SPECIALISE=off keeps the generic kernel, =cached never compiles
        self.specialise(os.environ.get("PBHC_SPECIALISE", "jit"))
        self._totals, self._stat_pending, self._stat_group, self._num_envs_total = None, None, None, float(N)     # enable_global_statistics()
        self._finalize_stream, self._step_done, self._fin_done, self._fin_pending = None, None, None, False        # set_finalize_stream()
        self._init_start_sampling()                 # before _build_io: the step's io names the start-time buffer
        self._init_buffers()
        self._init_obs_buffers()
        self._build_io()
        self.log_dict = {}
        self.extras = StepExtras(self)
        self.common_step_counter = 0
        self._resample_motion_times(torch.arange(N, device=dev))
        if config.get("resample_motion_when_training", False):
            self.resample_time_interval = np.ceil(config.resample_time_interval_s / self.dt)
        # domain_rand.reinit_epis_rand > 0: the episodic DR of EVERY env is re-drawn at exponentially distributed intervals
        # (legged_robot_base.py:149-151,390-395)
        self.reinit_epis_rand = float(config.domain_rand.get("reinit_epis_rand", -1))
        self._reinit = ReinitSchedule(self.reinit_epis_rand)
        if self._c.noise_process:                   # OUProcess.reset at construction (legged_robot_base.py:124-127): the stationary law
            self._ou_state.copy_(self._ou_stationary(N))
        self._init_save_motion()
        self._init_clip_statistics()
        if hasattr(self.simulator, "bind"):         # a simulator that writes its own frames (JointSpaceSim): its window, its kernel's parameters
            self.simulator.bind(self)
        self.init_done = True

    def specialise(self, mode="jit", verbose=False):
        """Run this env's steps on a build of k_env_step specialised to its config (pbhc_amd/specialise.py): "jit" compiles on a cache
        miss (~3 s of hipcc, once per config, source and compiler version), "cached" only uses an existing object, "off" returns to the generic
        kernel.  Same source, same results; returns True when a specialised kernel is attached."""
        from .. import specialise as _spec

        self._specialise_mode = mode
        self._io_epoch = getattr(self, "_io_epoch", 0) + 1         # a captured graph of steps names the kernel it was recorded with
        return _spec.attach(self._env, mode, verbose=verbose)

    @property
    def is_specialised(self):
        return bool(self._lib.pbhc_env_is_specialised(self._env))

    def _load_motions_initial(self):
        self._motion_lib.load_motions(random_sample=not self.is_evaluating)            # motion_tracking.py:176-180

    # ------------------------------------------------------------------------------------
    def __del__(self):
        try:
            if getattr(self, "_env", None):
                self._lib.pbhc_env_destroy(self._env)
                self._env = None
        except Exception:
            pass

    def _get_env_origins(self):
        # base_task.py:102-138, plane terrain branch
        N, dev = self.num_envs, self.device
        self.custom_origins = False
        self.env_origins = torch.zeros(N, 3, device=dev)
        num_cols = np.floor(np.sqrt(N))
        num_rows = np.ceil(N / num_cols)
        xx, yy = torch.meshgrid(torch.arange(num_rows), torch.arange(num_cols), indexing="ij")
        spacing = self.config.env_spacing
        self.env_origins[:, 0] = (spacing * xx.flatten()[:N]).to(dev)
        self.env_origins[:, 1] = (spacing * yy.flatten()[:N]).to(dev)

    def _init_buffers(self):
        N, D, dev, L = self.num_envs, self.num_dof, self.device, self.layout
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.actions, self.last_actions, self.actions_after_delay = f(N, D), f(N, D), f(N, D)
        self.action_queue = f(N, self._c.queue_len, D)
        dr = self.config.domain_rand
        if dr.randomize_ctrl_delay:
            self.action_delay_idx = torch.randint(dr.ctrl_delay_step_range[0], dr.ctrl_delay_step_range[1] + 1, (N,), device=dev, generator=self._gen)
        else:
            self.action_delay_idx = torch.zeros(N, dtype=torch.long, device=dev)
        self.last_dof_pos, self.last_dof_vel, self.torques = f(N, D), f(N, D), f(N, D)
        self.feet_air_time, self.contacts, self.contacts_filt = f(N, 2), f(N, 2), f(N, 2)
        self.last_contacts, self.last_contacts_filt = f(N, 2), f(N, 2)
        self._kp_scale, self._kd_scale = torch.ones(N, D, device=dev), torch.ones(N, D, device=dev)
        self._rfi_lim_scale, self._rao_scale = torch.ones(N, D, device=dev), torch.ones(N, D, device=dev)
        self.motion_start_times, self.motion_len, self.end_time_ratio_buf = f(N), f(N), f(N)
        self._episode_sums = f(N, len(L.sum_names))
        self.episode_sums = {name: self._episode_sums[:, i] for i, name in enumerate(L.sum_names)}
        self._episode_rew_out = f(N, len(L.sum_names))
        self._hist = _padded_rows(N, L.hist_dim, dev)            # rows start on 128-B lines
        self._episode_length_buf = torch.zeros(N, dtype=torch.long, device=dev)
        self.last_episode_length_buf = torch.zeros(N, dtype=torch.long, device=dev)
        self.reset_buf = torch.ones(N, dtype=torch.long, device=dev)
        self.time_out_buf = torch.zeros(N, dtype=torch.bool, device=dev)
        self.motion_ids = torch.arange(N, device=dev)
        self.rew_buf = f(N, L.num_rew_fn) if self.config.use_vec_reward else f(N)
        self._ref_time = f(N)                                # motion time of the last step's reference lookup (lazy reference bodies)
        self._ref_bodies = None
        self.default_dof_pos = torch.tensor([self._c.default_dof_pos[i] for i in range(D)], device=dev).repeat(N, 1)
        self.raw_default_dof_pos = self.default_dof_pos.clone()                    # legged_robot_base.py:81-93
        self.p_gains = torch.tensor([self._c.p_gains[i] for i in range(D)], device=dev)
        self.d_gains = torch.tensor([self._c.d_gains[i] for i in range(D)], device=dev)
        # obs.noise_process: the OU state [N, 6] (rpy, angular velocity), drawn from its stationary law at construction (noise_tool.py
        # OUProcess.reset); the step kernel reads and writes it in place, so a captured rollout graph carries it like any other state
        self._ou_state = f(N, 6)                    # (its construction-time draw: the end of __init__)

    def _init_obs_buffers(self):
        L = self.layout
        self._own_obs = {g: _padded_rows(self.num_envs, L.group_dims[g], self.device) for g in L.group_names[:-1]}
        self.obs_buf_dict = dict(self._own_obs)

    def rebuild_observations(self):
        """Re-derive the observation maps after `config.obs.obs_dict` changed (the reference re-reads the dict every step, so
        ppo_mimic's distillation adds the teacher's observation groups after the env exists, ppo_mimic.py:131-134).  State is kept;
        the set of history keys must not change."""
        old = self.layout
        self._flush_statistics()
        c, L = env_config.build(_TopView(self.config), self.skeleton, self._motion_lib, self.num_envs, self.device, self.simulator._link_mass_scale.shape[1],
                                seed=self._seed, mode=self.TRACKING_MODE)
        if (L.hist_keys, L.hist_len, L.hist_dim) != (old.hist_keys, old.hist_len, old.hist_dim) or L.sum_names != old.sum_names:
            raise _lib.PbhcError("rebuild_observations: history keys / reward terms changed")
        c.ref_init_yaw = self.ref_init_yaw
        env = C.c_void_p()
        _lib.check(self._lib.pbhc_env_create(C.byref(c), C.byref(self._motion_lib.table), self.globals.data_ptr(), C.byref(env)), "pbhc_env_create")
        self._lib.pbhc_env_destroy(self._env)
        self._env, self._c, self.layout = env, c, L
        if getattr(self, "_rec", None) is not None:
            if L.record["rows"] != old.record["rows"]:
                raise _lib.PbhcError("rebuild_observations: the recorded actor_obs row changed while env.config.save_motion is on")
            self._rec_io.obs_group = L.record["obs_group"]
        self._init_obs_buffers()
        self._build_io()
        if getattr(self, "_specialise_mode", None) not in (None, "off"):
            self.specialise(self._specialise_mode)                   # the new env object has a new config: its own specialised build

    @property
    def history(self):
        """per-key views [N, len, dim] of the packed history state (HistoryHandler.history)."""
        L = self.layout
        return {k: self._hist[:, L.hist_off[k]:L.hist_off[k] + L.hist_len[k] * L.obs_dims[k]].view(self.num_envs, L.hist_len[k], L.obs_dims[k]) for k in L.hist_keys}

    @property
    def episode_length_buf(self):
        return self._episode_length_buf

    @episode_length_buf.setter
    def episode_length_buf(self, v):           # MHPPO.learn assigns it (mh_ppo.py:208)
        self._episode_length_buf.copy_(v.to(self._episode_length_buf.dtype))

    @property
    def num_rew_fn(self):
        return self.layout.num_rew_fn

    def _build_io(self):
        s = self.simulator
        io = _lib.PbhcStepIO()
        p = lambda t: t.data_ptr()
        io.root_states, io.dof_state = p(s.robot_root_states), p(s.dof_state)
        # the simulator surface's rigid-body state and contact forces: re-derived by the stub on first access (ReplaySimStub.mark_step)
        io.rigid_body_state, io.contact_forces = None, None
        io.actions, io.last_actions, io.actions_after_delay, io.action_queue = p(self.actions), p(self.last_actions), p(self.actions_after_delay), p(self.action_queue)
        io.last_dof_pos, io.last_dof_vel, io.torques = p(self.last_dof_pos), p(self.last_dof_vel), p(self.torques)
        io.feet_air_time, io.contacts, io.contacts_filt = p(self.feet_air_time), p(self.contacts), p(self.contacts_filt)
        io.last_contacts, io.last_contacts_filt = p(self.last_contacts), p(self.last_contacts_filt)
        io.kp_scale, io.kd_scale, io.rfi_lim_scale, io.rao_scale = p(self._kp_scale), p(self._kd_scale), p(self._rfi_lim_scale), p(self._rao_scale)
        io.default_dof_pos = p(self.default_dof_pos) if self._c.randomize_default_dof_pos else None      # per-env defaults only when they are randomised
        io.motion_start_times, io.motion_len, io.end_time_ratio_buf = p(self.motion_start_times), p(self.motion_len), p(self.end_time_ratio_buf)
        io.episode_sums, io.hist = p(self._episode_sums), p(self._hist)
        io.ou_state = p(self._ou_state) if self._c.noise_process else None
        io.episode_length_buf, io.last_episode_length_buf = p(self._episode_length_buf), p(self.last_episode_length_buf)
        io.reset_buf, io.action_delay_idx = p(self.reset_buf), p(self.action_delay_idx)
        self._slot_clip = self._motion_lib.slot_table.contiguous()
        io.motion_ids = p(self._slot_clip)
        io.time_out_buf = p(self.time_out_buf)
        io.env_origins = p(self.env_origins)
        self._friction_flat = s.friction_coeffs.reshape(self.num_envs, -1).contiguous()
        io.dr_base_com, io.dr_link_mass, io.dr_friction = p(s._base_com_bias), p(s._link_mass_scale.contiguous()), p(self._friction_flat)
        io.dr_base_mass = p(s._base_mass_scale)
        L = self.layout
        for i, g in enumerate(L.group_names[:-1]):
            io.obs[i] = p(self.obs_buf_dict[g])
            io.obs_pitch[i] = self.obs_buf_dict[g].stride(0)
        io.obs[len(L.group_names) - 1] = p(self._hist)
        io.obs_pitch[len(L.group_names) - 1] = io.hist_pitch = self._hist.stride(0)
        io.rew_buf = p(self.rew_buf)
        io.ref_body_pos_extend, io.ref_body_rot_extend = None, None          # lazy: rebuilt from ref_time_out on first access (StepExtras)
        io.ref_time_out = p(self._ref_time)
        io.episode_rew_out = p(self._episode_rew_out)
        io.totals_out = self._totals.data_ptr() if getattr(self, "_totals", None) is not None else None
        self._io = io
        self._io_epoch = getattr(self, "_io_epoch", 0) + 1        # captured graphs of the step hold these addresses: a new epoch invalidates them
        self._overrides = {}
        self._replay_version = -1
        if self._start_time is not None and self._start_sampling_live():
            io.ovr_start_time = p(self._start_time)             # the reset path's start time: k_start_draw's buffer (start_sampling)

    def set_profiling(self, on=True):
        """per-launch HIP event pairs on k_env_step (bench.py's roofline meter; read with pbhc_env_profile_read).  While it is on the step
        launches through the hipExt call, which a stream capture cannot record: `rollout_graph_safe` says no."""
        _lib.check(self._lib.pbhc_env_profile(self._env, 1 if on else 0), "pbhc_env_profile")
        self._profiling = bool(on)

    def rollout_graph_safe(self, num_steps):
        """May the next `num_steps` control steps run as ONE captured graph?  Only if nothing in them needs the host: no per-step exchange of
        the batch statistics (data-parallel "step" mode), no re-draw / motion-resample event due inside the window, no per-launch event
        pairs, a replay window in place (the steps then read the frame index from the device-side cursor)."""
        if getattr(self, "_profiling", False) or self._totals is not None or self.simulator.replay is None or self.reinit_epis_rand > 0:
            return False
        if self.config.get("resample_motion_when_training", False):
            nxt = (self.common_step_counter // self.resample_time_interval + 1) * self.resample_time_interval
            if nxt - self.common_step_counter <= num_steps:
                return False
        return True

    def graph_key(self):
        """everything a captured env step froze: the io struct (its epoch moves with every pointer the env re-points), the simulator's replay
        window (a new one is picked up lazily inside the next step(), i.e. AFTER a caller has read this key: the version itself belongs to it),
        which kernel — generic or specialised — the launch names, and the batch size"""
        return (self._io_epoch, self.simulator.replay_version, self.is_specialised, self.num_envs)

    @contextlib.contextmanager
    def graph_steps(self, renew_events):
        """`with env.graph_steps(...)`: the step() calls inside are being recorded into a graph, not run.  They read the replay frame from the
        device-side cursor from now on; the host-side counter they advance is put back (after_graph_steps advances it, per replay).
        renew_events: the steps ran with a finalize stream — its events were recorded INSIDE the capture and are edges of the graph now, not
        events a later eager step may wait on."""
        self.simulator.use_device_cursor()
        counter0 = self.common_step_counter
        try:
            yield
        finally:
            self.common_step_counter = counter0
            self._fin_owed = False                   # (a recorded step owes nothing: what it left owed was recorded too, or the capture failed)
            if renew_events:
                self._step_done, self._fin_done, self._fin_pending = torch.cuda.Event(), torch.cuda.Event(), False

    def after_graph_steps(self, num_steps):
        """host-side book-keeping of `num_steps` control steps that ran inside a graph replay"""
        self.common_step_counter += num_steps
        self._ref_bodies = None
        self.extras.invalidate()
        self.simulator.mark_step(-1)
        self.extras["episode"] = EpisodeExtras(self)
        if self._rec is not None:                    # the replayed graph held one recorder launch per step
            self._record_launches += num_steps
            self._record_host_steps(num_steps)

    def set_eager_outputs(self, on=True):
        """Have the fused step STORE the optional outputs (rigid-body state, contact forces, reference bodies) instead of leaving them to be
        re-derived on access: for a consumer that reads them every step (an evaluation callback), and for the test that holds the two forms
        equal.  `env._eager` holds the four tensors."""
        N, B, Bx, dev = self.num_envs, self.num_bodies, self.skeleton.num_bodies_ext, self.device
        if on:
            self._eager = dict(rigid_body_state=torch.zeros(N, B, 13, device=dev), contact_forces=torch.zeros(N, B, 3, device=dev),
                               ref_body_pos_extend=torch.zeros(N, Bx, 3, device=dev), ref_body_rot_extend=torch.zeros(N, Bx, 4, device=dev))
        else:
            self._eager = None
        for k in ("rigid_body_state", "contact_forces", "ref_body_pos_extend", "ref_body_rot_extend"):
            setattr(self._io, k, self._eager[k].data_ptr() if on else None)
        self._io_epoch += 1

    def set_obs_outputs(self, tensors):
        """Point the observation outputs of the next step(s) at caller-owned `[N, dim]` tensors (e.g. the rollout-buffer slab of
        the next step) instead of the env-owned ones; `None` restores the env-owned buffers."""
        L = self.layout
        for i, g in enumerate(L.group_names[:-1]):
            t = self._own_obs[g] if tensors is None else _lib.require_gpu_rows(tensors[g], g, torch.float32, (self.num_envs, L.group_dims[g]))
            self.obs_buf_dict[g] = t
            self._io.obs[i] = t.data_ptr()
            self._io.obs_pitch[i] = t.stride(0)

    # ---- test / replay hooks: inject the random draws instead of the in-kernel Philox ---------
    def set_injected_draws(self, u_rfi=None, start_time=None, kp=None, kd=None, rfi_lim=None, rao=None, delay=None, dof_pos_bias=None, gate_u=None,
                           reset_root=None, reset_dof_pos=None, reset_dof_vel=None, ou_step=None, ou_reset=None, ps_kp=None, ps_kd=None, ps_rao=None,
                           ps_tau=None):
        """Keeps the tensors alive and points the kernel at them (None -> in-kernel RNG).  reset_root [N,13] / reset_dof_pos, reset_dof_vel [N,D]:
        the raw draws of the reset-state noise (PbhcStepIO.ovr_reset_*), consumed by the envs that reset.  ou_step / ou_reset [N,6]: the normals
        of the OU step (every env) and of its stationary redraw (envs that reset); ps_kp / ps_kd [N,J_pd]: the U(ratio) factors of
        parallel_serial_pd; ps_rao / ps_tau [N,J_tau]: parallel_serial_tau's episodic and per-step normals."""
        self._overrides = dict(u_rfi=u_rfi, ovr_start_time=start_time, ovr_kp=kp, ovr_kd=kd, ovr_rfi_lim=rfi_lim, ovr_rao=rao, ovr_delay=delay,
                               ovr_dof_pos_bias=dof_pos_bias, ovr_gate_u=gate_u, ovr_reset_root=reset_root, ovr_reset_dof_pos=reset_dof_pos,
                               ovr_reset_dof_vel=reset_dof_vel, ovr_ou_step=ou_step, ovr_ou_reset=ou_reset, ovr_ps_kp=ps_kp, ovr_ps_kd=ps_kd,
                               ovr_ps_rao=ps_rao, ovr_ps_tau=ps_tau)
        self._io_epoch += 1
        for k, v in self._overrides.items():
            setattr(self._io, k, None if v is None else v.data_ptr())
        self._point_start_time()                     # start_sampling: injected start times win while set, clearing them re-points the buffer

    # ---- data-parallel runs: batch statistics over ALL ranks' envs ---------------------------
    def enable_global_statistics(self, group=None, mode="rollout"):
        """One process per GPU, envs sharded over ranks: adaptive sigma, average episode length, the curricula keyed on it and the logged
        means are batch statistics of the reference's single process (motion_tracking.py:1030-1048, legged_robot_base.py:875-900).
          mode "rollout" (default): every step updates them from THIS rank's shard (4096 envs: already a tight estimate), and
                 `sync_globals()` — called by the agents once per rollout — replaces every rank's copy by the mean over the ranks: ONE
                 1 KB all-reduce per PPO iteration, nothing on the step -> policy -> step chain;
          mode "step": each step writes its shard's batch sums (PBHC_NUM_TOTALS doubles), ONE 512-byte all-reduce sums them over the ranks
                 while the next policy forward runs, and `pbhc_env_finalize` applies them right before the next step launches: every rank
                 then holds exactly the sigma / curriculum state ONE process with all the envs would (tests/test_gpu_dist.py) — at 24
                 latency-critical collectives per iteration."""
        if not pdist.active(group):
            return False
        if self._c.terminate_when_dof_far:
            # one env past the threshold resets every env (motion_tracking.py:343-349): across ranks that is a collective before every step's
            # reset path — on the step -> policy -> step chain — and each rank deciding alone would not be the reference's batch
            raise NotImplementedError("termination.terminate_when_dof_far under data parallelism: the batch-global decision would need a "
                                      "cross-rank collective every step")
        assert mode in ("rollout", "step"), mode
        self._flush_statistics()
        self._stat_group, self._stat_mode = group, mode
        if mode == "step":
            n = torch.tensor([float(self.num_envs)], dtype=torch.float64, device=self.device)
            pdist.all_reduce(n, group=group)
            self._num_envs_total = float(n)
            self._totals = torch.zeros(K["PBHC_NUM_TOTALS"], dtype=torch.float64, device=self.device)
            self._io.totals_out = self._totals.data_ptr()
        return True

    def sync_globals(self):
        """mode "rollout": the batch-statistics state (sigma, EMA, curricula, log means: the `globals` vector) becomes the mean over the ranks"""
        if getattr(self, "_stat_mode", None) != "rollout":
            return
        self.wait_finalize()
        pdist.allreduce_mean_(self.globals, group=self._stat_group)
        # the step counter (the kernels' Philox counter, read as (uint32_t)) is the same integer on every rank; a mean formed as
        # sum(x / n) may come back one ulp short for world sizes that are not powers of two — truncation would then replay a counter
        c = K["PBHC_G_STEP_COUNTER"]
        self.globals[c:c + 1].round_()

    def set_finalize_stream(self, stream):
        """Run every step's one-workgroup reduction (`pbhc_env_step_finish`: sigma EMA, curricula, log means, step counter) on `stream`
        instead of the stepping stream (None: back to one stream).  The env orders it after its fused launch and joins it before the next
        one; a caller that reads the globals on the stepping stream in between (pbhc_policy_sample reads the step counter) calls
        `wait_finalize()` first."""
        self.wait_finalize()
        if stream is not None and self._fin_deferred:
            raise _lib.PbhcError("set_finalize_stream: the env leaves its reductions to riders (set_finalize_deferred)")
        self._finalize_stream = stream
        if stream is not None and self._step_done is None:
            self._step_done, self._fin_done = torch.cuda.Event(), torch.cuda.Event()

    def set_finalize_deferred(self, on):
        """on: a step launches its fused kernel only (`pbhc_env_step_launch`) and leaves its one-workgroup reduction OWED — no finish launch,
        no side stream, no event.  The caller takes the reduction over as a rider of a launch of its own that follows the step on the stepping
        stream (`take_finalize_rider()`: the rollout's next policy forward, agents/rollout.py); whatever nobody took is launched as the plain
        `pbhc_env_step_finish` by `flush_finalize()`, which the next step and every reader of the globals call first (through
        `wait_finalize()`), so that no caller can step on, or read, stale globals by forgetting.  off: back to a reduction per step, after
        flushing.  Not with a finalize stream, the per-step statistics exchange, or the clip / start collectors (they live behind the
        reduction)."""
        if on and (self._finalize_stream is not None or self._totals is not None or self._clip_window is not None or self._start_window is not None):
            raise _lib.PbhcError("set_finalize_deferred: not with a finalize stream, the per-step statistics exchange or the clip / start collectors")
        if not on:
            self.flush_finalize()
        self._fin_deferred = bool(on)

    def _sync_replay_io(self):
        """the step's view of the simulator's replay window (frame arrays, cursor, length), picked up lazily after the simulator got a new one"""
        s, io = self.simulator, self._io
        if self._replay_version != s.replay_version or s.replay is None:
            s.ensure_replay()
            r = s.replay
            io.frame_root, io.frame_dof_pos = r["root"].data_ptr(), r["dof_pos"].data_ptr()
            io.frame_dof_vel, io.frame_contact = r["dof_vel"].data_ptr(), r["contact"].data_ptr()
            io.frame_cursor, io.num_frames = s.frame_cursor.data_ptr(), s.replay_len
            self._replay_version = s.replay_version
            self._io_epoch += 1

    def finalize_rider(self):
        """-> a `PbhcRider` whose finalize half describes this env's reduction (nothing is launched, no state changes): the same for every
        step while `graph_key()` stays what it is — a captured launch may hold it"""
        self._sync_replay_io()
        r = _lib.PbhcRider()
        _lib.check(self._lib.pbhc_env_finalize_rider(self._env, C.byref(self._io), C.byref(r)), "pbhc_env_finalize_rider")
        return r

    @property
    def finalize_owed(self):
        """a deferred step's reduction is still to be launched or taken (False again once something on the way flushed it)"""
        return self._fin_owed

    def take_finalize_rider(self):
        """The caller runs the owed reduction of the last step as a rider of a launch it queues NEXT on the stepping stream, before anything
        that reads the globals: -> the descriptor (`finalize_rider()`); the reduction counts as handed over."""
        if not self._fin_owed:
            raise _lib.PbhcError("take_finalize_rider: no reduction is owed (set_finalize_deferred(True), then step())")
        self._fin_owed = False
        return self.finalize_rider()

    def flush_finalize(self):
        """launch the reduction a deferred step still owes (if any) as the plain `pbhc_env_step_finish` on the current stream"""
        if self._fin_owed:
            self._fin_owed = False
            _lib.check(self._lib.pbhc_env_step_finish(self._env, C.byref(self._io), _lib.current_stream()), "pbhc_env_step_finish")

    def wait_finalize(self):
        """the current stream is behind the last step's reduction: waits for the finalize stream's (no-op on one stream), launches an owed one"""
        self.flush_finalize()
        if self._fin_pending:
            torch.cuda.current_stream().wait_event(self._fin_done)
            self._fin_pending = False

    def finalize_joined(self):
        """The caller has made the stepping stream wait for something it queued on the finalize stream AFTER the last step's reduction
        (the rollout's book-keeping kernel): that wait covers the reduction, a second cross-stream wait (~10 us of dispatch latency each,
        signalled or not) is not needed."""
        self._fin_pending = False

    def _flush_statistics(self):
        h = self._stat_pending
        if h is not None:
            self._stat_pending = None
            h.wait()
            _lib.check(self._lib.pbhc_env_finalize(self._env, self._totals.data_ptr(), self._num_envs_total, _lib.current_stream()), "pbhc_env_finalize")

    # ------------------------------------------------------------------------------------
    def set_is_evaluating(self):
        self.is_evaluating = True

    @property
    def is_evaluating(self):
        return self._is_evaluating

    @is_evaluating.setter
    def is_evaluating(self, v):
        """(a property since start_sampling: evaluation suspends it — the step's start-time pointer and the collector follow the flag)"""
        changed = bool(v) != self._is_evaluating
        self._is_evaluating = bool(v)
        if changed and getattr(self, "_start_window", None) is not None:
            self._io_epoch += 1                      # a captured graph of steps holds, or does not hold, the collector's launches
            self._point_start_time()

    def _resample_motion_times(self, env_ids):
        # motion_tracking.py:369-378
        if len(env_ids) == 0:
            return
        self.motion_len[env_ids] = self._motion_lib.get_motion_length(self.motion_ids[env_ids])
        if self.is_evaluating and not self.config.enforce_randomize_motion_start_eval:
            self.motion_start_times[env_ids] = 0.0
        elif self._start_time is not None and self._start_sampling_live():
            self.motion_start_times[env_ids] = self._start_time[env_ids]
            self._redraw_start_times()               # a draw is used once
        else:
            self.motion_start_times[env_ids] = self._motion_lib.sample_time(self.motion_ids[env_ids])

    def _reference_bodies(self):
        """(ref_body_pos_extend [N,Bx,3], ref_body_rot_extend [N,Bx,4]) of the LAST step: the lookup the fused kernel did at `_ref_time`
        (before a reset), repeated with the stand-alone lookup kernel — cached until the next step"""
        if self._ref_bodies is None:
            ref = self._motion_lib.get_motion_state(self.motion_ids, self._ref_time, offset=self.env_origins)
            self._ref_bodies = (ref["rg_pos_t"], ref["rg_rot_t"])
        return self._ref_bodies

    @property
    def ref_body_pos_extend(self):
        return self._reference_bodies()[0]

    @property
    def ref_body_rot_extend(self):
        return self._reference_bodies()[1]

    def resample_motion(self, keep_reset_buf=False):
        """motion_tracking.py:385-389 / general_tracking.py:291-297"""
        if self._clip_window is not None or self._start_window is not None:
            self.wait_finalize()                     # the collectors of the last step, on the finalize stream, read the OLD slot -> clip table
        if self.common_step_counter > 0:
            self._reference_bodies()                 # the last step's lazy reference bodies belong to the OLD slot -> clip table: freeze them
        if self._clip["sampling"]:
            # all-reduce (data parallel) -> update kernel -> device slot draw -> crop rebuild; the reset below cuts episodes short that are
            # not counted: only step() launches the collector
            self.update_clip_sampling()
            self._motion_lib.sample_slots_device(self._seed, self._clip_draws)
            self._clip_draws += 1
        else:
            self._motion_lib.load_motions(random_sample=True, max_len=self.max_len)
        self.curr_motion_ids = self._motion_lib.slot_clip
        self._redraw_start_times()                   # start_sampling: the buffered start times belong to the OLD table's clip lengths
        self._reset_all_state(keep_reset_buf=keep_reset_buf)

    def reset_all(self):
        """base_task.py:83-93: reset every env, then one step with zero actions.  Start-up path,
        done with torch ops on the device (the per-step reset of terminated envs is in the kernel)."""
        self._reset_all_state()
        obs_dict, _, _, _ = self.step({"actions": torch.zeros(self.num_envs, self.dim_actions, device=self.device)})
        return obs_dict

    def _reset_all_state(self, keep_reset_buf=False):
        """reset_envs_idx(arange(N)) (legged_robot_base.py:491-517).  keep_reset_buf: the periodic resample inside step() — the reference's
        resample_motion() resets every env WITHOUT touching reset_buf, the dones of that step stay those of its own _check_termination."""
        self.wait_finalize()
        N, dev = self.num_envs, self.device
        ids = torch.arange(N, device=dev)
        g = self.globals
        # _reset_buffers_callback (legged_robot_base.py:670-686)
        for t in (self.actions, self.last_actions, self.actions_after_delay, self.last_dof_pos, self.last_dof_vel, self.feet_air_time,
                  self.contacts, self.contacts_filt, self.last_contacts, self.last_contacts_filt, self._hist):
            t.zero_()
        self._flush_statistics()
        cur = torch.mean(self.last_episode_length_buf, dtype=torch.float)
        n_all = N
        if self._totals is not None:                       # every rank resets all its envs: the mean over all ranks' envs
            m = torch.stack([self.last_episode_length_buf.sum().double(), torch.tensor(float(N), dtype=torch.float64, device=dev)])
            pdist.all_reduce(m, group=self._stat_group)
            cur, n_all = (m[0] / m[1]).float(), float(m[1])
        frac = n_all / self._c.num_compute_average_epl
        avg = g[K["PBHC_G_AVG_EP_LEN"]].float() * (1 - frac) + cur * frac
        g[K["PBHC_G_AVG_EP_LEN"]] = avg.double()
        self._episode_length_buf.zero_()
        if not keep_reset_buf:
            self.reset_buf.fill_(1)
        self._episodic_domain_randomization_all()
        # curricula keyed on average_episode_length (legged_robot_base.py:882-900, motion_tracking.py:309-317)
        c = self._c
        avg_f = float(avg)
        if c.penalty_curriculum:
            p = float(g[K["PBHC_G_PENALTY_SCALE"]])
            p *= (1 - c.penalty_degree) if avg_f < c.penalty_down else ((1 + c.penalty_degree) if avg_f > c.penalty_up else 1.0)
            g[K["PBHC_G_PENALTY_SCALE"]] = float(np.clip(p, c.penalty_min, c.penalty_max))
        if c.noise_curriculum:
            v = float(g[K["PBHC_G_NOISE_CURRICULUM"]])
            v *= (1 - c.noise_degree) if avg_f < c.noise_down else ((1 + c.noise_degree) if avg_f > c.noise_up else 1.0)
            g[K["PBHC_G_NOISE_CURRICULUM"]] = float(np.clip(v, c.noise_min, c.noise_max))
        end_time = self.last_episode_length_buf * self.dt + self.motion_start_times
        self.end_time_ratio_buf.copy_(end_time / self.motion_len.clamp(min=1e-9))
        self._resample_motion_times(ids)
        if c.terminate_when_motion_far and c.motion_far_curriculum:
            t = float(g[K["PBHC_G_MOTION_FAR_THR"]])
            t *= (1 + c.motion_far_degree) if avg_f < c.motion_far_down else ((1 - c.motion_far_degree) if avg_f > c.motion_far_up else 1.0)
            g[K["PBHC_G_MOTION_FAR_THR"]] = float(np.clip(t, c.motion_far_min, c.motion_far_max))
        if c.terminate_when_dof_far and c.dof_far_curriculum:                    # motion_tracking.py:283-292, the same call site
            t = float(g[K["PBHC_G_DOF_FAR_THR"]])
            t *= (1 + c.dof_far_degree) if avg_f < c.dof_far_down else ((1 - c.dof_far_degree) if avg_f > c.dof_far_up else 1.0)
            g[K["PBHC_G_DOF_FAR_THR"]] = float(np.clip(t, c.dof_far_min, c.dof_far_max))
        # _reset_dofs / _reset_root_states from the reference frame at (0+1)*dt + start
        ref = self._motion_lib.get_motion_state(self.motion_ids, (self._episode_length_buf + 1) * self.dt + self.motion_start_times, offset=self.env_origins)
        s = self.simulator
        ref_dof = ref if self.TRACKING_MODE == 0 else self._motion_lib.get_motion_state(       # general_tracking.py:463-476: t = ep_len*dt + start
            self.motion_ids, self._episode_length_buf * self.dt + self.motion_start_times, offset=self.env_origins)
        s.dof_pos.copy_(ref_dof["dof_pos"]); s.dof_vel.copy_(ref_dof["dof_vel"])
        s.robot_root_states[:, 0:3] = ref["root_pos"]; s.robot_root_states[:, 3:7] = ref["root_rot"]
        s.robot_root_states[:, 7:10] = ref["root_vel"]; s.robot_root_states[:, 10:13] = ref["root_ang_vel"]
        if c.reset_noise:
            self._reset_state_noise()
        self._reset_all_noise_process_and_parallel_serial()
        self.extras["episode"] = {"rew_" + k: (v / self.max_episode_length_s).clone() for k, v in self.episode_sums.items()}
        self.extras["episode"]["end_epis_length"] = self.last_episode_length_buf.clone()
        self._episode_sums.zero_()
        self.extras["time_outs"] = self.time_out_buf

    def _reset_state_noise(self):
        """noise_to_initial_level != 0: _reset_dofs / _reset_root_states of every env (motion_tracking.py:470-545, general_tracking.py:405-485)
        on the state just written, with the env's generator (the kernel's per-env resets draw from Philox streams of their own)."""
        N, D, dev, c, s = self.num_envs, self.num_dof, self.device, self._c, self.simulator
        gen = self._gen
        draw = torch.randn if self.TRACKING_MODE == 0 else torch.rand            # general tracking: rand_like on the dofs, sic
        s.dof_pos.add_(draw(N, D, device=dev, generator=gen) * c.rn_dof_pos)
        s.dof_vel.add_(draw(N, D, device=dev, generator=gen) * c.rn_dof_vel)
        rs = s.robot_root_states
        rs[:, 0:3] += torch.randn(N, 3, device=dev, generator=gen) * c.rn_root_pos
        axis = torch.randn(N, 3, device=dev, generator=gen)
        axis = axis / torch.norm(axis, dim=1, keepdim=True)
        half = c.rn_root_rot * torch.rand(N, 1, device=dev, generator=gen) / 2
        small = torch.cat([torch.sin(half) * axis, torch.cos(half)], dim=1)        # small_random_quaternions (xyzw)
        rs[:, 3:7] = _quat_mul_xyzw(small, rs[:, 3:7].clone())
        rs[:, 7:10] += torch.randn(N, 3, device=dev, generator=gen) * c.rn_root_vel
        rs[:, 10:13] += torch.randn(N, 3, device=dev, generator=gen) * c.rn_root_ang_vel

    def _episodic_domain_randomization_all(self):
        """_episodic_domain_randomization(arange(N)) (legged_robot_base.py:599-635): kp / kd / rfi-limit / rao scales, control delay."""
        N, dev, D = self.num_envs, self.device, self.num_dof
        dr = self.config.domain_rand
        u = lambda lo, hi: (hi - lo) * torch.rand(N, D, device=dev, generator=self._gen) + lo
        if dr.randomize_pd_gain:
            self._kp_scale.copy_(u(dr.kp_range[0], dr.kp_range[1]))
            self._kd_scale.copy_(u(dr.kd_range[0], dr.kd_range[1]))
        if dr.randomize_rfi_lim:
            self._rfi_lim_scale.copy_(u(dr.rfi_lim_range[0], dr.rfi_lim_range[1]))
        if dr.use_rao:
            self._rao_scale.copy_(u(-dr.rao_lim, dr.rao_lim))
        if dr.randomize_ctrl_delay:
            self.action_queue.zero_()
            self.action_delay_idx.copy_(torch.randint(dr.ctrl_delay_step_range[0], dr.ctrl_delay_step_range[1] + 1, (N,), device=dev, generator=self._gen))
        if dr.get("randomize_default_dof_pos", False):                            # legged_robot_base.py:632-635
            self.default_dof_pos.copy_(u(dr.dof_pos_range[0], dr.dof_pos_range[1]) + self.raw_default_dof_pos)

    def _reset_all_noise_process_and_parallel_serial(self):
        """The host-side forms of parallel_serial_pd / parallel_serial_tau (the episodic part) and of the OU redraw, for every env.  Drawn
        LAST from the env's generator, so that every other draw of _reset_all_state is the same with the switches on or off (the reference's
        draw order on its generator is not reproduced anyway); the arithmetic is the reference's: the factors multiply the gains that
        _episodic_domain_randomization_all left, the normals add to the rao scale it drew."""
        N, dev, c, L = self.num_envs, self.device, self._c, self.layout
        if c.ps_pd:                    # legged_robot_base.py:607-613: compounds on the old scale when randomize_pd_gain is off
            r = lambda: (c.ps_pd_ratio[1] - c.ps_pd_ratio[0]) * torch.rand(N, c.ps_pd_num, device=dev, generator=self._gen) + c.ps_pd_ratio[0]
            self._kp_scale[:, L.ps_pd_idx] *= r()
            self._kd_scale[:, L.ps_pd_idx] *= r()
        if c.ps_tau and c.use_rao:     # :621-623, accumulating; without use_rao the scale never reaches the torque, so it is not drawn
            self._rao_scale[:, L.ps_tau_idx] += c.ps_tau_rao_lim * torch.randn(N, c.ps_tau_num, device=dev, generator=self._gen)
        if c.noise_process:            # _reset_tasks_callback -> noise_process.reset_part (:593-597)
            self._ou_state.copy_(self._ou_stationary(N))

    def _ou_stationary(self, n):
        """n draws of the OU process's stationary law, mu + sigma / sqrt(2 theta) N(0,1) per component (noise_tool.py OUProcess.reset_part)"""
        c = self._c
        return torch.randn(n, 6, device=self.device, generator=self._gen) * c.ou_sigma / c.ou_sqrt_2theta + c.ou_mu

    @property
    def noise_process_state(self):
        """the OU state of obs.noise_process [N, 6] (rpy, angular velocity), as the reference's env.noise_process.x; zeros when it is off"""
        return self._ou_state

    def step(self, actor_state):
        """legged_robot_base.py:239-265 — one fused launch."""
        actions = actor_state["actions"]
        if actions.dtype != torch.float32 or not actions.is_contiguous() or actions.device != self.device:
            actions = actions.to(self.device, torch.float32).contiguous()
        if tuple(actions.shape) != (self.num_envs, self.num_dof):
            raise _lib.PbhcError(f"actions must be [{self.num_envs},{self.num_dof}], got {tuple(actions.shape)}")
        self._actions_in = actions
        s = self.simulator
        io = self._io
        io.actions_in = actions.data_ptr()
        self.flush_finalize()                        # (a deferred step's reduction nobody took: before io moves on, and before this step)
        self._sync_replay_io()
        io.frame_index = s.take_host_frame()
        # _update_tasks_callback's re-draw of every env's episodic DR (legged_robot_base.py:390-395): decided on the host, done by the kernel
        # in this very step (after its torques, before its observations — where the reference does it)
        io.redraw_all = int(self._reinit.due(self.common_step_counter + 1))
        self._ref_bodies = None                      # the lazy members of last step's extras end here
        self.extras.invalidate()
        s.mark_step(io.frame_index)                  # the stub's rigid-body state / contact forces of this step: re-derived on first access
        # the previous step's lazy extras["episode"]: gather it now if somebody kept it (its buffers are about to be overwritten)
        prev = self.extras.pop("episode", None)
        if isinstance(prev, EpisodeExtras) and prev._data is None and sys.getrefcount(prev) > 2:
            prev.materialise()
        del prev
        self._flush_statistics()
        fs = self._finalize_stream
        advance = getattr(s, "advance", None)        # a closed-loop simulator writes this step's frame directly in front of the step launch
        if self._fin_deferred:
            # the fused launch only: its reduction is owed (set_finalize_deferred) — taken over by the caller's next launch on this stream, or
            # flushed before the next step / the next reader of the globals
            st = _lib.current_stream()
            if advance is not None:
                advance(self)
            _lib.check(self._lib.pbhc_env_step_launch(self._env, C.byref(io), st), "pbhc_env_step_launch")
            if self._rec is not None:                # the recorder needs the step's per-env outputs only, not its reduction
                _lib.check(self._lib.pbhc_record_motion(self._env, C.byref(io), C.byref(self._rec_io), st), "pbhc_record_motion")
            self._fin_owed = True
        elif fs is None:
            if advance is not None:
                advance(self)
            _lib.check(self._lib.pbhc_env_step(self._env, C.byref(io), _lib.current_stream()), "pbhc_env_step")
            if self._rec is not None:
                _lib.check(self._lib.pbhc_record_motion(self._env, C.byref(io), C.byref(self._rec_io), _lib.current_stream()), "pbhc_record_motion")
            if self._clip_window is not None:
                self._launch_clip_stats(_lib.current_stream())
            if self._start_window is not None:
                self._launch_start_sampling(_lib.current_stream())
        else:
            # the fused launch here, its one-workgroup reduction on the side stream (set_finalize_stream): this stream goes straight on to
            # the policy forward of the new observations; the reduction is joined again before the next launch (wait_finalize)
            cur = torch.cuda.current_stream()
            self.wait_finalize()
            if advance is not None:
                advance(self)
            _lib.check(self._lib.pbhc_env_step_launch(self._env, C.byref(io), cur.cuda_stream), "pbhc_env_step_launch")
            if self._rec is not None:                # the recorder needs the step's per-env outputs only, not its reduction
                _lib.check(self._lib.pbhc_record_motion(self._env, C.byref(io), C.byref(self._rec_io), cur.cuda_stream), "pbhc_record_motion")
            self._step_done.record(cur)
            fs.wait_event(self._step_done)
            _lib.check(self._lib.pbhc_env_step_finish(self._env, C.byref(io), fs.cuda_stream), "pbhc_env_step_finish")
            if self._clip_window is not None:        # off the step -> policy -> step chain; wait_finalize() orders it before the next step
                self._launch_clip_stats(fs.cuda_stream)
            if self._start_window is not None:       # behind the reduction: the step counter k_start_draw keys its draw with is settled
                self._launch_start_sampling(fs.cuda_stream)
            self._fin_done.record(fs)
            self._fin_pending = True
        if self._totals is not None:
            if fs is None:
                self._stat_pending = pdist.all_reduce(self._totals, group=self._stat_group, async_op=True)
            else:
                with torch.cuda.stream(fs):      # the shard's totals are written by the reduction on the side stream: the exchange follows it there
                    self._stat_pending = pdist.all_reduce(self._totals, group=self._stat_group, async_op=True)
        self.common_step_counter += 1
        # _update_tasks_callback (motion_tracking.py:320-325, general_tracking.py:216-222): periodic slot -> clip resampling + reset of every
        # env.  The reference does it inside the step, before termination and reward of that step; here it follows the fused launch, i.e.
        # it takes effect one control step later — once every resample_time_interval (50 000 - 100 000 steps in the shipped configs).
        # The dones returned for this step stay the kernel's own (the reference's resample_motion does not touch reset_buf).
        if self.config.get("resample_motion_when_training", False) and self.common_step_counter % self.resample_time_interval == 0:
            self.resample_motion(keep_reset_buf=True)
        else:
            self.extras["episode"] = EpisodeExtras(self)
        self.extras["time_outs"] = self.time_out_buf
        self.extras["to_log"] = self.log_dict
        self.extras["episode_rew"] = self._episode_rew_out
        if self._rec is not None and not torch.cuda.is_current_stream_capturing():
            # (a step that is being captured runs later, as part of a graph replay: after_graph_steps counts it)
            self._record_launches += 1
            self._record_host_steps(1)
        return self.obs_buf_dict, self.rew_buf, self.reset_buf, self.extras

    # ---- evaluation recorder (env.config.save_motion, opt/record.yaml) ------------------------
    def _init_save_motion(self):
        """motion_tracking.py:140-170.  The reference appends twelve `.cpu()` copies to python lists in every control step; here the frames
        go to device-resident [N, T, ...] buffers (T = save_total_steps), written by k_record_motion right after the fused step, indexed by
        a device-side counter: nothing of it touches the host until the recording is complete."""
        self.save_motion, self._rec, self._record_launches = False, None, 0
        if "save_motion" not in self.config:
            return
        self._motion_episode_length = torch.ceil((self.motion_len / self.dt)[0]).int()
        assert (self._motion_episode_length - self.motion_len[0] / self.dt).norm() < 1, f"Motion length {self.motion_len} is not divisible by motion dt {self.dt}, {self._motion_episode_length=}, {(self._motion_episode_length- self.motion_len[0]/self.dt).norm()=}"
        assert self._motion_episode_length > 0, f"Motion length {self.motion_len} is not positive"
        R = self.layout.record
        if R is None:                                # save_motion: False
            return
        if R["ckpt_dir"] is None:
            raise _lib.PbhcError("env.config.save_motion needs env.config.ckpt_dir (the recording goes to {ckpt_dir}/motions/)")
        N, T, dev = self.num_envs, R["total_steps"], self.device
        per_frame = sum(int(np.prod(shape, dtype=np.int64)) * (8 if k == "terminate" else 4) for k, shape in R["rows"].items())
        need = N * T * per_frame
        free = torch.cuda.mem_get_info(dev)[0]
        if need > free:
            raise _lib.PbhcError(f"env.config.save_motion: the recording buffers take num_envs x save_total_steps x {per_frame} B = {N} x {T} x "
                                 f"{per_frame} = {need} bytes ({need / 2**30:.2f} GiB); {free} bytes ({free / 2**30:.2f} GiB) of device memory are free")
        os.makedirs(os.path.join(str(R["ckpt_dir"]), "motions"), exist_ok=True)
        self.save_motion_dir = os.path.join(str(R["ckpt_dir"]), "motions", f"{R['save_note']}_{R['eval_timestamp']}")
        self.save_motion = True
        self.num_augment_joint = self.num_extend_bodies
        self._write_to_file = True
        self._rec = {k: torch.zeros((N, T) + tuple(shape), dtype=torch.int64 if k == "terminate" else torch.float32, device=dev)
                     for k, shape in R["rows"].items()}
        self._rec_counter = torch.zeros(K["PBHC_REC_COUNTER_WORDS"], dtype=torch.int32, device=dev)
        self._rec_steps, self._rec_dumped, self._saved_motion_dict = 0, False, None
        rio = _lib.PbhcRecordIO()
        rio.total_steps, rio.obs_group, rio.counter = T, R["obs_group"], self._rec_counter.data_ptr()
        for k, t in self._rec.items():
            setattr(rio, k, t.data_ptr())
        self._rec_io = rio

    def _record_host_steps(self, n):
        """host mirror of the recorder's device-side counter; the step that completes the recording writes the file (never inside a capture:
        its callers are step() outside a capture and after_graph_steps())"""
        self._rec_steps += n
        if not self._rec_dumped and self._rec_steps >= self.layout.record["total_steps"] + 3:
            self._rec_dumped = True
            self._dump_motion()

    @property
    def recorded_steps(self):
        """control steps the recorder has seen since the env was built"""
        return self._rec_steps

    def clip_of_env(self, i):
        """the motion clip env `i` tracks (what its recording is scored against)"""
        return self._motion_lib.built_clip(int(self._motion_lib.slot_clip[i]))

    @property
    def motion_recorded(self):
        """True once save_total_steps + 3 control steps have run with the recorder on"""
        return self._rec is not None and self._rec_steps >= self.layout.record["total_steps"] + 3

    def recorded_motion_device(self):
        """the complete recording as device tensors [N, T, ...] (the recorder's own buffers, no copy) + fps: what
        pbhc_amd.eval.metrics.eval_batch_traj_device takes"""
        if not self.motion_recorded:
            raise _lib.PbhcError("recorded_motion_device: no complete recording (env.config.save_motion on and save_total_steps + 3 steps run?)")
        return dict(self._rec, fps=1 / self.dt)

    @property
    def saved_motion_dict(self):
        """the reference's attribute (motion_tracking.py:869-876): numpy arrays [N, T, ...] per key, available once save_total_steps + 3
        steps have run; one device -> host copy on first access"""
        if not self.motion_recorded:
            raise AttributeError("saved_motion_dict: not available before save_total_steps + 3 steps have run with env.config.save_motion on")
        if self._saved_motion_dict is None:
            self._saved_motion_dict = {k: self._rec[k].cpu().numpy() for k in env_config.RECORD_KEYS}
        return self._saved_motion_dict

    def _dump_motion(self):
        """motion_tracking.py:878-898: one entry per env, `motion{i}` -> per-key arrays + fps, joblib-compressed"""
        N, T = self.num_envs, self.layout.record["total_steps"]
        save_path = f"{self.save_motion_dir}_{N}x{T}-{int(self._motion_episode_length)}.pkl"
        if not self._write_to_file:
            print(f"Not saving motion data to {save_path}, because {self._write_to_file=}")
            return
        import joblib

        d = self.saved_motion_dict
        dump_data = {}
        for i in range(N):
            dump_data[f"motion{i}"] = {key: d[key][i] for key in d}
            dump_data[f"motion{i}"]["fps"] = 1 / self.dt
        joblib.dump(dump_data, save_path, compress=3)
        self.saved_motion_path = save_path
        print(f"Saved motion data to {save_path}")

    # ---- per-clip episode statistics / failure-weighted clip sampling (env.config.clip_statistics, clip_sampling) ----
    def _init_clip_statistics(self):
        """`_clip_window [M,4]` int64 (episodes, failures, sum of end_time_ratio * 2^24, sum of episode lengths) per unique clip, filled by
        k_clip_stats after every fused step: nothing of it touches the host.  None when the keys are absent — then no launch is added."""
        self._clip = env_config.clip_options(self.config)
        self._clip_window, self._clip_draws = None, 0
        if self._clip["statistics"]:
            self._clip_window = torch.zeros(self._motion_lib._num_unique_motions, 4, dtype=torch.int64, device=self.device)

    def _launch_clip_stats(self, stream):
        ml = self._motion_lib
        _lib.check(self._lib.pbhc_clip_stats(self.reset_buf.data_ptr(), self.time_out_buf.data_ptr(), self.end_time_ratio_buf.data_ptr(),
                                             self.last_episode_length_buf.data_ptr(), ml.slot_clip.data_ptr(), self.num_envs,
                                             ml._num_unique_motions, self._clip_window.data_ptr(), stream), "pbhc_clip_stats")

    def _require_clip_statistics(self, what):
        if self._clip_window is None:
            raise _lib.PbhcError(f"{what}: env.config.clip_statistics (or clip_sampling.enable) is not set")

    def clip_statistics(self):
        """The episodes that ended in step() since the window was last cleared, per unique clip, as device tensors [M]: `episodes`,
        `failures` (int64; an episode that ended without a time-out), `end_time_ratio_mean`, `episode_length_mean` (float64, 0 where a
        clip has no episode).  No host synchronisation."""
        self._require_clip_statistics("clip_statistics")
        self.wait_finalize()
        w = self._clip_window
        e = w[:, 0].clone()
        n = e.clamp(min=1).double()
        return dict(episodes=e, failures=w[:, 1].clone(), end_time_ratio_mean=w[:, 2].double() / 16777216.0 / n,
                    episode_length_mean=w[:, 3].double() / n)

    def clear_clip_statistics(self):
        self._require_clip_statistics("clear_clip_statistics")
        self.wait_finalize()
        self._clip_window.zero_()

    def update_clip_sampling(self):
        """Fold the window into the motion library's sampling hooks (`_sampling_history`, `_termination_history`, `_success_rate`,
        `_sampling_prob`) with the configured decay / prior_episodes / uniform_floor, and clear it.  Data parallel: the window is first
        summed over the ranks (one exact int64 all-reduce), so every rank holds the same probabilities.  resample_motion() calls it when
        clip_sampling is enabled; public, so that a user can fold at their own cadence."""
        self._require_clip_statistics("update_clip_sampling")
        self.wait_finalize()
        group = getattr(self, "_stat_group", None)
        if pdist.active(group):
            pdist.all_reduce(self._clip_window, group=group)
        c = self._clip
        self._motion_lib.update_sampling_device(self._clip_window, c["decay"], c["prior_episodes"], c["uniform_floor"])

    # ---- failure-weighted start-time sampling (env.config.start_statistics, start_sampling; csrc/pbhc_start_sampling.hip) ----
    def _init_start_sampling(self):
        """`_start_window [M,K,2]` int64 (visit differences, failures per phase bin of every unique clip), filled by k_start_stats after
        every fused step, and — start_sampling.enable — `_start_time [N]`: the start time every env takes at its NEXT reset, which the step
        reads through PbhcStepIO.ovr_start_time and k_start_draw refreshes for the envs that just reset.  Both None when the keys are
        absent: no buffer, no launch, the pointer stays NULL."""
        self._start = env_config.start_options(self.config)
        self._start_window, self._start_time, self._start_redraws, self._start_suspended = None, None, 0, False
        if not self._start["statistics"]:
            return
        ml = self._motion_lib
        if ml.max_len > 0:
            raise _lib.PbhcError("env.config.start_sampling / start_statistics cannot be combined with robot.motion.motion_max_len crops: slot "
                                 "times are crop-relative there, a phase bin of the clip means nothing")
        ml.init_start_sampling(self._start["bins"])
        self._start_window = torch.zeros(ml._num_unique_motions, self._start["bins"], 2, dtype=torch.int64, device=self.device)
        if self._start["sampling"]:
            self._start_time = torch.zeros(self.num_envs, device=self.device)
            self._redraw_start_times()

    def _start_collecting(self):
        """suspended, not refused: evaluation and library_sweep() collect nothing and leave the tables alone"""
        return not self._is_evaluating and not self._start_suspended

    def _start_sampling_live(self):
        return self._start["sampling"] and self._start_collecting()

    def _point_start_time(self):
        """io.ovr_start_time: the buffer while start sampling is live, NULL while it is suspended; injected start times (set_injected_draws) win"""
        if self._start_time is None or self._overrides.get("ovr_start_time") is not None:
            return
        p = self._start_time.data_ptr() if self._start_sampling_live() else None
        if self._io.ovr_start_time != p:
            self._io.ovr_start_time = p
            self._io_epoch += 1

    def _step_counter_ptr(self):
        return self.globals[K["PBHC_G_STEP_COUNTER"]:].data_ptr()

    def _redraw_start_times(self):
        """a fresh start time for EVERY env from the current tables; salt = the count of these calls (>= 1: the per-step launch uses 0, so a
        redraw between two steps never repeats a per-step key)"""
        if self._start_time is None or not self._start_sampling_live():
            return
        self._start_redraws += 1
        self._motion_lib.draw_start_times_device(self._start_time, self._seed, self._step_counter_ptr(), self._start_redraws)

    def _launch_start_sampling(self, stream):
        if not self._start_collecting():
            return
        ml = self._motion_lib
        M, Kb = ml._num_unique_motions, self._start["bins"]
        _lib.check(self._lib.pbhc_start_stats(self.reset_buf.data_ptr(), self.time_out_buf.data_ptr(), self.end_time_ratio_buf.data_ptr(),
                                              self.last_episode_length_buf.data_ptr(), ml.slot_clip.data_ptr(), ml._motion_lengths.data_ptr(),
                                              float(self.dt), self.num_envs, M, Kb, self._start_window.data_ptr(), stream), "pbhc_start_stats")
        if self._start_time is not None:             # the envs that just reset used their draw: the next one (salt 0, keyed by the new counter)
            ml.draw_start_times_device(self._start_time, self._seed, self._step_counter_ptr(), 0, reset_buf=self.reset_buf, stream=stream)

    def _require_start_statistics(self, what):
        if self._start_window is None:
            raise _lib.PbhcError(f"{what}: env.config.start_statistics (or start_sampling.enable) is not set")

    def start_statistics(self):
        """The episodes that ended in step() since the window was last cleared or folded, per unique clip and phase bin, as device tensors
        [M,K]: `visits` (int64: episodes that passed through the bin), `failures` (int64: episodes that ended in it without a time-out),
        `visits_history`, `failures_history` (float32: the decayed sums of the folds) and `prob` (float32: the start-bin law in force).
        No host synchronisation."""
        self._require_start_statistics("start_statistics")
        self.wait_finalize()
        w, ml = self._start_window, self._motion_lib
        return dict(visits=torch.cumsum(w[:, :, 0], dim=1), failures=w[:, :, 1].clone(), visits_history=ml._start_visits.clone(),
                    failures_history=ml._start_failures.clone(), prob=ml._start_prob.clone())

    def clear_start_statistics(self):
        self._require_start_statistics("clear_start_statistics")
        self.wait_finalize()
        self._start_window.zero_()

    def update_start_sampling(self):
        """The fold: the window into the motion library's start-sampling tables (`_start_visits`, `_start_failures`, `_start_prob`,
        `_start_cdf`) with the configured decay / prior_episodes / uniform_floor / look-ahead, the window cleared, then — start_sampling.enable —
        a fresh start time for every env.  Data parallel: the window is first summed over the ranks (one exact int64 all-reduce), so every
        rank holds the same law.  The rollout driver calls it every update_every_rollouts rollouts; public, so that a user can fold at
        their own cadence.  Suspended (evaluation, library_sweep): nothing happens, -> False."""
        self._require_start_statistics("update_start_sampling")
        if not self._start_collecting():
            return False
        self.wait_finalize()
        group = getattr(self, "_stat_group", None)
        if pdist.active(group):
            pdist.all_reduce(self._start_window, group=group)
        c = self._start
        self._motion_lib.update_start_sampling_device(self._start_window, c["decay"], c["prior_episodes"], c["uniform_floor"], c["lookahead_bins"],
                                                      c["lookahead_decay"])
        self._redraw_start_times()
        return True

    # ---- library evaluation: every unique clip once from motion time 0, scored on the device (csrc/pbhc_clip_track.hip) ----
    def _library_sweep_refusal(self):
        """why library_sweep() cannot run now, or None — host-side state only, checked before anything is launched"""
        if getattr(self, "_stat_mode", None) is not None:
            return "a data-parallel statistics group is active (every rank would sweep the whole library)"
        if getattr(self, "_rec", None) is not None:
            return "the evaluation recorder is on (env.config.save_motion): it records env 0's clip, not a library"
        if self.config.get("enforce_randomize_motion_start_eval", False):
            return "env.config.enforce_randomize_motion_start_eval is set: the sweep plays every clip from motion time 0"
        if torch.cuda.is_current_stream_capturing():
            return "called inside a stream capture (the sweep reads the device once per sync_every steps)"
        return None

    def library_sweep(self, act, max_steps=None, sync_every=32, before_wave=None):
        """Play every unique clip of the motion library once from motion time 0 under `act` (obs_dict -> actions [N,D]) and score it on its
        FIRST episode: ceil(M / N) waves of N clips, wave w = clips w N .. w N + N - 1 on envs 0 .. N - 1 (`load_motions(random_sample=False,
        start_idx=w N)`; the idle envs of the last wave wrap around to a valid clip and are not scored).  Per wave: `before_wave(w, clip_ids)`
        (clip_ids [N] int64 on the device, -1 = idle; a ReplaySimStub user installs the wave's replay window there), a reset of every env,
        one step with zero actions (as reset_all(), counted), then act -> step until every clip's episode has ended — looked at once per
        `sync_every` steps, the only host reads — or `max_steps` (default: ceil(longest clip of the wave / dt) + 8) have run.  After every
        step two launches on the stepping stream: k_clip_stats into the sweep's OWN [M,4] episode window and k_clip_track, which scores the
        frame of every clip still in its first episode and retires the clips whose episode just ended.  The frame that ends an episode
        is not scored (its post-step state is the next episode's).  Eager, one stream: the finalize stream is detached for the duration,
        the periodic motion resample of step() is suspended, the training window (`_clip_window`) and the sampling hooks are not touched;
        afterwards the slot -> clip table is what it was and every env is reset.  Calls set_is_evaluating().
        -> dict of device tensors [M]: episodes (0/1), failures, success (bool: the episode ended by a time-out), end_time_ratio,
        episode_length, frames, E_gmpbpe, E_mpbpe (m), E_mpjpe (rad) (float64 means over the scored frames as pbhc_amd.eval.metrics
        eval_accuracy defines them per frame, NaN without a frame), and host scalars from ONE copy at the end: success_rate (of all M
        clips), the three errors averaged over the clips with frames, unfinished (clip ids still running at the cap), waves, steps."""
        why = self._library_sweep_refusal()
        if why is not None:
            raise _lib.PbhcError("library_sweep: " + why)
        ml, N, dev = self._motion_lib, self.num_envs, self.device
        M = ml._num_unique_motions
        sync_every = max(1, int(sync_every))
        fs = self._finalize_stream
        self.set_finalize_stream(None)                       # (waits for the last step's reduction first)
        interval = getattr(self, "resample_time_interval", None)
        if interval is not None:
            self.resample_time_interval = float("inf")       # step(): counter % inf is never 0
        window, self._clip_window = self._clip_window, None   # step() does not collect the sweep's episodes into the training window
        self._start_suspended = True                         # nor into the start-time window; the step draws its own start times
        self._point_start_time()
        slot_before = ml.slot_clip.clone()
        crops_before = ml.crop_starts.clone() if ml.max_len > 0 else None
        self.set_is_evaluating()
        episodes = torch.zeros(M, 4, dtype=torch.int64, device=dev)
        track = torch.zeros(M, 4, dtype=torch.int64, device=dev)
        eval_clip = torch.empty(N, dtype=torch.int64, device=dev)
        zero_act = torch.zeros(N, self.dim_actions, device=dev)
        waves, steps, unfinished = -(-M // N), 0, []
        s, lib = self.simulator, self._lib
        try:
            for w in range(waves):
                ml.load_motions(random_sample=False, start_idx=w * N, max_len=self.max_len)
                ids = torch.arange(N, device=dev) + w * N
                eval_clip.copy_(torch.where(ids < M, ids, torch.full_like(ids, -1)))
                if before_wave is not None:
                    before_wave(w, eval_clip.clone())
                self._reset_all_state()
                cap = int(max_steps) if max_steps is not None else int(np.ceil(float(self.motion_len[:min(N, M - w * N)].max()) / self.dt)) + 8
                obs = None
                for k in range(cap):
                    obs = self.step({"actions": zero_act if k == 0 else act(obs)})[0]
                    steps += 1
                    st = _lib.current_stream()
                    _lib.check(lib.pbhc_clip_stats(self.reset_buf.data_ptr(), self.time_out_buf.data_ptr(), self.end_time_ratio_buf.data_ptr(),
                                                   self.last_episode_length_buf.data_ptr(), eval_clip.data_ptr(), N, M, episodes.data_ptr(), st),
                               "pbhc_clip_stats")
                    _lib.check(lib.pbhc_clip_track(C.byref(s._csk), C.byref(ml.table), s.robot_root_states.data_ptr(), s.dof_state.data_ptr(),
                                                   self._ref_time.data_ptr(), self.env_origins.data_ptr(), self._slot_clip.data_ptr(),
                                                   self.reset_buf.data_ptr(), eval_clip.data_ptr(), eval_clip.data_ptr(), N, M, track.data_ptr(), st),
                               "pbhc_clip_track")
                    if (k + 1) % sync_every == 0 and not bool((eval_clip >= 0).any()):
                        break
                else:
                    unfinished += eval_clip[eval_clip >= 0].tolist()
        finally:
            ml.slot_clip.copy_(slot_before)
            if crops_before is not None:
                ml._build_slot_crops(crops_before)
            self._reset_all_state()
            self._clip_window = window
            self._start_suspended = False
            self._point_start_time()                         # (back only if the env is no longer evaluating)
            if interval is not None:
                self.resample_time_interval = interval
            self.set_finalize_stream(fs)
        e = episodes[:, 0]
        n = e.clamp(min=1).double()
        frames = track[:, 0]
        nan = torch.full((M,), float("nan"), dtype=torch.float64, device=dev)
        err = [torch.where(frames > 0, track[:, k].double() / 1048576.0 / frames.clamp(min=1).double(), nan) for k in (1, 2, 3)]
        out = dict(episodes=e, failures=episodes[:, 1], success=(e > 0) & (episodes[:, 1] == 0), end_time_ratio=episodes[:, 2].double() / 16777216.0 / n,
                   episode_length=episodes[:, 3].double() / n, frames=frames, E_gmpbpe=err[0], E_mpbpe=err[1], E_mpjpe=err[2])
        scored = (frames > 0).double()
        host = torch.stack([out["success"].double().sum() / M] + [torch.nan_to_num(x).sum() / scored.sum() for x in err]).cpu().tolist()
        out.update(success_rate=host[0], E_gmpbpe_mean=host[1], E_mpbpe_mean=host[2], E_mpjpe_mean=host[3], unfinished=unfinished, waves=waves, steps=steps)
        return out

    # ---- exact resume (DESIGN.md §8 "Exact resume") -------------------------------------------
    _STATE_TENSORS = ("globals", "actions", "last_actions", "actions_after_delay", "action_queue", "action_delay_idx", "last_dof_pos", "last_dof_vel",
                      "torques", "feet_air_time", "contacts", "contacts_filt", "last_contacts", "last_contacts_filt", "_kp_scale", "_kd_scale",
                      "_rfi_lim_scale", "_rao_scale", "default_dof_pos", "motion_start_times", "motion_len", "end_time_ratio_buf", "_episode_sums",
                      "_episode_rew_out", "_hist", "_episode_length_buf", "last_episode_length_buf", "reset_buf", "time_out_buf", "rew_buf",
                      "_ref_time", "_ou_state", "_start_time", "_start_window", "_clip_window")
    _STATE_HOST = ("common_step_counter", "_clip_draws", "_start_redraws")

    def _state_tensors(self):
        return {k: getattr(self, k) for k in self._STATE_TENSORS}

    def config_fingerprint(self):
        """the env's resolved config as text without addresses (utils/resume.py) + the motion table's clip count and frame counts: checked,
        not restored, by load_state_dict — with `_seed`, the step's Philox key, among its members"""
        ml = self._motion_lib
        return resume.config_fingerprint(self._c, ml._num_unique_motions, ml.clip_frame_counts())

    def _state_dict_refusal(self):
        """why the env's state cannot be saved now, or None — host-side state only"""
        if getattr(self, "_rec", None) is not None and not self._rec_dumped:
            return "an evaluation recording is running (env.config.save_motion): its buffers and counters are not part of the state"
        if self._start_suspended:
            return "library_sweep() is running: the slot -> clip table and every env are the sweep's, not the training run's"
        if torch.cuda.is_current_stream_capturing():
            return "called inside a stream capture"
        return None

    def state_dict(self):
        """Everything that decides how this env goes on, as copies: the `_STATE_TENSORS`, the host counters, the re-draw schedule, the
        generator of ranks > 0, the simulator's and the motion library's state.  Waits for the last step's reduction; draws from no
        generator, launches nothing that writes state and leaves every captured graph valid."""
        why = self._state_dict_refusal()
        if why is not None:
            raise _lib.PbhcError("state_dict: " + why)
        self.wait_finalize()
        self._flush_statistics()
        sd = resume.snapshot(self._state_tensors())
        sd.update({k: int(getattr(self, k)) for k in self._STATE_HOST})
        sd.update(version=resume.STATE_VERSION, num_envs=int(self.num_envs), seed=int(self._seed), fingerprint=self.config_fingerprint(),
                  reinit_counter=float(self._reinit.counter), is_evaluating=bool(self._is_evaluating),
                  gen=None if self._gen is None else rng_state.pack_torch(self._gen.get_state()),
                  simulator=self.simulator.state_dict(), motion_lib=self._motion_lib.state_dict())
        return sd

    def check_state_dict(self, sd):
        """everything `load_state_dict` would refuse, without writing anything: another version, num_envs, Philox key or config, a tensor
        of another shape, a replay cursor outside the current window"""
        what = f"{type(self).__name__}.load_state_dict"
        resume.check_version(sd, what)
        resume.check_equal(what, "num_envs", int(sd["num_envs"]), int(self.num_envs))
        resume.check_equal(what, "the env's Philox key `_seed` (seed torch with the saving run's config.seed before building the env)",
                           int(sd["seed"]), int(self._seed))
        resume.check_fingerprint(what, sd["fingerprint"], self.config_fingerprint())
        resume.check_tensors(what, sd, self._state_tensors())
        if (sd["gen"] is None) != (self._gen is None):
            raise _lib.PbhcError(f"{what}: the env's host generator differs: the saved state has {'none' if sd['gen'] is None else 'one'}, this "
                                 f"run has {'none' if self._gen is None else 'one'} (another rank?)")
        self.simulator.check_state_dict(sd["simulator"])
        self._motion_lib.check_state_dict(sd["motion_lib"])

    def load_state_dict(self, sd):
        """Restore what `state_dict()` saved, every tensor in place (the step's io struct, the riders and the captured graphs hold the
        addresses).  The caller has built this env as the saving run did — the same config, torch seeded the same way — and has set the
        replay window the saving run had; a mismatch raises PbhcError naming what differs and both values, before anything is written."""
        why = self._state_dict_refusal()
        if why is not None:
            raise _lib.PbhcError("load_state_dict: " + why)
        self.check_state_dict(sd)
        self.wait_finalize()
        self._flush_statistics()
        resume.restore(sd, self._state_tensors())
        for k in self._STATE_HOST:
            setattr(self, k, int(sd[k]))
        self._reinit.counter = float(sd["reinit_counter"])
        self.is_evaluating = bool(sd["is_evaluating"])
        if self._gen is not None:
            self._gen.set_state(rng_state.unpack_torch(sd["gen"]))
        self.simulator.load_state_dict(sd["simulator"])
        self._motion_lib.load_state_dict(sd["motion_lib"])
        self.curr_motion_ids = self._motion_lib.slot_clip
        self._ref_bodies = None                      # the lazy members of a step this process never ran
        self.extras.invalidate()
        self.extras["episode"] = EpisodeExtras(self)

    # ---- logging: device-side means, read back on demand (no per-step sync) ----------------
    def read_log(self):
        self.wait_finalize()
        self._flush_statistics()
        g = self.globals.cpu().numpy()
        L0 = K["PBHC_G_LOG"]
        out = {
            "upper_body_diff_norm": g[L0 + K["PBHC_L_UPPER_BODY_DIFF_NORM"]], "lower_body_diff_norm": g[L0 + K["PBHC_L_LOWER_BODY_DIFF_NORM"]],
            "vr_3point_diff_norm": g[L0 + K["PBHC_L_VR_3POINT_DIFF_NORM"]], "joint_pos_diff_norm": g[L0 + K["PBHC_L_JOINT_POS_DIFF_NORM"]],
            "action_clip_frac": g[L0 + K["PBHC_L_ACTION_CLIP_FRAC"]], "terminate_by_gravity": g[L0 + K["PBHC_L_TERM_GRAVITY"]],
            "terminate_by_motion_far": g[L0 + K["PBHC_L_TERM_MOTION_FAR"]], "terminate_by_time_out": g[L0 + K["PBHC_L_TERM_TIME_OUT"]],
            "terminate_by_motion_end": g[L0 + K["PBHC_L_TERM_MOTION_END"]], "end_time_ratio": g[L0 + K["PBHC_L_END_TIME_RATIO"]],
            "end_time_ratio_std": g[L0 + K["PBHC_L_END_TIME_RATIO_STD"]], "penalty_scale": g[K["PBHC_G_PENALTY_SCALE"]], **({"current_noise_curriculum_value": g[K["PBHC_G_NOISE_CURRICULUM"]]} if self._c.noise_curriculum else {}),
            "average_episode_length": g[K["PBHC_G_AVG_EP_LEN"]], "terminate_when_motion_far_threshold": g[K["PBHC_G_MOTION_FAR_THR"]],
            "reward_mean": g[L0 + K["PBHC_L_REW_MEAN"]],
        }
        for flag, slot, name in ((self._c.soft_pos_curriculum, "PBHC_G_SOFT_POS_VAL", "soft_dof_pos"), (self._c.soft_vel_curriculum, "PBHC_G_SOFT_VEL_VAL", "soft_dof_vel"),
                                 (self._c.soft_tau_curriculum, "PBHC_G_SOFT_TAU_VAL", "soft_torque")):
            if flag:                                      # legged_robot_base.py:753-758
                out[name + "_curriculum_value"] = g[K[slot]]
        if self._c.terminate_by_contact:
            out["terminate_by_contact"] = g[L0 + K["PBHC_L_TERM_CONTACT"]]
        if self._c.terminate_by_low_height:
            out["terminate_by_low_height"] = g[L0 + K["PBHC_L_TERM_LOW_HEIGHT"]]
        for flag, key, name in ((self._c.terminate_close_pos, "PBHC_L_TERM_DOF_POS_LIMIT", "dof_pos_limit"), (self._c.terminate_close_vel, "PBHC_L_TERM_DOF_VEL_LIMIT", "dof_vel_limit"),
                                (self._c.terminate_close_tau, "PBHC_L_TERM_TORQUE_LIMIT", "torque_limit")):
            if flag:
                out["terminate_by_" + name] = g[L0 + K[key]]
        if self._c.terminate_when_dof_far:                # motion_tracking.py:346-349 (the threshold: when its curriculum is enabled)
            out["terminate_by_dof_far"] = g[L0 + K["PBHC_L_TERM_DOF_FAR"]]
            if self._c.dof_far_curriculum:
                out["terminate_when_dof_far_threshold"] = g[L0 + K["PBHC_L_DOF_FAR_THR"]]
        for i, k in enumerate(env_config.SIGMA_KEYS):
            out["adp_sigma_" + k] = g[K["PBHC_G_SIGMA"] + i]
            out["error_ema_" + k] = g[K["PBHC_G_EMA"] + i]
        if self._start_window is not None:                # one device -> host copy: the window's failures per bin and max(_start_prob)
            f = self._start_window[:, :, 1].sum(dim=0).double()
            bins = torch.arange(f.shape[0], dtype=torch.float64, device=self.device)
            t = torch.stack([f.sum(), (f * bins).sum(), self._motion_lib._start_prob.max().double()]).cpu().numpy()
            out["start_sampling_concentration"] = f.shape[0] * t[2]
            out["start_failure_bin_mean"] = t[1] / t[0] if t[0] > 0 else 0.0
        if self._clip_window is not None:                 # one device -> host copy: the window's two count columns and max(_sampling_prob)
            w = self._clip_window
            t = torch.stack([w[:, 0].sum().double(), w[:, 1].sum().double(), self._motion_lib._sampling_prob.max().double()]).cpu().numpy()
            out["clip_episodes"] = t[0]
            out["clip_success_rate"] = 1.0 - t[1] / t[0] if t[0] > 0 else 0.0
            out["clip_sampling_concentration"] = w.shape[0] * t[2]
        self.log_dict.update({k: torch.tensor(float(v)) for k, v in out.items()})
        return out


def _quat_mul_xyzw(a, b):
    """Hamilton product of [N,4] xyzw quaternions: the 9-multiplication form of csrc/pbhc_math.h quat_mul (the kernel's reset path)"""
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    ww = (az + ax) * (bx + by)
    yy = (aw - ay) * (bw + bz)
    zz = (aw + ay) * (bw - bz)
    xx = ww + yy + zz
    qq = 0.5 * (xx + (az - ax) * (bx - by))
    return torch.stack([qq - xx + (ax + aw) * (bx + bw), qq - yy + (aw - ax) * (by + bz), qq - zz + (az + ay) * (bw - bx),
                        qq - ww + (az - ay) * (by - bz)], dim=-1)


def _padded_rows(n, dim, device, dtype=torch.float32):
    """[n, dim] view of an [n, ceil32(dim)] buffer: every row starts on a 128-byte line."""
    return torch.zeros(n, _lib.padded_width(dim), dtype=dtype, device=device)[:, :dim]


class _TopView:
    """env.config holds aliases of the top-level nodes; present them under the top-level names the
    config builder uses (cfg.env.config, cfg.robot, cfg.obs, ...)."""

    def __init__(self, env_cfg):
        self.env = _NS(config=env_cfg)
        self.robot, self.obs, self.rewards = env_cfg.robot, env_cfg.obs, env_cfg.rewards
        self.domain_rand, self.terrain, self.simulator = env_cfg.domain_rand, env_cfg.terrain, env_cfg.simulator


class _NS:
    def __init__(self, **kw):
        self.__dict__.update(kw)
