"""Re-home a live env into arenas (tests/arena.py): every caller-owned buffer the per-step launches name — `PbhcStepIO` of `k_env_step`,
`k_dof_far_any`, `k_env_finalize`, `k_record_motion` and the closed-loop simulators' kernels — moves, contents preserved, into a buffer with
poisoned margins and poisoned row padding, the env's attributes are re-pointed at the views and `env._build_io()` binds the new addresses.
tests/test_gpu_step_memory.py then runs the oracle comparisons the suite already has on such an env and calls `assert_intact` after every step.

Poison.  f32 buffers: the payload NaN of tests/arena.py, compared bit for bit, for inputs, outputs and read+write state alike.  Integer
buffers hold values that are HARMLESS AS DATA, because the kernels turn them into addresses: `motion_ids` margins name the library's last
clip, `action_delay_idx` / `ovr_delay` margins the last slot of the action queue, `frame_cursor` margins frame 0, the episode counters and
`reset_buf` margins `1 << 20`.  A leaked read then shows as a mismatch against the oracle and can never leave a table — except for `motion_ids`
in a single-clip library, where the only valid id is the one every env uses: there the margin is harmless but a leaked read of it changes
nothing; the multi-clip general-tracking case is where such a read would show.  `time_out_buf` (u8)
margins hold 0xA5, which no store of a bool produces.

Pitches.  Observation rows are built at the smallest pitch the entry accepts — `PbhcEnvConfig.groups[g].pitch`, which is the group's
dimension (dense rows; `env_step_check` refuses less) — plus `obs_pitch_extra`; history rows at `hist_dim` for the generic kernel and at
`hist_dim` rounded up to 4 floats, 16-byte aligned, when a specialised kernel is attached (its rule in `pbhc_env_step_launch`), plus
`hist_pitch_extra`.  `offset` (floats) moves every f32 operand whose contract is 4-byte alignment off its 16-byte boundary; the history rows
of a specialised kernel stay where their contract puts them.

Not re-homed (NOT_REHOMED holds the reasons per `PbhcStepIO` field): `env.globals` and the library's own `d_partials` / `d_cfg` are bound at
`pbhc_env_create`; re-homing them means re-creating the env, and they are no field of `PbhcStepIO`."""
import ctypes as C

import torch

from tests.arena import POISON, arena

# PbhcStepIO pointer fields this module never puts into an arena, with the reason.  tests/test_gpu_step_memory.py holds
# REHOMED | NOT_REHOMED against the struct's fields: a field added later fails there until someone decides.
NOT_REHOMED = {
    "totals_out": "non-NULL only in a data-parallel run (enable_global_statistics('step') with a process group): a buffer of k_env_finalize's, "
                  "PBHC_NUM_TOTALS doubles, not of the fused step's per-env paths; tests/test_gpu_dist.py owns that mode",
}
# field -> (owner: "env" | "sim", attribute) of the plain [N, ...] buffers _build_io binds
_PLAIN = {
    "actions": ("env", "actions"), "last_actions": ("env", "last_actions"), "actions_after_delay": ("env", "actions_after_delay"),
    "action_queue": ("env", "action_queue"), "last_dof_pos": ("env", "last_dof_pos"), "last_dof_vel": ("env", "last_dof_vel"),
    "torques": ("env", "torques"), "feet_air_time": ("env", "feet_air_time"), "contacts": ("env", "contacts"),
    "contacts_filt": ("env", "contacts_filt"), "last_contacts": ("env", "last_contacts"), "last_contacts_filt": ("env", "last_contacts_filt"),
    "kp_scale": ("env", "_kp_scale"), "kd_scale": ("env", "_kd_scale"), "rfi_lim_scale": ("env", "_rfi_lim_scale"), "rao_scale": ("env", "_rao_scale"),
    "default_dof_pos": ("env", "default_dof_pos"), "motion_start_times": ("env", "motion_start_times"), "motion_len": ("env", "motion_len"),
    "end_time_ratio_buf": ("env", "end_time_ratio_buf"), "ou_state": ("env", "_ou_state"), "rew_buf": ("env", "rew_buf"),
    "ref_time_out": ("env", "_ref_time"), "episode_rew_out": ("env", "_episode_rew_out"),
    "episode_length_buf": ("env", "_episode_length_buf"), "last_episode_length_buf": ("env", "last_episode_length_buf"),
    "reset_buf": ("env", "reset_buf"), "action_delay_idx": ("env", "action_delay_idx"), "time_out_buf": ("env", "time_out_buf"),
    "dr_base_com": ("sim", "_base_com_bias"), "dr_link_mass": ("sim", "_link_mass_scale"), "dr_friction": ("sim", "friction_coeffs"),
    "dr_base_mass": ("sim", "_base_mass_scale"),
}
_SPECIAL = ("actions_in", "frame_root", "frame_dof_pos", "frame_dof_vel", "frame_contact", "frame_cursor", "root_states", "dof_state",
            "episode_sums", "hist", "motion_ids", "env_origins", "obs", "rigid_body_state", "contact_forces", "ref_body_pos_extend",
            "ref_body_rot_extend")
# set_injected_draws: keyword -> PbhcStepIO field (held against env._overrides, the env's own table, at every call)
_DRAWS = dict(u_rfi="u_rfi", start_time="ovr_start_time", kp="ovr_kp", kd="ovr_kd", rfi_lim="ovr_rfi_lim", rao="ovr_rao", delay="ovr_delay",
              dof_pos_bias="ovr_dof_pos_bias", gate_u="ovr_gate_u", reset_root="ovr_reset_root", reset_dof_pos="ovr_reset_dof_pos",
              reset_dof_vel="ovr_reset_dof_vel", ou_step="ovr_ou_step", ou_reset="ovr_ou_reset", ps_kp="ovr_ps_kp", ps_kd="ovr_ps_kd",
              ps_rao="ovr_ps_rao", ps_tau="ovr_ps_tau")
REHOMED = set(_PLAIN) | set(_SPECIAL) | set(_DRAWS.values())
EAGER = ("rigid_body_state", "contact_forces", "ref_body_pos_extend", "ref_body_rot_extend")


def pointer_fields(struct):
    """the names of a ctypes Structure's pointer fields (arrays of pointers included)"""
    return [n for n, t in struct._fields_ if t is C.c_void_p or getattr(t, "_type_", None) is C.c_void_p]


def int_fill(env, field):
    """the margin value of an integer buffer: harmless as data (see the module docstring)"""
    if field in ("episode_length_buf", "last_episode_length_buf", "reset_buf", "rec.terminate"):
        return 1 << 20
    if field in ("action_delay_idx", "ovr_delay"):
        return int(env._c.queue_len) - 1
    if field == "motion_ids":
        return int(env._motion_lib.table.num_motions) - 1
    if field == "frame_cursor":
        return 0
    if field == "time_out_buf":
        return 0xA5
    raise KeyError(field)


def put(env, registry, field, t, *, pitch=None, offset=0):
    """tensor `t` ([n] or [rows, ...]) into an arena registered as `field` -> the view inside the arena, in t's shape (2-D when pitched)"""
    rows, cols = (1, t.numel()) if t.dim() == 1 else (t.shape[0], t.numel() // t.shape[0])
    fill = POISON if t.dtype.is_floating_point else int_fill(env, field)
    a = arena(rows, cols, pitch, offset if t.dtype == torch.float32 else 0, fill, t.reshape(rows, cols), env.device, t.dtype, field)
    registry[field] = a
    out = a.view if (pitch or cols) != cols else a.view.reshape(t.shape)
    assert out.data_ptr() == a.ptr()
    return out


def rehome(env, *, obs_pitch_extra=0, hist_pitch_extra=0, eager=False, offset=0):
    """-> {PbhcStepIO field (or "obs[<group>]", a simulator's extra buffer): Arena}; see the module docstring"""
    env.wait_finalize()
    torch.cuda.synchronize()
    reg, s, N, D, L = {}, env.simulator, env.num_envs, env.num_dof, env.layout
    mv = lambda field, t, **k: put(env, reg, field, t, offset=offset, **k)
    # ---- the simulator surface
    s.robot_root_states = s.all_root_states = mv("root_states", s.robot_root_states)
    s.base_quat = s.robot_root_states[..., 3:7]
    s.dof_state = mv("dof_state", s.dof_state.view(N, D * 2)).view(N * D, 2)
    s.dof_pos, s.dof_vel = s.dof_state.view(N, D, 2)[..., 0], s.dof_state.view(N, D, 2)[..., 1]
    env.env_origins = s.env_origins = mv("env_origins", env.env_origins)
    # ---- the plain buffers (an empty one — no randomised link masses — has nothing to move: the kernel reads dr_base_com in its place)
    for field, (owner, attr) in _PLAIN.items():
        obj = env if owner == "env" else s
        t = getattr(obj, attr)
        if t.numel():
            setattr(obj, attr, mv(field, t))
    env._episode_sums = mv("episode_sums", env._episode_sums)
    env.episode_sums = {name: env._episode_sums[:, i] for i, name in enumerate(L.sum_names)}
    if env._start_time is not None:
        env._start_time = mv("start_time_buffer", env._start_time)         # (bound as ovr_start_time while no start time is injected)
    # ---- pitched rows: the history (16 bytes per lane in a specialised build: its contract, not an offset) and the observation groups
    wide = env.is_specialised
    hp = ((L.hist_dim + 3) & ~3 if wide else L.hist_dim) + hist_pitch_extra
    env._hist = put(env, reg, "hist", env._hist, pitch=hp, offset=0 if wide else offset)
    for g in L.group_names[:-1]:
        env._own_obs[g] = put(env, reg, f"obs[{g}]", env._own_obs[g], pitch=L.group_dims[g] + obs_pitch_extra, offset=offset)
    env.obs_buf_dict = dict(env._own_obs)
    # ---- the replay window and its cursor (a closed-loop simulator owns a one-frame window and refuses set_replay)
    s.ensure_replay()
    frame = int(s.frame_cursor.item())
    s.frame_cursor = mv("frame_cursor", s.frame_cursor)
    r = {k: mv("frame_" + k, v.reshape(v.shape[0], -1)).reshape(v.shape) for k, v in s.replay.items()}
    if hasattr(s, "advance"):
        s.replay = r
        s.replay_version += 1
    else:
        host = s._host_frame
        s.set_replay(r["root"], r["dof_pos"], r["dof_vel"], r["contact"], start_frame=frame)
        s._host_frame = host if host < 0 else s._host_frame
    env._build_io()
    env._slot_clip = mv("motion_ids", env._slot_clip)
    env._io.motion_ids = env._slot_clip.data_ptr()
    if eager:
        env.set_eager_outputs(True)
        for k in EAGER:
            env._eager[k] = mv(k, env._eager[k])
            setattr(env._io, k, env._eager[k].data_ptr())
    # ---- a closed-loop simulator's own tables and debug outputs
    p = getattr(s, "_params", None)
    if p is not None:
        for attr, field in (("tau0", "tau0"), ("root_acc", "root_acc"), ("_points_dev", "points")):
            t = getattr(s, attr, None)
            if t is not None:
                setattr(s, attr, mv("sim." + field, t))
                setattr(p, field, getattr(s, attr).data_ptr())
    _wrap(env, reg, offset)
    torch.cuda.synchronize()
    return reg


def _wrap(env, reg, offset):
    """the per-step operands go through arenas too: the tensors of set_injected_draws and the actions handed to step()"""
    inject, step = env.set_injected_draws, env.step

    def set_injected_draws(**kw):
        for field in _DRAWS.values():
            reg.pop(field, None)
        moved = {k: (None if v is None else put(env, reg, _DRAWS[k], v.to(env.device), offset=offset)) for k, v in kw.items()}
        inject(**moved)
        for k, v in moved.items():
            assert env._overrides[_DRAWS[k]] is v, k

    def step_in_arena(actor_state):
        a = actor_state["actions"].to(env.device, torch.float32)
        return step(dict(actor_state, actions=put(env, reg, "actions_in", a, offset=offset)))

    env.set_injected_draws, env.step = set_injected_draws, step_in_arena


def bound(env, registry):
    """the PbhcStepIO fields that are non-NULL right now -> each must be the arena's operand (nothing re-pointed the io behind the test)"""
    io, names = env._io, []
    for f in pointer_fields(type(io)):
        if f == "obs":
            for i, g in enumerate(env.layout.group_names):
                key = "hist" if i == len(env.layout.group_names) - 1 else f"obs[{g}]"
                assert io.obs[i] == registry[key].ptr(), key
            continue
        v = getattr(io, f)
        if v is None or f in NOT_REHOMED:
            continue
        if f == "dr_link_mass" and not env.simulator._link_mass_scale.numel():
            continue
        homes = [registry[k].ptr() for k in ((f, "start_time_buffer") if f == "ovr_start_time" else (f,)) if k in registry]
        assert v in homes, f"PbhcStepIO.{f} is bound to memory outside the arenas"
        names.append(f)
    return names


def assert_intact(registry, declared=None):
    """every arena's surroundings still hold their fill, bit for bit.  `declared`: {name: logical width} other than the operand's own."""
    torch.cuda.synchronize()
    found = [d for d in (a.damage(cols=(declared or {}).get(name)) for name, a in registry.items()) if d is not None]
    assert not found, "stores outside an operand:\n  " + "\n  ".join(found)
