"""Everything launched once per control step — `k_env_step` (generic and specialised), `k_dof_far_any`, `k_env_finalize`, `k_record_motion`,
`pbhc_motion_state`, `pbhc_sim_fk` and the closed-loop simulators' kernels — pinned against what it does to memory AROUND its operands.
The values stay held by the oracles, traces and float64 models the suite already trusts, with their tolerances; what is new is that every
caller-owned operand sits in an arena (tests/arena.py, tests/step_arena.py): payload-NaN margins and row padding compared bit for bit,
integer margins that are harmless as data, observation and history rows at the smallest pitch the entry accepts and at that pitch + 4,
base pointers 0, 1, 2 and 3 floats behind a 16-byte boundary where the written contract (include/pbhc_hip.h) is 4-byte alignment, and
the smallest batch sizes at which a workgroup is ragged.  Every comparison also demands a FINITE result (tests/test_gpu_parity.py's
`close` lets a NaN pass: `nan > tol` is false), so poison that leaks into a result fails the case; `assert_intact` runs after every step.

Notes on the cases:
  * the optional buffers (OU process, parallel-serial DR, reset-state noise, dof-far pre-pass) are held to the REFERENCE'S TRACES by the
    drivers of tests/test_gpu_imu_noise_dr.py and tests/test_gpu_reset_options.py; a trace fixes its batch at 16 envs (its log means and
    the batch-global dof-far decision are statistics of those 16), so these cases run at N = 16: four full workgroups, no ragged one;
  * the recorder case starts its counter at 3 (the three dropped records behind it), so that 6 steps cover frames 0..2 AND three
    saturated steps; the header's rule is "value k writes frame k - 3, values >= T + 3 record nothing".
  * JointSpaceSim has no test-only export, so it runs through the env (N = 5: one ragged workgroup, and 33); the two exports that exist
    (`pbhc_debug_articulated_substeps`, `pbhc_debug_floating_substeps`) run at n = 1, CL_EPB + 1 = 9 and 33.

Measured on an MI355X: the worst `err / tol` (or `err / bound`) of a case over its steps and compared quantities, printed by every case as
`WORST`; the figures did not depend on the pitch, on the base offset or on the kernel (generic / specialised) in any case:
  a. motion-tracking step vs oracle, T = 4         N = 1  0.002    N = 5  0.010    N = 13  0.019    (offsets 1..3, device cursor: 0.010)
     eager outputs vs the lazy forms, N = 5        0.157 (rigid-body pose, bound 2e-6); contact forces and reference bodies bit-equal
     23-DoF student trace, actor_obs 877 columns at pitch 878 (generic kernel)      0.038; offset 0: padding column 877 written, as the
                                                   contract says, and nothing else; offset 1 (element-wise stores): all padding intact
  b. general-tracking step, 29-DoF teacher         N = 1  0.025    N = 5  0.054
  c. OU + parallel-serial (trace, N = 16)          0.063           reset noise + dof-far pre-pass (trace, N = 16)  0.064
     default_dof_pos N = 5  0.010                  redraw_all N = 5  0.010                        close-to-limit gates N = 37  0.039
  d. recorder N = 5, T = 3                         copies bit-equal; nothing stored once the counter is saturated; counter words 1.. stay 0
  e. pbhc_motion_state (on the table's last clip)  n = 1  0.009    n = 5  0.020    n = 37  0.051
     pbhc_sim_fk (stride 1 / 2)                    n = 1  0.024 / 0.025    n = 5  0.050 / 0.037    n = 37  0.047 / 0.057
  f. articulated sub-step                          n = 1  0.022    n = 9  0.103    n = 33  0.268
     floating sub-step (acceleration / forces)     n = 1  0.008 / 0.034    n = 9  0.038 / 0.059    n = 33  0.050 / 0.111
     FloatingBaseSim env N = 5  0.083              JointSpaceSim env N = 5  0.245, N = 33  0.396       (offsets 0..3 at N = 5: the same)
No entry stored outside its operands or let poison into a result.  Two things the header had left unsaid are now written there and held
here: the generic kernel's paired stores write the ONE float of row padding behind an observation row of odd dimension (even pitch, 8-byte
aligned base: test_the_float_behind_an_odd_row_is_the_only_padding_the_step_may_write), and the one thing the entries assumed without checking —
8-byte alignment of the int64 buffers and of the f64 totals — is now refused at `pbhc_env_step*`, `pbhc_record_motion`, `pbhc_motion_state` and the simulators'
step entries (test_misaligned_buffers_are_refused_before_the_launch and the ends of the recorder and JointSpaceSim cases).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import step_arena as SA
from tests.arena import MARGIN, POISON, POISON_BITS, Arena, arena

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class Worst:
    """wraps a driver module's `close`: demands a finite result and keeps the largest err / bound of the case"""

    def __init__(self, monkeypatch, *modules):
        import importlib

        self.ratio, self.what = 0.0, ""
        for name in modules:
            mod = importlib.import_module(name)
            monkeypatch.setattr(mod, "close", self._wrap(mod.close))

    def _wrap(self, close):
        from tests.test_gpu_parity import close_limit

        def checked(a, b, tol, what, rtol=None, hard=None, frac=0.0, tol_override=None):
            x = torch.as_tensor(a).detach().float().cpu()
            y = torch.as_tensor(b).detach().float().cpu()
            assert bool(torch.isfinite(x).all()), f"{what}: {int((~torch.isfinite(x)).sum())} non-finite element(s) — poison reached a result"
            lim = hard if hard is not None else close_limit(y, tol, what, rtol, tol_override)[1]       # the driver's own limit
            r = float(((x - y).abs() / torch.as_tensor(lim).clamp(min=1e-30)).max()) if x.numel() else 0.0
            if r > self.ratio:
                self.ratio, self.what = r, what
            return close(a, b, tol, what, rtol=rtol, hard=hard, frac=frac, tol_override=tol_override)

        return checked

    def report(self, case):
        print(f"WORST {case}: err/tol {self.ratio:.3f} ({self.what})")


def _hooks(state, **rehome):
    """prepare / after_step for the drivers: re-home the env, then check binding and arenas after every step"""
    def prepare(env):
        state["reg"] = SA.rehome(env, **rehome)
        state["env"] = env
        if state.get("pad_column"):                      # rows of odd dimension: column `dim` of the padding is the kernel's (see the test)
            dims = dict(env.layout.group_dims, hist=env.layout.hist_dim)
            state["declared"] = {("hist" if g == "hist" else f"obs[{g}]"): d + 1 for g, d in dims.items() if d & 1 and (g == "hist" or g in env._own_obs)}
        if state.get("cursor"):
            env.simulator.use_device_cursor()

    def after_step(env, k):
        state["bound"] = set(state.get("bound", ())) | set(SA.bound(env, state["reg"]))
        SA.assert_intact(state["reg"], state.get("declared"))
        if "each" in state:
            state["each"](env, k)

    return dict(prepare=prepare, after_step=after_step)


def _kernel(monkeypatch, kernel):
    monkeypatch.setenv("PBHC_SPECIALISE", "off" if kernel == "generic" else "jit")


# ---- a. the motion-tracking step against the oracle ------------------------------------------------------------------------------------
# N = 1: one partly filled workgroup (PBHC_EPB = 4 envs); 5: a full one plus one env; 13: the suite's ragged case.  The specialised build
# is keyed on the config, not on num_envs, so it runs the same sweep.
@pytest.mark.parametrize("extra", [0, 4])
@pytest.mark.parametrize("kernel", ["generic", "specialised"])
@pytest.mark.parametrize("N", [1, 5, 13])
def test_motion_tracking_step_in_arenas(N, kernel, extra, monkeypatch):
    from tests.test_gpu_parity import _env_step_vs_oracle

    _kernel(monkeypatch, kernel)
    w, st = Worst(monkeypatch, "tests.test_gpu_parity"), {}
    _env_step_vs_oracle(N, 4, **_hooks(st, obs_pitch_extra=extra, hist_pitch_extra=extra))
    assert st["env"].is_specialised == (kernel == "specialised")
    assert st["env"].simulator.replay_len == 4                     # exactly T frames: the last step read the last one
    w.report(f"a N={N} {kernel} pitch+{extra}")


@pytest.mark.parametrize("kernel", ["generic", "specialised"])
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_motion_tracking_step_at_4_byte_aligned_bases(offset, kernel, monkeypatch):
    """every f32 operand `offset` floats behind a 16-byte boundary (the specialised kernel's history rows keep their 16-byte contract)"""
    from tests.test_gpu_parity import _env_step_vs_oracle

    _kernel(monkeypatch, kernel)
    w, st = Worst(monkeypatch, "tests.test_gpu_parity"), {}
    _env_step_vs_oracle(5, 4, **_hooks(st, offset=offset))
    for name in ("torques", "obs[actor_obs]", "frame_contact", "u_rfi", "actions_in"):
        assert st["reg"][name].ptr() % 16 == 4 * offset, name
    w.report(f"a offset={offset} {kernel}")


@pytest.mark.parametrize("offset", [0, 1])
def test_the_float_behind_an_odd_row_is_the_only_padding_the_step_may_write(offset, monkeypatch):
    """The generic kernel stores observation elements in pairs when a row's pitch is even and its base 8-byte aligned; the second half of
    an odd row's last pair then lands in padding column `dim` (the contract in include/pbhc_hip.h grants exactly that float, and
    `_lib.padded_width` leaves room for it).  The 23-DoF student's actor_obs has 877 columns: at pitch 878 and offset 0 column 877 is
    written and declared, every other float of padding — and every row of even dimension, whose pitch is then odd: the element-wise path —
    stays poison; one float off the 8-byte boundary (offset 1) the element-wise path runs and ALL padding stays poison.  Values: the
    reset-noise trace of tests/test_gpu_reset_options.py."""
    import tests.test_gpu_reset_options as T

    _kernel(monkeypatch, "generic")
    w, st = Worst(monkeypatch, "tests.test_gpu_reset_options"), {"pad_column": offset == 0}
    T._trace("env_v2_student23_resetnoise", T.STUDENT, T.NOISE, general=True, **_hooks(st, obs_pitch_extra=1, hist_pitch_extra=1, offset=offset))
    dim = st["env"].layout.group_dims["actor_obs"]
    assert dim & 1 and st["reg"]["obs[actor_obs]"].view.stride(0) == dim + 1
    if offset == 0:
        assert st["declared"] == {"obs[actor_obs]": dim + 1}
        assert st["reg"]["obs[actor_obs]"].damage().startswith(f"obs[actor_obs]: in row padding at (row 0, column {dim})")
    w.report(f"a student23 generic pitch+1 offset={offset}")


def test_motion_tracking_step_reads_the_device_cursor_in_arenas(monkeypatch):
    """frame_index < 0: the kernel takes the frame from the i32 cursor (in an arena, frame 0 in its margins) and advances it"""
    from tests.test_gpu_parity import _env_step_vs_oracle

    w, st = Worst(monkeypatch, "tests.test_gpu_parity"), {"cursor": True}

    def each(env, k):
        assert env._io.frame_index < 0, k

    st["each"] = each
    _env_step_vs_oracle(5, 4, **_hooks(st))
    assert int(st["reg"]["frame_cursor"].view[0, 0]) == 0          # 4 steps through 4 frames: back at the start
    w.report("a device cursor N=5")


@pytest.mark.parametrize("kernel", ["generic", "specialised"])
def test_motion_tracking_step_eager_outputs_in_arenas(kernel, monkeypatch):
    """rigid_body_state, contact_forces and ref_body_*_extend stored by the step (non-NULL, in arenas) equal the lazy forms, as in
    test_lazy_simulator_surface_and_reference_bodies_equal_the_stored_ones"""
    import tests.test_gpu_parity as P
    from tests.test_gpu_parity import _env_step_vs_oracle

    _kernel(monkeypatch, kernel)
    w, st = Worst(monkeypatch, "tests.test_gpu_parity"), {}

    def each(env, k):
        e, s, close = env._eager, env.simulator, P.close
        for name in SA.EAGER:
            assert getattr(env._io, name) == st["reg"][name].ptr() and bool(torch.isfinite(e[name]).all()), name
        close(s._rigid_body_state[..., :7], e["rigid_body_state"][..., :7], 2e-6, f"step {k} lazy rigid-body pose", rtol=2e-6)
        close(s._rigid_body_state[..., 7:], e["rigid_body_state"][..., 7:], 1e-5, f"step {k} lazy rigid-body twist", rtol=1e-5)
        assert torch.equal(s.contact_forces, e["contact_forces"]), k
        assert torch.equal(env.extras["ref_body_pos_extend"], e["ref_body_pos_extend"]), k
        assert torch.equal(env.extras["ref_body_rot_extend"], e["ref_body_rot_extend"]), k

    st["each"] = each
    _env_step_vs_oracle(5, 4, **_hooks(st, eager=True))
    w.report(f"a eager N=5 {kernel}")


def test_a_one_column_overrun_is_seen(monkeypatch):
    """The check can see what it is for: after one ordinary step, `torques` declared one column narrower than it is must fail the check, by
    name and column — the kernel's own, legitimate store into column D - 1 is then a store into row padding."""
    from tests.test_gpu_parity import _env_step_vs_oracle

    st = {}
    _env_step_vs_oracle(5, 1, **_hooks(st))
    SA.assert_intact(st["reg"])
    D = st["env"].num_dof
    with pytest.raises(AssertionError, match=rf"torques: in row padding at \(row 0, column {D - 1}\)"):
        SA.assert_intact(st["reg"], declared={"torques": D - 1})
    dim = st["env"].layout.group_dims["actor_obs"]
    with pytest.raises(AssertionError, match=rf"obs\[actor_obs\]: in row padding at \(row 0, column {dim - 1}\)"):
        SA.assert_intact(st["reg"], declared={"obs[actor_obs]": dim - 1})


# ---- b. the general-tracking step (tracking_mode 1), 29-DoF teacher: D and Bx closest to the 32 lanes of an env ---------------------------
@pytest.mark.parametrize("kernel", ["generic", "specialised"])
@pytest.mark.parametrize("N", [1, 5])
def test_general_tracking_step_in_arenas(N, kernel, monkeypatch):
    from tests.test_gpu_parity_v2 import _multi_clip_vs_oracle

    _kernel(monkeypatch, kernel)
    w, st = Worst(monkeypatch, "tests.test_gpu_parity_v2", "tests.test_gpu_parity"), {}
    _multi_clip_vs_oracle(N, 4, 3, **_hooks(st, obs_pitch_extra=0 if N == 1 else 4, hist_pitch_extra=0 if N == 1 else 4, offset=0 if N == 1 else 3))
    assert st["env"].is_specialised == (kernel == "specialised") and "dr_base_mass" in st["bound"]
    w.report(f"b N={N} {kernel}")


# ---- c. the optional buffers ----------------------------------------------------------------------------------------------------------
def test_ou_process_and_parallel_serial_buffers_in_arenas(monkeypatch):
    """ou_state, ovr_ou_step / ovr_ou_reset, ovr_ps_kp / kd / rao / tau: the walk trace of tests/test_gpu_imu_noise_dr.py"""
    import tests.test_gpu_imu_noise_dr as T

    w, st = Worst(monkeypatch, "tests.test_gpu_imu_noise_dr"), {}
    ov = dict(T._names(T.WALK, T.ROOT2), **{"obs.noise_process": T.OU, "domain_rand.parallel_serial_pd": T.PS_PD, "domain_rand.parallel_serial_tau": T.PS_TAU})
    T._trace("env_v1_walk_imunoise", T.WALK, ov, general=False, **_hooks(st, obs_pitch_extra=4, hist_pitch_extra=4, offset=3))
    assert {"ou_state", "ovr_ou_step", "ovr_ou_reset", "ovr_ps_kp", "ovr_ps_kd", "ovr_ps_rao", "ovr_ps_tau"} <= st["bound"]
    w.report("c OU + parallel-serial (trace, N=16)")


def test_reset_noise_and_dof_far_prepass_in_arenas(monkeypatch):
    """ovr_reset_root / dof_pos / dof_vel and the k_dof_far_any pre-pass (frame_dof_pos, motion_ids, episode clock): the walk trace of
    tests/test_gpu_reset_options.py"""
    import tests.test_gpu_reset_options as T

    w, st = Worst(monkeypatch, "tests.test_gpu_reset_options"), {}
    T._trace("env_v1_walk_doffar", T.WALK, dict(T.DOF_FAR, **T.NOISE), general=False, **_hooks(st))
    assert st["env"]._c.terminate_when_dof_far and {"ovr_reset_root", "ovr_reset_dof_pos", "ovr_reset_dof_vel"} <= st["bound"]
    w.report("c reset noise + dof-far (trace, N=16)")


def test_randomized_default_dof_pos_in_arenas(monkeypatch):
    """default_dof_pos (bound only when it is randomised) and ovr_dof_pos_bias, against the oracle"""
    from tests.test_gpu_parity import _env_step_vs_oracle

    w, st = Worst(monkeypatch, "tests.test_gpu_parity"), {}
    ov = {"domain_rand.randomize_default_dof_pos": True, "domain_rand.dof_pos_range": [-0.05, 0.05]}
    _env_step_vs_oracle(5, 4, overrides=ov, default_bias=True, **_hooks(st, offset=2))
    assert {"default_dof_pos", "ovr_dof_pos_bias"} <= st["bound"]
    w.report("c default_dof_pos N=5")


def test_redraw_all_in_arenas(monkeypatch):
    """redraw_all: the episodic DR of EVERY env re-drawn inside the step (scales, delay, action queue), against the oracle"""
    from tests.test_gpu_parity import _env_step_vs_oracle

    w, st = Worst(monkeypatch, "tests.test_gpu_parity"), {}
    seen = []
    st["each"] = lambda env, k: seen.append(int(env._io.redraw_all))
    _env_step_vs_oracle(5, 4, redraw_steps=(1, 2), **_hooks(st, offset=1))
    assert seen == [0, 1, 1, 0]
    w.report("c redraw_all N=5")


def test_close_to_limit_gates_in_arenas(monkeypatch):
    """ovr_gate_u [3], the smallest operand of the step"""
    from tests.test_gpu_parity import _env_step_vs_oracle

    w, st = Worst(monkeypatch, "tests.test_gpu_parity"), {}
    ov = {"env.config.termination.terminate_when_close_to_dof_pos_limit": True, "env.config.termination.terminate_when_close_to_dof_vel_limit": True,
          "env.config.termination.terminate_when_close_to_torque_limit": True,
          "env.config.termination_scales.termination_close_to_dof_pos_limit": 0.55, "env.config.termination_scales.termination_close_to_dof_vel_limit": 0.02,
          "env.config.termination_scales.termination_close_to_torque_limit": 0.35}
    _env_step_vs_oracle(37, 4, overrides=ov, gates=[[0.1, 0.9, 0.9], [0.9, 0.1, 0.9], [0.9, 0.9, 0.1], [0.2, 0.2, 0.2]], **_hooks(st))
    assert "ovr_gate_u" in st["bound"]
    w.report("c gates N=37")


# ---- every PbhcStepIO pointer field is decided ---------------------------------------------------------------------------------------------
# NULL-able fields -> the case above that binds them non-NULL (each of those cases asserts it through `bound`)
NULLABLE = {
    "u_rfi": "test_motion_tracking_step_in_arenas", "ovr_start_time": "test_motion_tracking_step_in_arenas", "ovr_kp": "test_motion_tracking_step_in_arenas",
    "ovr_kd": "test_motion_tracking_step_in_arenas", "ovr_rfi_lim": "test_motion_tracking_step_in_arenas", "ovr_rao": "test_motion_tracking_step_in_arenas",
    "ovr_delay": "test_motion_tracking_step_in_arenas", "ovr_dof_pos_bias": "test_randomized_default_dof_pos_in_arenas",
    "ovr_gate_u": "test_close_to_limit_gates_in_arenas", "ovr_reset_root": "test_reset_noise_and_dof_far_prepass_in_arenas",
    "ovr_reset_dof_pos": "test_reset_noise_and_dof_far_prepass_in_arenas", "ovr_reset_dof_vel": "test_reset_noise_and_dof_far_prepass_in_arenas",
    "ovr_ou_step": "test_ou_process_and_parallel_serial_buffers_in_arenas", "ovr_ou_reset": "test_ou_process_and_parallel_serial_buffers_in_arenas",
    "ovr_ps_kp": "test_ou_process_and_parallel_serial_buffers_in_arenas", "ovr_ps_kd": "test_ou_process_and_parallel_serial_buffers_in_arenas",
    "ovr_ps_rao": "test_ou_process_and_parallel_serial_buffers_in_arenas", "ovr_ps_tau": "test_ou_process_and_parallel_serial_buffers_in_arenas",
    "rigid_body_state": "test_motion_tracking_step_eager_outputs_in_arenas", "contact_forces": "test_motion_tracking_step_eager_outputs_in_arenas",
    "ref_body_pos_extend": "test_motion_tracking_step_eager_outputs_in_arenas", "ref_body_rot_extend": "test_motion_tracking_step_eager_outputs_in_arenas",
    "default_dof_pos": "test_randomized_default_dof_pos_in_arenas", "ou_state": "test_ou_process_and_parallel_serial_buffers_in_arenas",
    "dr_base_mass": "test_general_tracking_step_in_arenas", "ref_time_out": "test_motion_tracking_step_in_arenas",
    "episode_rew_out": "test_motion_tracking_step_in_arenas",
}


def test_every_step_io_pointer_field_is_rehomed_or_listed():
    from pbhc_amd import _lib

    fields = SA.pointer_fields(_lib.PbhcStepIO)
    assert len(fields) > 60 and "obs" in fields and "time_out_buf" in fields
    undecided = [f for f in fields if f not in SA.REHOMED and f not in SA.NOT_REHOMED]
    assert not undecided, f"PbhcStepIO pointer fields neither re-homed by tests/step_arena.py nor listed there with a reason: {undecided}"
    assert not set(SA.REHOMED) & set(SA.NOT_REHOMED) and set(SA.REHOMED) | set(SA.NOT_REHOMED) == set(fields)
    assert all(len(r) > 20 for r in SA.NOT_REHOMED.values())
    for f, case in NULLABLE.items():
        assert f in SA.REHOMED and callable(globals().get(case)), (f, case)


def test_the_plain_step_binds_what_the_table_says(monkeypatch):
    """the fields NULLABLE credits to the plain case are bound, in arenas, by that case"""
    from tests.test_gpu_parity import _env_step_vs_oracle

    st = {}
    _env_step_vs_oracle(5, 1, **_hooks(st))
    want = {f for f, case in NULLABLE.items() if case == "test_motion_tracking_step_in_arenas"}
    assert want <= st["bound"], want - st["bound"]
    required = set(SA.pointer_fields(type(st["env"]._io))) - set(NULLABLE) - set(SA.NOT_REHOMED) - {"obs"}
    if not st["env"].simulator._link_mass_scale.numel():                     # (no randomised link masses: an empty tensor, a NULL pointer)
        required.discard("dr_link_mass")
    assert required <= st["bound"], required - st["bound"]


# ---- d. the recorder -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_recorder_buffers_in_arenas(offset, tmp_path):
    """k_record_motion with the [N, T, ...] buffers of PbhcRecordIO and its counter in arenas, N = 5, total_steps = 3, counter started at 3
    (the three dropped records behind it): steps 0..2 write frames 0..2 — copies of what the step left, as tests/test_gpu_record.py holds
    them —, steps 3..5 find the counter saturated at T + 3 and store nothing anywhere; only counter word 0 ever differs from 0."""
    import bench
    from scipy.spatial.transform import Rotation

    from pbhc_amd import _lib
    from tests.helpers import build_hip_env, skel_from_golden
    from tests.test_gpu_record import WALK, _record
    from tests.test_record_cpu import ROTVEC_TOL

    N, T = 5, 3
    cfg, env = build_hip_env(WALK, N, overrides=_record(tmp_path, T))
    env._write_to_file = False
    env.reset_all()                                                         # recorder step 0
    env.simulator.set_replay(*bench.make_replay_on_device(env, 6, seed=5))
    reg = SA.rehome(env, obs_pitch_extra=4, offset=offset)
    rio, D = env._rec_io, env.num_dof
    for k, t in list(env._rec.items()):
        env._rec[k] = SA.put(env, reg, "rec." + k, t, offset=offset)
        setattr(rio, k, env._rec[k].data_ptr())
    ctr = arena(1, _lib.K["PBHC_REC_COUNTER_WORDS"], fill=0x5A5A5A5A, data=torch.zeros(1, _lib.K["PBHC_REC_COUNTER_WORDS"], dtype=torch.int32), device=DEV,
                dtype=torch.int32, name="rec.counter")
    reg["rec.counter"] = ctr
    env._rec_counter = ctr.view[0]
    rio.counter = env._rec_counter.data_ptr()
    env._rec_counter[0] = 3
    env._rec_steps = 3
    gen = torch.Generator(device=DEV).manual_seed(1)
    axis = torch.as_tensor(np.asarray(skel_from_golden()["dof_axis"], np.float32), device=DEV)
    snap = None
    for k in range(6):
        if k == 1:
            env.episode_length_buf[::2] = 10 ** 6                            # resets inside the recording
        obs, rew, reset, _ = env.step({"actions": 0.5 * torch.randn(N, D, device=DEV, generator=gen)})
        SA.assert_intact(reg)
        SA.bound(env, reg)
        r, s = env._rec, env.simulator
        assert int(env._rec_counter[0]) == min(4 + k, T + 3) and not bool(env._rec_counter[1:].any()), k
        if k < T:
            assert torch.equal(r["root_trans_offset"][:, k], s.robot_root_states[:, 0:3] - env.env_origins), k
            assert torch.equal(r["root_rot"][:, k], s.robot_root_states[:, 3:7]) and torch.equal(r["root_lin_vel"][:, k], s.robot_root_states[:, 7:10])
            assert torch.equal(r["root_ang_vel"][:, k], s.robot_root_states[:, 10:13])
            assert torch.equal(r["dof"][:, k], s.dof_pos) and torch.equal(r["dof_vel"][:, k], s.dof_vel)
            assert torch.equal(r["action"][:, k], env.actions) and torch.equal(r["contact_mask"][:, k], env.contacts_filt)
            assert torch.equal(r["actor_obs"][:, k], obs["actor_obs"]) and torch.equal(r["terminate"][:, k], reset)
            mt = env.episode_length_buf.float() * float(env.dt) + env.motion_start_times
            assert float((r["motion_times"][:, k] - mt).abs().max()) <= float(np.spacing(np.float32(T * env.dt))), k
            assert torch.equal(r["pose_aa"][:, k, 1:D + 1], axis[None] * r["dof"][:, k, :, None]) and not bool(r["pose_aa"][:, k, D + 1:].any())
            rv = Rotation.from_quat(r["root_rot"][:, k].double().cpu().numpy()).as_rotvec()
            assert float(np.abs(r["pose_aa"][:, k, 0].double().cpu().numpy() - rv).max()) <= ROTVEC_TOL, k
            if k == 1:
                assert bool(reset[::2].all())
            if k == T - 1:
                snap = {name: reg["rec." + name].buf.clone() for name in r}
        else:
            for name in r:
                assert torch.equal(reg["rec." + name].buf.view(torch.uint8), snap[name].view(torch.uint8)), (k, name)
    assert env.motion_recorded
    # ... and a `terminate` 4 bytes off its 8-byte boundary is refused by the entry, before any launch
    bad = type(rio).from_buffer_copy(rio)
    bad.terminate = rio.terminate + 4
    before = {name: a.buf.clone() for name, a in reg.items()}
    assert _lib.lib().pbhc_record_motion(env._env, C.byref(env._io), C.byref(bad), _lib.current_stream()) == _lib.K["PBHC_EINVAL"]
    torch.cuda.synchronize()
    for name, a in reg.items():
        assert torch.equal(a.buf.view(torch.uint8), before[name].view(torch.uint8)), name


# ---- 4. what the kernels assume beyond 4-byte alignment is refused at the entry, before any launch -----------------------------------------
@pytest.mark.parametrize("what", ["reset_buf", "motion_ids", "ovr_delay", "hist (specialised)", "totals_out"])
def test_misaligned_buffers_are_refused_before_the_launch(what):
    """int64 buffers and the f64 totals 4 bytes off an 8-byte boundary, and the specialised kernel's history rows 4 bytes off their 16-byte
    boundary: PBHC_EINVAL from the entry itself, and no byte of any arena changes (nothing was launched)"""
    from pbhc_amd import _lib
    from tests.test_gpu_parity import _env_step_vs_oracle

    st = {}
    _env_step_vs_oracle(5, 1, **_hooks(st))                                  # a live, re-homed env with every override bound
    env, reg = st["env"], st["reg"]
    assert env.is_specialised
    torch.cuda.synchronize()
    before = {k: a.buf.clone() for k, a in reg.items()}
    io = type(env._io).from_buffer_copy(env._io)
    field = "hist" if what.startswith("hist") else what
    entries = ("pbhc_env_step_launch", "pbhc_env_step")
    if field == "totals_out":                                                # NULL in a single-process env: a buffer of its size, in an arena
        n_tot = _lib.K["PBHC_NUM_TOTALS"]
        reg["totals_out"] = arena(1, n_tot + 1, fill=POISON, data=torch.zeros(1, n_tot + 1, dtype=torch.float64), device=DEV, dtype=torch.float64, name="totals_out")
        before["totals_out"] = reg["totals_out"].buf.clone()
        io.totals_out = reg["totals_out"].ptr()
        entries += ("pbhc_env_step_finish",)
        rc = _lib.lib().pbhc_env_finalize(env._env, io.totals_out + 4, 5.0, _lib.current_stream())
        assert rc == _lib.K["PBHC_EINVAL"], rc
    setattr(io, field, getattr(io, field) + 4)
    for entry in entries:
        rc = getattr(_lib.lib(), entry)(env._env, C.byref(io), _lib.current_stream())
        assert rc == _lib.K["PBHC_EINVAL"], (entry, rc)
        assert ("16-byte aligned" if field == "hist" else ("totals_out" if field == "totals_out" else "8-byte aligned")) in _lib.lib().pbhc_last_error().decode()
    torch.cuda.synchronize()
    for k, a in reg.items():
        assert torch.equal(a.buf.view(torch.uint8), before[k].view(torch.uint8)), k


def test_misaligned_ids_of_the_motion_lookup_are_refused():
    """pbhc_motion_state with `ids` 4 bytes off an 8-byte boundary: PBHC_EINVAL, `out` untouched"""
    from pbhc_amd import _lib

    lib = _lib.lib()
    sk, ml, _ = _two_clip_library()
    n, D, Bx = 5, sk.num_dof, sk.num_bodies_ext
    ids = arena(1, n + 1, fill=0, data=torch.ones(1, n + 1, dtype=torch.int64), device=DEV, dtype=torch.int64, name="ids")
    times = arena(1, n, fill=POISON, data=torch.zeros(1, n), device=DEV, name="times")
    out = arena(n, ml.row, fill=POISON, device=DEV, name="out")
    rc = lib.pbhc_motion_state(C.byref(ml.table), Bx, D, ids.ptr() + 4, times.ptr(), None, n, out.ptr(), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == _lib.K["PBHC_EINVAL"] and out.untouched()


# ---- e. pbhc_motion_state and pbhc_sim_fk through the C ABI -----------------------------------------------------------------------------------
_LIB2 = {}


def _two_clip_library():
    """(skeleton, HIP MotionLib of three clips whose frame rows were REBUILT into an arena, the rows' arena).  Lookups use clips 1 and 2:
    clip 2 is the table's LAST, so the row behind its last row is poison — a whole row of it, more than a lookup that lost its clamp would
    read — and clip 1's last row has clip 2's first behind it.  Clip 0 is the spare one the margins of `ids` name."""
    if not _LIB2:
        import bench
        from pbhc_amd.motion_lib import MotionLib
        from pbhc_amd.skeleton import Skeleton
        from tests.helpers import GOLDEN

        g = dict(np.load(os.path.join(GOLDEN, "motion_state_origin_walk.npz")))
        clips = bench.synth_library(dict(pose_aa=g["pose_aa"][:40], root_trans_offset=g["root_trans_offset"][:40], fps=int(g["fps"])), 3, seed=2)
        sk = Skeleton.from_json(os.path.join(GOLDEN, "skeleton_g1_23dof_lock_wrist_fitmotionONLY.json"))
        ml = MotionLib(sk, clips, 4, DEV)
        torch.cuda.synchronize()
        first = ml.frames.clone()
        F_, row = first.shape
        buf = torch.full((2 * MARGIN + (F_ + 1) * row,), POISON_BITS[torch.float32], dtype=torch.int32, device=DEV).view(torch.float32)
        rows = Arena(buf, buf.as_strided((F_, row), (row, 1), MARGIN), POISON, "table rows")        # (one more row of poison behind the last)
        ml._build_unique_tables(ml._clips, into=rows.view)                  # pbhc_motion_build_batch stores straight into the arena
        torch.cuda.synchronize()
        assert rows.intact(), rows.damage()
        assert torch.equal(rows.view, first), "the rebuild into the arena differs from the first build"
        ml.frames = rows.view
        ml.table.frames = rows.ptr()
        _LIB2.update(sk=sk, ml=ml, rows=rows, clips=clips)
    return _LIB2["sk"], _LIB2["ml"], _LIB2["rows"]


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 5, 37])
def test_motion_state_in_arenas(n, offset):
    """ids, times, offset and out in arenas, the table's rows in an arena with poison behind the last row; times 0, a frame boundary, exactly
    the clip length and beyond it.  On the table's LAST clip both frames of the pair are then its last row: the blend is exactly 0 there, so a
    lookup that read the row behind it would still match the oracle if that row were data — it is poison, and 0 x NaN fails the
    finite-result check.  On the clip before it the row behind is the last clip's first, and the result must still be its own clamp.
    Against oracle/motion_lib.py with the tolerances of test_motion_state_matches_reference."""
    from oracle.motion_lib import MotionLib as OML
    from pbhc_amd import _lib
    from tests.helpers import skel_from_golden
    from tests.test_gpu_parity import angvel_tol, close, slerp_jump_bound, table_speed_floor

    sk, ml, rows = _two_clip_library()
    oml = _LIB2.setdefault("oml", OML(skel_from_golden(), _LIB2["clips"]))
    D, Bx = sk.num_dof, sk.num_bodies_ext
    gen = torch.Generator().manual_seed(n)
    ids = 1 + torch.arange(n) % 2
    ids[0] = 2
    mlen, dt = oml.motion_len[ids], oml.motion_dt[ids]
    t = torch.rand(n, generator=gen) * mlen
    edge = [mlen[0], torch.tensor(0.0), 7 * dt[0], mlen[0] + 0.37, mlen[0] - 0.5 * dt[0]]       # n = 1: exactly the clip length, on the last clip
    for i, v in enumerate(edge[:n]):
        t[i], ids[i] = v, 2
    if n > 8:
        assert int(ids[6]) == 1 and int(ids[8]) == 1
        t[6], t[8] = mlen[6], mlen[8] + 1.0                                 # the same on clip 1, whose last row has clip 2's first behind it
    off = torch.randn(n, 3, generator=gen)
    a_ids = arena(1, n, fill=0, data=ids[None], device=DEV, dtype=torch.int64, name="ids")
    a_t = arena(1, n, offset=offset, fill=POISON, data=t[None], device=DEV, name="times")
    a_off = arena(n, 3, offset=offset, fill=POISON, data=off, device=DEV, name="offset")
    a_out = arena(n, ml.row, offset=offset, fill=POISON, device=DEV, name="out")
    _lib.check(_lib.lib().pbhc_motion_state(C.byref(ml.table), Bx, D, a_ids.ptr(), a_t.ptr(), a_off.ptr(), n, a_out.ptr(), _lib.current_stream()), "pbhc_motion_state")
    torch.cuda.synchronize()
    for a in (a_ids, a_t, a_off, a_out, rows):
        assert a.intact(), a.damage()
    out = a_out.view.cpu()
    assert bool(torch.isfinite(out).all()), "poison reached a result"
    ref = oml.get_motion_state(ids, t, offset=off)
    f0, f1, _ = oml.calc_frame_blend(t, oml.motion_len[ids], oml.num_frames[ids], oml.motion_dt[ids])
    f0, f1 = f0 + oml.length_starts[ids], f1 + oml.length_starts[ids]
    last = rows.view.shape[0] - 1
    assert int(f0[0]) == last and int(f1[0]) == last                        # t = clip length on the last clip: both frames are the table's last row
    if n > 3:
        assert int(f0[3]) == last and int(f1[3]) == last                    # ... and beyond it
    if n > 8:
        assert int(f1[6]) == int(f1[8]) == int(oml.length_starts[2]) - 1    # clip 1's clamp stays inside clip 1
    rot_tol = slerp_jump_bound(oml.cat["grs_t"][f0], oml.cat["grs_t"][f1])
    speed = table_speed_floor(oml.cat["gavs_t"])
    speed = torch.minimum(speed[f0], speed[f1])
    o = 2 * D + 2
    got = dict(dof_pos=out[:, :D], dof_vel=out[:, D:2 * D], rg_pos_t=out[:, o:o + 3 * Bx].view(n, Bx, 3), rg_rot_t=out[:, o + 3 * Bx:o + 7 * Bx].view(n, Bx, 4),
               body_vel_t=out[:, o + 7 * Bx:o + 10 * Bx].view(n, Bx, 3), body_ang_vel_t=out[:, o + 10 * Bx:].view(n, Bx, 3))
    worst = 0.0
    for k, x in got.items():
        r = ref[k].float()
        if "ang_vel" in k:
            tol = angvel_tol(r, float(dt[0]), norm=speed)
            close(x, r, tol, k)
        elif "rot" in k:
            tol = rot_tol.expand_as(r) + 5e-5 * r.abs()
            close(x, r, rot_tol.expand_as(r), k, rtol=5e-5)
        else:
            tol = 5e-5 + 5e-5 * r.abs()
            close(x, r, 5e-5, k)
        worst = max(worst, float(((x - r).abs() / tol).max()))
    print(f"WORST e motion_state n={n} offset={offset}: err/tol {worst:.3f}")


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("n", [1, 5, 37])
def test_sim_fk_in_arenas(n, stride, offset):
    """root, dof_pos / dof_vel (stride 2: the two columns of ONE [n, D, 2] dof_state operand) and out in arenas, against oracle/fk.py with the
    tolerances of test_sim_fk_matches_oracle"""
    from oracle.fk import sim_fk
    from pbhc_amd import _lib
    from pbhc_amd.skeleton import Skeleton
    from tests.helpers import GOLDEN, skel_from_golden
    from tests.test_gpu_parity import close

    sk = Skeleton.from_json(os.path.join(GOLDEN, "skeleton_g1_23dof_lock_wrist_fitmotionONLY.json"))
    D, B = sk.num_dof, sk.num_bodies
    gen = torch.Generator().manual_seed(10 * n + stride)
    root = torch.randn(n, 13, generator=gen)
    root[:, 3:7] /= root[:, 3:7].norm(dim=-1, keepdim=True)
    q, qd = torch.randn(n, D, generator=gen), torch.randn(n, D, generator=gen)
    a_root = arena(n, 13, offset=offset, fill=POISON, data=root, device=DEV, name="root_states")
    a_out = arena(n, B * 13, offset=offset, fill=POISON, device=DEV, name="out")
    if stride == 2:
        a_q = a_qd = arena(n, 2 * D, offset=offset, fill=POISON, data=torch.stack([q, qd], -1).reshape(n, 2 * D), device=DEV, name="dof_state")
        pq, pqd = a_q.ptr(), a_q.ptr() + 4
    else:
        a_q = arena(n, D, offset=offset, fill=POISON, data=q, device=DEV, name="dof_pos")
        a_qd = arena(n, D, offset=offset, fill=POISON, data=qd, device=DEV, name="dof_vel")
        pq, pqd = a_q.ptr(), a_qd.ptr()
    csk = sk.to_c()
    _lib.check(_lib.lib().pbhc_sim_fk(C.byref(csk), a_root.ptr(), pq, pqd, stride, n, a_out.ptr(), _lib.current_stream()), "pbhc_sim_fk")
    torch.cuda.synchronize()
    for a in (a_root, a_q, a_qd, a_out):
        assert a.intact(), a.damage()
    out = a_out.view.cpu().view(n, B, 13)
    assert bool(torch.isfinite(out).all()), "poison reached a result"
    p, r, v, w = sim_fk(skel_from_golden(), root, q, qd)
    worst = 0.0
    for name, x, ref, tol in (("pos", out[..., 0:3], p, 1e-5), ("rot", out[..., 3:7], r, 1e-5), ("vel", out[..., 7:10], v, 2e-5), ("ang", out[..., 10:13], w, 2e-5)):
        close(x, ref, tol, name)
        worst = max(worst, float(((x - ref).abs() / (tol + tol * ref.abs())).max()))
    print(f"WORST e sim_fk n={n} stride={stride} offset={offset}: err/tol {worst:.3f}")


# ---- f. the closed-loop simulators ------------------------------------------------------------------------------------------------------------
CL_EPB = 8                                                   # envs per workgroup of the simulators' kernels (csrc/pbhc_closed_loop.h, their launches)


def _placer(reg, offset):
    def place(name, t):
        rows, cols = t.shape[0], t.numel() // t.shape[0]
        reg[name] = arena(rows, cols, offset=offset, fill=POISON, data=t.reshape(rows, cols), device=DEV, name=name)
        return reg[name].view.reshape(t.shape)

    return place


def test_cl_epb_is_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pbhc_amd", "csrc", "pbhc_closed_loop.h")).read()
    assert f"#define CL_EPB {CL_EPB} " in src


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, CL_EPB + 1, 33])
def test_articulated_substep_in_arenas(n, offset, monkeypatch):
    """pbhc_debug_articulated_substeps, one sub-step, every pointer argument in an arena: test_qdd_of_one_substep_equals_the_model's comparison
    and bound (K = 16) at a partly filled workgroup, one workgroup plus one env, and 33"""
    import functools

    import tests.test_gpu_articulated_sim as A

    reg = {}
    monkeypatch.setattr(A, "_debug", functools.partial(A._debug, place=_placer(reg, offset)))
    ratios = []
    monkeypatch.setattr(A, "_report", lambda what, err, tol, err32=None: ratios.append(float((err / tol).max())))
    A.test_qdd_of_one_substep_equals_the_model(A.TREE if n != 33 else A.G1, n)
    assert set(reg) == {"base", "q", "v", "tau", "out_q", "out_v", "out_qdd0"}
    for a in reg.values():
        assert a.intact(), a.damage()
        assert bool(torch.isfinite(a.view).all()), a.name
    print(f"WORST f articulated n={n} offset={offset}: err/bound {ratios[0]:.3f}")


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, CL_EPB + 1, 33])
def test_floating_substep_in_arenas(n, offset):
    """pbhc_debug_floating_substeps, one sub-step, every pointer argument in an arena, the point table included: [a_0, alpha_0, q''] and every
    point's force against tests/floating_model.py within test_one_substep_equals_the_model's bounds (K = 16)"""
    import tests.test_gpu_floating_sim as F
    from tests import floating_model as fm

    mjcf = F.TREE if n != 33 else F.G1
    sk, m, p, table = F._setup(mjcf)
    reg = {}
    place = _placer(reg, offset)
    table = place("points", table)
    p.points = table.data_ptr()
    root, q, v, tau = fm.random_states(m, n, 5)
    want, f, d = fm.forward(m, fm.state(root, q, v), tau, F.H)
    tol, tol_f = F.GAMMA * d["terms"], F.GAMMA * d["f_abs"]
    got = F._debug(sk, p, root, q, v, tau, 1, place=place)
    assert set(reg) == {"points", "root", "q", "v", "tau", "out_root", "out_q", "out_v", "out_acc0", "out_force"}
    for a in reg.values():
        assert a.intact(), a.damage()
        assert bool(torch.isfinite(a.view).all()), a.name
    gf = F._by_point(m, got["force"])
    err, ef = np.abs(got["acc0"] - want), np.abs(gf - f)
    print(f"WORST f floating n={n} offset={offset}: err/bound {float((err / tol).max()):.3f}, forces {float((ef / np.maximum(tol_f, 1e-300)).max()):.3f}")
    assert (ef <= tol_f).all(), float((ef / np.maximum(tol_f, 1e-300)).max())
    assert (err <= tol).all(), (float((err / tol).max()), np.argwhere(err > tol)[:5].tolist())


def _small_scenario(mod, monkeypatch):
    """the simulators' scenario at a batch below ten envs: its three 'ending' envs folded into the batch"""
    scenario = mod.scenario

    def folded(N, D, clip, **kw):
        sc = scenario(N, D, clip, **kw)
        sc["ending"] = sorted({e % N for e in sc["ending"]})
        sc["beyond_limit"] = [(e % N, d_, side) for e, d_, side in sc["beyond_limit"]]
        return sc

    monkeypatch.setattr(mod, "scenario", folded)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_floating_base_sim_env_in_arenas(offset, monkeypatch):
    """FloatingBaseSim through the env, N = 5 (one ragged workgroup of k_floating_sim AND of k_env_step), 2 steps, the env re-homed: tau0,
    the point table, the one-frame window the simulator writes and the step reads, the contact frame.  The frame against the model within
    the carried bound of test_frame_equals_the_model_one_step_at_a_time; tau0 is the step's torques bit for bit."""
    import tests.test_gpu_floating_sim as F

    _small_scenario(F, monkeypatch)
    st = {}
    hooks = _hooks(st, offset=offset)
    rehome = hooks["prepare"]

    def prepare(env):
        env.simulator.set_debug_root(True)                   # root_acc [N, 6]: one more buffer the kernel stores
        rehome(env)

    env, m, steps = F._run_case(F.WALK, 5, False, steps=2, **dict(hooks, prepare=prepare))
    reg, p = st["reg"], env.simulator._params
    assert {"sim.tau0", "sim.points", "sim.root_acc", "frame_root", "frame_contact", "frame_dof_pos", "frame_dof_vel"} <= set(reg)
    assert p.tau0 == reg["sim.tau0"].ptr() and p.points == reg["sim.points"].ptr() and p.root_acc == reg["sim.root_acc"].ptr()
    for name in ("sim.tau0", "sim.points", "sim.root_acc", "frame_root", "frame_contact", "frame_dof_pos", "frame_dof_vel"):
        assert reg[name].ptr() % 16 == 4 * offset, name
    assert bool(torch.isfinite(env.simulator.root_acc).all())
    SA.bound(env, reg)
    SA.assert_intact(reg)
    D, worst = env.num_dof, 0.0
    owners = sorted({b for b, _ in m["points"]})
    for k, r in enumerate(steps):
        for name in ("frame_q", "frame_v", "frame_root", "root", "dof_pos"):
            assert np.isfinite(r[name]).all(), (k, name)
        mm, err, ok = F._compare_step(m, r, D)
        if ok.any():
            worst = max(worst, float((err / mm["E"])[ok].max()))
        assert not (err > mm["E"])[ok].any(), (k, float((err / mm["E"])[ok].max()))
        keep = torch.from_numpy(~r["reset"]).to(r["tau0"].device)
        assert torch.equal(r["tau0"][keep], r["torques"][keep]), k
        c = r["frame_contact"].cpu().double().numpy()
        c[:, owners] = 0.0
        assert not c.any(), k
    print(f"WORST f FloatingBaseSim env N=5 offset={offset}: err/bound {worst:.3f}")
    _entry_refuses_misaligned_int64("pbhc_floating_sim_step", env, reg)


def _entry_refuses_misaligned_int64(entry, env, reg):
    """a simulator's step entry with an int64 buffer 4 bytes off its 8-byte boundary: PBHC_EINVAL, no byte of any arena changes"""
    from pbhc_amd import _lib

    before = {name: a.buf.clone() for name, a in reg.items()}
    for field in ("motion_ids", "episode_length_buf", "action_delay_idx"):
        io = type(env._io).from_buffer_copy(env._io)
        setattr(io, field, getattr(env._io, field) + 4)
        rc = getattr(_lib.lib(), entry)(env._env, C.byref(io), C.byref(env.simulator._params), _lib.current_stream())
        assert rc == _lib.K["PBHC_EINVAL"], (entry, field, rc)
    torch.cuda.synchronize()
    for name, a in reg.items():
        assert torch.equal(a.buf.view(torch.uint8), before[name].view(torch.uint8)), name


def test_articulated_sim_entry_refuses_misaligned_int64():
    """pbhc_articulated_sim_step shares the simulators' argument check: held on an ArticulatedSim env of its own, re-homed, nothing launched"""
    import tests.test_gpu_articulated_sim as A

    cfg, env = A._build(A.WALK, 5, False)
    env.reset_all()
    reg = SA.rehome(env)
    env._sync_replay_io()
    env._io.actions_in = SA.put(env, reg, "actions_in", torch.zeros(5, env.num_dof, device=DEV)).data_ptr()
    assert env.simulator.STEP == "pbhc_articulated_sim_step"
    _entry_refuses_misaligned_int64("pbhc_articulated_sim_step", env, reg)


@pytest.mark.parametrize("N,offset", [(5, 0), (5, 1), (5, 2), (5, 3), (33, 0)])
def test_joint_space_sim_env_in_arenas(N, offset, monkeypatch):
    """JointSpaceSim has no test-only export: through the env, re-homed, at one ragged workgroup (N = 5) and at 33; the frame against
    tests/joint_sim_model.py within the bounds of test_integrator_equals_the_model_one_step_at_a_time, arenas checked after every step"""
    import tests.test_gpu_joint_sim as J

    _small_scenario(J, monkeypatch)
    st = {}
    env, sc, steps = J._run_case(J.WALK, N, False, True, **_hooks(st, offset=offset))
    reg = st["reg"]
    assert env.simulator._params.tau0 == reg["sim.tau0"].ptr() and "u_rfi" in st["bound"]
    for name in ("sim.tau0", "frame_root", "frame_contact", "frame_dof_pos", "frame_dof_vel"):
        assert reg[name].ptr() % 16 == 4 * offset, name
    worst = 0.0
    for k, r in enumerate(steps):
        P, m = r["P"], r["model"]
        tol_v = 32 * J.EPS * (m["vmax"] + P["h"] * P["torque_limit"] / P["inertia"])
        tol_q = tol_v * P["decimation"] * P["h"] + 8 * J.EPS * np.abs(m["q"])
        ok = m["margin"] >= 1e-5
        assert np.isfinite(r["frame_v"]).all() and np.isfinite(r["frame_q"]).all() and np.isfinite(r["tau0"]).all() and np.isfinite(r["torques"]).all(), k
        ev, eq = np.abs(r["frame_v"] - m["v"]), np.abs(r["frame_q"] - m["q"])
        worst = max(worst, float((ev / tol_v)[ok].max()), float((eq / tol_q)[ok].max()))
        assert not (ev > tol_v)[ok].any() and not (eq > tol_q)[ok].any(), (k, float((ev / tol_v)[ok].max()), float((eq / tol_q)[ok].max()))
        keep = ~r["reset"]
        assert np.array_equal(r["dof_pos"][keep], r["frame_q"][keep]) and np.array_equal(r["dof_vel"][keep], r["frame_v"][keep])
    print(f"WORST f JointSpaceSim env N={N} offset={offset}: err/bound {worst:.3f}")
    _entry_refuses_misaligned_int64("pbhc_joint_sim_step", env, reg)
