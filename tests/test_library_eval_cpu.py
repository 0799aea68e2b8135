"""Library evaluation (env.library_sweep, k_clip_track): the C ABI's argument checks and the sweep's host-side refusals (no GPU)."""
import ctypes as C
import types

import pytest
import torch

from pbhc_amd import _lib
from pbhc_amd.envs.motion_tracking import LeggedRobotMotionTracking
from pbhc_amd.skeleton import Skeleton
from tests.helpers import skel_from_golden


def _skeleton(robot="g1_23dof"):
    s = skel_from_golden(robot)
    return Skeleton(s["body_names"], s["body_names_ext"], s["parents"], s["offsets"], s["local_rot_wxyz"], s["dof_axis"]).to_c()


def _table(csk, p, entries=1):
    t = _lib.PbhcMotionTable()
    t.frames = t.length_starts = t.num_frames = t.motion_dt = t.motion_len = p.value
    t.row, t.num_motions = 2 * csk.num_dof + 2 + 13 * csk.num_bodies_ext, entries
    return t


def test_clip_track_is_exported():
    assert "pbhc_clip_track" in _lib.EXPORTS
    assert callable(_lib.lib().pbhc_clip_track)


def test_null_bad_sizes_and_oversize_skeletons_return_einval_without_a_gpu():
    lib, E = _lib.lib(), _lib.K["PBHC_EINVAL"]
    p = C.c_void_p(64)                 # never dereferenced: every call below is refused on the host
    sk = _skeleton()
    tbl = _table(sk, p)

    def call(skel=sk, table=tbl, ptrs=None, N=4, M=2, window=p):
        ptrs = [p] * 8 if ptrs is None else ptrs                  # root_states .. slot_clip, retire
        return lib.pbhc_clip_track(C.byref(skel) if skel is not None else None, C.byref(table) if table is not None else None, *ptrs, N, M, window, None)

    def refused(rc):
        return rc == E and b"bad argument" in lib.pbhc_last_error()

    assert refused(call(skel=None)) and refused(call(table=None)) and refused(call(window=None))
    assert b"pbhc_clip_track" in lib.pbhc_last_error()
    for k in range(7):                 # each pointer on its own; retire (the eighth) may be NULL
        ptrs = [p] * 8
        ptrs[k] = None
        assert refused(call(ptrs=ptrs)), k
    for member in ("frames", "length_starts", "num_frames", "motion_dt", "motion_len"):
        t = _table(sk, p)
        setattr(t, member, None)
        assert refused(call(table=t)), member
    assert refused(call(N=0)) and refused(call(N=-3)) and refused(call(M=0))
    assert refused(call(table=_table(sk, p, entries=0)))
    t = _table(sk, p)
    t.row += 1                         # a table built for another skeleton
    assert refused(call(table=t))
    K = _lib.K
    for member, value in (("num_bodies_ext", K["PBHC_MAX_BODIES"] + 1), ("num_dof", K["PBHC_MAX_DOF"] + 1), ("num_bodies", 0)):
        big = _skeleton()
        setattr(big, member, value)
        assert refused(call(skel=big, table=_table(big, p))), member
    deep = _skeleton()
    deep.chain_len[deep.num_bodies - 1] = K["PBHC_MAX_DEPTH"] + 1
    assert refused(call(skel=deep))
    stray = _skeleton()                # a chain entry that is not a body: what the kernel would index LDS with
    stray.chain[stray.num_bodies - 1][0] = 1000
    assert refused(call(skel=stray))


class _NeverLaunched:
    """stands for every member library_sweep would touch after its checks: any use is a test failure"""

    def __getattr__(self, name):
        raise AssertionError(f"library_sweep went on to use .{name} after a refusal was due")


def _bare_env(**state):
    env = LeggedRobotMotionTracking.__new__(LeggedRobotMotionTracking)
    env.config = types.SimpleNamespace(get=lambda k, d=None: state.get(k, d))
    env._rec = state.get("_rec")
    if "_stat_mode" in state:
        env._stat_mode = state["_stat_mode"]
    env._motion_lib = env.simulator = env._lib = _NeverLaunched()
    return env


@pytest.mark.parametrize("state,match", [(dict(_stat_mode="rollout"), "data-parallel"), (dict(_stat_mode="step"), "data-parallel"),
                                         (dict(_rec={"root_trans_offset": None}), "recorder"),
                                         (dict(enforce_randomize_motion_start_eval=True), "enforce_randomize_motion_start_eval")])
def test_library_sweep_refusals_come_before_any_launch(state, match):
    env = _bare_env(**state)
    with pytest.raises(_lib.PbhcError, match=match):
        env.library_sweep(lambda obs: None)


def test_library_sweep_is_refused_inside_a_stream_capture(monkeypatch):
    env = _bare_env()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)      # (no device here to ask)
    assert env._library_sweep_refusal() is None
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.PbhcError, match="stream capture"):
        env.library_sweep(lambda obs: None)
