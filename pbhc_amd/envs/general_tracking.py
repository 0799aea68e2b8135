"""LeggedRobotGeneralTracking — drop-in for the reference's KungfuBot2 (general tracking) env.

Same constructor / methods / attributes as the reference class
(reference: humanoidverse/envs/motion_tracking/general_tracking.py:29-107, on legged_robot_base.py and base_task.py), selected by
`env._target_: pbhc_amd.envs.general_tracking.LeggedRobotGeneralTracking`.  The whole `step()` is the MODE-1 instantiation of the
fused HIP kernel (true quaternion differences, anchor-relative frames, 20-step future targets, key-body rewards, the three
anchor / body-z terminations); see pbhc_amd/envs/motion_tracking.py for the shared host logic.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from . import env_config
from .motion_tracking import LeggedRobotMotionTracking

K = _lib.K


class LeggedRobotGeneralTracking(LeggedRobotMotionTracking):
    TRACKING_MODE = 1

    def __init__(self, config, device):
        super().__init__(config, device)
        L = self.layout
        self.key_body_id = L.key
        self.anchor_index = int(self._c.anchor_index)
        self.num_key_bodies = len(L.key)
        self.tar_obs_steps = torch.tensor(L.future_steps, dtype=torch.long, device=self.device)     # PPO reads len(env.tar_obs_steps)
        self.curr_motion_ids = self._motion_lib.slot_clip
        self.num_motions = self._motion_lib._num_unique_motions
        self.motion_start_idx = 0

    def _load_motions_initial(self):
        self._motion_lib.load_motions(random_sample=False, max_len=self.max_len)                 # general_tracking.py:57-61: init not random sample

    def next_task(self):
        self.motion_start_idx += self.num_envs
        if self.motion_start_idx >= self.num_motions:
            self.motion_start_idx = 0
        if self._clip_window is not None or self._start_window is not None:
            self.wait_finalize()                     # the collectors of the last step read the old slot -> clip table
        self._motion_lib.load_motions(random_sample=False, start_idx=self.motion_start_idx, max_len=self.max_len)
        self.curr_motion_ids = self._motion_lib.slot_clip
        self._redraw_start_times()                   # start_sampling: the buffered start times belong to the old table's clip lengths
        self.reset_all()

    # ---- the left <-> right mirror of observations and actions (algo.config.symmetry) ----------------------------------------
    def rebuild_observations(self):
        super().rebuild_observations()
        self._mirror_maps = None                    # the groups changed: the maps are rebuilt on their next use

    def mirror_maps(self):
        """{group: (index int32[C], sign float32[C])} for every observation group, plus "actions", as device tensors:
        `mirrored[j] = sign[j] * x[index[j]]` (envs/obs_mirror.py).  Built on first use and again after rebuild_observations()."""
        maps = self.__dict__.get("_mirror_maps")
        if maps is None:
            from . import obs_mirror
            from .motion_tracking import _TopView

            aug = getattr(self._motion_lib, "augmentation", None)
            host = obs_mirror.build(_TopView(self.config), self.skeleton, aug.symmetry_tol if aug is not None else 1e-4)
            maps = self._mirror_maps = {g: (torch.from_numpy(i).to(self.device), torch.from_numpy(s).to(self.device)) for g, (i, s) in host.items()}
        return maps

    def mirror_rows(self, jobs):
        """ONE `pbhc_mirror_rows` launch for [(group, x [rows, C] float32, out [rows, >= C])]: out[:, :C] = the mirror of x; the rows of x and of
        out may be padded (unit inner stride), and out may be a wider tensor whose leading C columns are written in place.
        No out may share memory with an x of the same call: refused."""
        maps = self.mirror_maps()
        arr = (_lib.PbhcMirrorJob * len(jobs))()
        rows = jobs[0][1].shape[0]
        for q, (group, x, out) in zip(arr, jobs):
            index, sign = maps[group]
            C_ = index.numel()
            _lib.require_gpu_rows(x, f"mirror_rows[{group}] x", torch.float32, (rows, C_))
            _lib.require_gpu_rows(out, f"mirror_rows[{group}] out", torch.float32)
            if out.shape[0] != rows or out.shape[1] < C_:
                raise _lib.PbhcError(f"mirror_rows[{group}] out: expected [{rows}, >= {C_}], got {tuple(out.shape)}")
            if C_ > K["PBHC_MIRROR_MAX_WIDTH"]:
                raise _lib.PbhcError(f"mirror_rows[{group}]: {C_} columns, at most {K['PBHC_MIRROR_MAX_WIDTH']}")
            q.src, q.dst, q.index, q.sign = x.data_ptr(), out.data_ptr(), index.data_ptr(), sign.data_ptr()
            q.width, q.src_pitch, q.dst_pitch = C_, x.stride(0), out.stride(0)
        # the kernel gathers while other lanes and rows store: no destination of the launch may share memory with a source of it
        span = lambda t, w: (t.data_ptr(), t.data_ptr() + 4 * ((rows - 1) * t.stride(0) + w))
        for gd, _, out in jobs:
            d0, d1 = span(out, maps[gd][0].numel())
            for gs, x, _ in jobs:
                s0, s1 = span(x, maps[gs][0].numel())
                if d0 < s1 and s0 < d1:
                    raise _lib.PbhcError(f"mirror_rows[{gd}] out overlaps the source of [{gs}]: the mirror cannot run in place")
        _lib.check(self._lib.pbhc_mirror_rows(arr, len(jobs), rows, _lib.current_stream()), "pbhc_mirror_rows")

    def mirror_observation(self, group, x, out=None):
        """the mirror image of observation rows x [rows, C] of `group` (float32, device) -> out (a new tensor unless given; it must not
        share memory with x)"""
        if group not in self.mirror_maps() or group == "actions":
            raise _lib.PbhcError(f"mirror_observation: {group!r} is not an observation group ({[g for g in self.mirror_maps() if g != 'actions']})")
        if out is None:
            out = torch.empty(x.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
        self.mirror_rows([(group, x, out)])
        return out

    def mirror_action(self, a, out=None):
        """the mirror image of action rows a [rows, num_actions] -> out (a new tensor unless given; it must not share memory with a)"""
        if out is None:
            out = torch.empty(a.shape[0], a.shape[1], dtype=torch.float32, device=a.device)
        self.mirror_rows([("actions", a, out)])
        return out

    _STATE_HOST = LeggedRobotMotionTracking._STATE_HOST + ("motion_start_idx",)      # exact resume: next_task()'s position in the library

    def read_log(self):
        out = super().read_log()
        g = self.globals.cpu().numpy()
        L0 = K["PBHC_G_LOG"]
        extra = {
            "key_body_diff_norm": g[L0 + K["PBHC_L_KEY_BODY_DIFF_NORM"]], "local_upper_body_diff_norm": g[L0 + K["PBHC_L_LOCAL_UPPER_BODY_DIFF_NORM"]],
            "local_lower_body_diff_norm": g[L0 + K["PBHC_L_LOCAL_LOWER_BODY_DIFF_NORM"]], "local_vr_3point_diff_norm": g[L0 + K["PBHC_L_LOCAL_VR_3POINT_DIFF_NORM"]],
            "local_key_body_diff_norm": g[L0 + K["PBHC_L_LOCAL_KEY_BODY_DIFF_NORM"]], "terminate_by_ref_pos_z": g[L0 + K["PBHC_L_TERM_REF_POS_Z"]],
            "terminate_by_ref_ori": g[L0 + K["PBHC_L_TERM_REF_ORI"]], "terminate_by_body_z": g[L0 + K["PBHC_L_TERM_BODY_Z"]],
        }
        out.update(extra)
        self.log_dict.update({k: torch.tensor(float(v)) for k, v in extra.items()})
        return out
