"""Reference-motion library on the GPU: load-time FK tables + per-step phase lookup.

Drop-in for the parts of MotionLibBase / MotionLibRobot / MotionLibRobotWJX the env uses
(reference: humanoidverse/utils/motion_lib/motion_lib_base.py:123-259,261-391,486-513;
motion_lib_robot_WJX.py:146-293).  Differences by design:
* FK + filtered velocities run once per UNIQUE clip in HIP (`pbhc_motion_build`), not once per
  env slot in Python; slots map to clips through `slot_clip`.
* all per-frame quantities live in ONE packed row per frame
  `[dof_pos D | dof_vel D | contact 2 | pos Bx*3 | rot Bx*4 | vel Bx*3 | ang Bx*3]`
  so a lookup reads two contiguous rows.
Ingestion (`motion_ingest`): retarget (key-point clips -> joint angles) -> upload -> screen (contact masks, stability) -> augment (variants) -> extend (lead-in / lead-out frames) ->
build (FK tables); a stage whose key is absent is skipped.
Motion files: the reference's joblib .pkl (read by the static, non-executing parser
`pbhc_amd.utils.safe_pkl`) or an .npz with the same arrays.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib, motion_ingest
from .motion_augment import Augmentation, mirror_tables
from .motion_interp import Interpolation
from .motion_retarget import RetargetSettings
from .motion_screen import ContactDetection, Screening
from .utils import resume, rng_state, safe_pkl


def load_motion_file(path):
    """-> list of (name, clip dict) with root_trans_offset [F,3], pose_aa [F,Bx,3], fps, optional contact_mask [F,2]."""
    if os.path.isdir(path):
        out = []
        for f in sorted(os.listdir(path)):
            if f.endswith((".pkl", ".npz")):
                out.extend(load_motion_file(os.path.join(path, f)))
        return out
    if path.endswith(".npz"):
        z = np.load(path, allow_pickle=False)
        names = sorted({k.split("::")[0] for k in z.files})
        clips = []
        for n in names:
            c = {k.split("::")[1]: z[k] for k in z.files if k.startswith(n + "::")}
            c["fps"] = int(c["fps"])
            clips.append((n, c))
        return clips
    data = safe_pkl.load(path)
    return [(k, v) for k, v in data.items()]


def save_motion_npz(path, clips):
    arrs = {}
    for name, c in clips:
        for k in ("root_trans_offset", "pose_aa", "contact_mask"):
            if k in c:
                arrs[f"{name}::{k}"] = np.asarray(c[k])
        arrs[f"{name}::fps"] = np.int64(c["fps"])
    np.savez_compressed(path, **arrs)


def rebase_heading(clip, target_heading):
    """motion_lib_base.py:445-456 on the host, in float64 like the reference (scipy Rotation): heading_delta = target * inv(heading of the first
    root rotation); root pose_aa <- heading_delta * root rotation, root translation <- translation @ heading_delta^T."""
    from scipy.spatial.transform import Rotation as sRot

    pose = np.array(clip["pose_aa"], dtype=np.float32, copy=True)
    trans = np.asarray(clip["root_trans_offset"])
    q0 = sRot.from_rotvec(pose[0, 0].astype(np.float64)).as_quat()                     # xyzw
    # calc_heading_quat_inv (isaac_utils/rotations.py:296-306) in fp32 like the reference's torch call: rotate the x axis, atan2, -heading about z
    q = q0.astype(np.float32)
    w = q[3]
    v = np.array([1.0, 0.0, 0.0], np.float32)
    rot = v * (2.0 * w * w - 1.0) + np.cross(q[:3], v) * w * 2.0 + q[:3] * np.dot(q[:3], v) * 2.0
    heading = np.float32(np.arctan2(rot[1], rot[0]))
    hinv = np.array([0.0, 0.0, np.sin(-heading / 2.0), np.cos(-heading / 2.0)], dtype=np.float32)
    delta = sRot.from_quat(np.asarray(target_heading, dtype=np.float64)) * sRot.from_quat(hinv.astype(np.float64))
    pose[:, 0] = (delta * sRot.from_rotvec(pose[:, 0].astype(np.float64))).as_rotvec().astype(np.float32)
    out = dict(clip)
    out["pose_aa"] = pose
    out["root_trans_offset"] = (trans.astype(np.float64) @ delta.as_matrix().squeeze().T).astype(np.float32)
    return out


class MotionLib:
    def __init__(self, skeleton, clips, num_envs, device, max_len=-1, interpolation=None, augmentation=None, contact_detection=None,
                 screening=None, retarget=None):
        """clips: list of clip dicts (see load_motion_file).  max_len > 0: `load_motions` gives every env slot its own random crop of at most
        `max_len` frames of its clip (motion_lib_base.py:420-428) — the tables are then per SLOT (num_envs entries of max_len rows, allocated
        once so that the step kernel's pointers stay valid) instead of per unique clip.
        The optional stages, in the module docstring's order; None or not active: no launch.
        contact_detection / screening (motion_screen.ContactDetection / Screening): one pre-pass over the source clips, after the cut below,
        derives the contact masks of the clips that ship none (or of all, `overwrite`) into copies of the clip dicts — `contact_derived` —
        and fills `screen_report` (arrays over the source clips as given); `action: exclude` drops the unstable clips there.
        augmentation (motion_augment.Augmentation): every clip becomes V clips — itself, its mirror image, time-scaled copies: clip
        src * V + v is variant v of source clip src (`variant_source`, `variant_info`); everything downstream sees M * V ordinary clips.
        interpolation (motion_interp.Interpolation): every clip is cut to [clip_start:clip_end] on the host, first of all, and gets lead-in /
        lead-out frames from / to a default pose: lengths, tables and crops describe the extended clips.
        retarget (motion_retarget.RetargetSettings): before everything else, the clips that hold `keypoints` and no `pose_aa` are fitted on
        the device and become ordinary clips; `retarget_report` holds their indices and first / last loss."""
        clips, self.retarget_report = motion_ingest.retarget(clips, skeleton, device, retarget)
        if interpolation is not None:
            if interpolation.num_dof != skeleton.num_dof:
                raise _lib.PbhcError(f"interpolation was set up for {interpolation.num_dof} dofs, the skeleton has {skeleton.num_dof}")
            clips = [interpolation.trim(c) for c in clips]
        self.interpolation = interpolation if interpolation is not None and interpolation.active else None
        self.augmentation = augmentation if augmentation is not None and augmentation.active else None
        self.contact_detection = contact_detection if contact_detection is not None and contact_detection.active else None
        self.screening = screening if screening is not None and screening.active else None
        self.skeleton = skeleton
        self.device = torch.device(device)
        self.num_envs = num_envs
        self._csk = skeleton.to_c()
        self.row = motion_ingest.row_width(skeleton)
        self.contact_derived = [False] * len(clips)      # per source clip as given: its mask was derived here, not shipped
        self.screen_report = None
        self._screen_dist = self._screen_starts = None
        batch = None                                     # the pre-pass's upload: the build continues from it
        if self.contact_detection is not None or self.screening is not None:
            clips, batch = self._screen(clips)
        self.has_contact_mask = all("contact_mask" in c for c in clips)
        if batch is not None:
            motion_ingest.upload(clips, skeleton, self.device, self.has_contact_mask, batch)
        self.max_len = int(max_len)
        self.generator = None              # torch.Generator for the sampling draws (None: the global one, as the reference)
        self._clips = clips                              # the SOURCE clips (host arrays), kept for load_motions(target_heading=...) and extended_clips()
        self._built_clips = None
        frames = self._init_variants(clips)              # of every clip as the tables hold them: len(clips) * variants
        M = self._num_unique_motions
        # sampling hooks of the reference (setup_constants, motion_lib_base.py:109-118): per-unique-clip tensors a curriculum may write
        self._sampling_prob = torch.ones(M, device=self.device) / M
        self._termination_history = torch.zeros(M, device=self.device)
        self._success_rate = torch.zeros(M, device=self.device)
        self._sampling_history = torch.zeros(M, device=self.device)
        self._sampling_cdf = None          # double [M], written by update_sampling_device (clip_sampling only)
        # start_sampling only (init_start_sampling): per clip and phase bin, the decayed visit / failure histories, the start-bin law, its CDF
        self._start_visits = self._start_failures = self._start_prob = self._start_cdf = None
        self.slot_clip = torch.zeros(num_envs, dtype=torch.long, device=self.device)
        self.table = _lib.PbhcMotionTable()
        if self.max_len > 0 and any(F >= self.max_len for F in frames):
            self._init_slot_tables(self._ingest(clips, batch))
            return
        self.max_len = -1
        self._raw = None
        self.slot_table = self.slot_clip                 # the kernel's motion ids: unique-clip tables, slot -> clip
        self._build_unique_tables(clips, batch)

    def _init_variants(self, clips):
        """`variant_source`, `variant_info` and the mirror tables; the skeleton's symmetry is checked here, once, when the mirror is on
        -> the frame count of every clip after the augmentation and the extension"""
        aug, dev = self.augmentation, self.device
        self.mirror_body_perm = self.mirror_dof_perm = self.mirror_dof_sign = None
        self.mirror_asymmetry = None
        self._d_perm = None
        frames = [np.asarray(c["pose_aa"]).shape[0] for c in clips]
        if aug is None:
            self.variant_info = [(i, False, 1.0) for i in range(len(clips))]
        else:
            self.variant_info = [(i,) + aug.variant(v) for i in range(len(clips)) for v in range(aug.num_variants)]
            frames = motion_ingest.augment_frames(frames, aug)
            if aug.mirror:
                mt = mirror_tables(self.skeleton, aug.symmetry_tol)
                self.mirror_body_perm = torch.from_numpy(mt.body_perm).to(dev)
                self.mirror_dof_perm = torch.from_numpy(mt.dof_perm).to(dev)
                self.mirror_dof_sign = torch.from_numpy(mt.dof_sign).to(dev)
                self.mirror_asymmetry = mt.asymmetry
                self._d_perm = torch.from_numpy(mt.body_perm.astype(np.int32)).to(dev)
        self._num_unique_motions = len(self.variant_info)
        self.variant_source = torch.from_numpy(np.array([v[0] for v in self.variant_info], dtype=np.int64)).to(dev)
        return frames if self.interpolation is None else motion_ingest.extend_frames(frames, self.interpolation)

    def _screen(self, clips):
        """the pre-pass on the source clips -> (the clips the library keeps, those whose mask was derived as copies; their upload)"""
        cd = self.contact_detection
        derive = motion_ingest.derive_flags(clips, cd)
        batch = motion_ingest.upload(clips, self.skeleton, self.device, with_contact=False)
        self._screen_starts = batch.starts
        batch, self.screen_report, self._screen_dist, kept, masks = motion_ingest.screen(batch, self.skeleton, cd, self.screening, derive)
        if cd is not None:
            self.contact_derived = derive
        return [clips[i] if masks[i] is None else dict(clips[i], contact_mask=masks[i]) for i in kept], batch

    def stability_distance(self, i):
        """the per-frame distance between centre of mass and centre of pressure of source clip `i` (as given, before `exclude`) [F] float32"""
        if self._screen_dist is None:
            raise _lib.PbhcError("stability_distance: the library was built without robot.motion.screening")
        a, b = int(self._screen_starts[int(i)]), int(self._screen_starts[int(i) + 1])
        return self._screen_dist[a:b].cpu().numpy()

    def _ingest(self, clips, batch=None):
        """-> the clips as the tables hold them (`batch`: the upload of `clips`, if the pre-pass made it)"""
        return motion_ingest.ingest(clips if batch is None else batch, self._csk, self.device, self.has_contact_mask, self.augmentation, self._d_perm,
                                    self.interpolation)

    def extended_clips(self):
        """The library's clips as the tables were built from them — trimmed, every variant of `augmentation` (clip src * V + v), with the
        lead-in / lead-out frames — as host clip dicts (root_trans_offset, pose_aa, fps, contact_mask if the library has one): what
        `save_motion_npz` or the deploy side needs."""
        if self.interpolation is None and self.augmentation is None:
            return [dict(c) for c in self._clips]
        return self._ingest(self._clips).to_host_clips()

    def _build_unique_tables(self, clips, batch=None, into=None):
        """ingestion + `motion_ingest.build` of every unique clip.  `into`: rebuild in place (same row count)."""
        batch = self._ingest(clips, batch)
        rows, dt, lengths = motion_ingest.build(batch, self._csk, out=into)
        if into is not None:
            return
        self.frames = rows
        self.length_starts = batch.d_starts[:-1].contiguous()
        self.num_frames = torch.tensor(batch.nframes, dtype=torch.int32, device=self.device)
        self._motion_dt, self._motion_lengths = dt, lengths
        dt0 = 1.0 / batch.fps[0]
        self._fill_table(len(batch.nframes), batch.nframes[0], dt0, dt0 * (batch.nframes[0] - 1))

    def _fill_table(self, num_entries, f0, dt0, len0):
        self.table.frames = self.frames.data_ptr()
        self.table.row = self.row
        self.table.num_motions = num_entries
        self.table.length_starts = self.length_starts.data_ptr()
        self.table.num_frames = self.num_frames.data_ptr()
        self.table.motion_dt = self._motion_dt.data_ptr()
        self.table.motion_len = self._motion_lengths.data_ptr()
        self.table.single_num_frames = int(f0)
        self.table.single_dt = float(torch.tensor(dt0, dtype=torch.float32))
        self.table.single_len = float(torch.tensor(len0, dtype=torch.float32))

    # ---- per-slot crops (max_len) -----------------------------------------------------------
    def _init_slot_tables(self, batch):
        """crops are drawn from the clips as the tables would hold them (the variants, the extended clips), as from the reference's
        processed pickle"""
        N, K, dev = self.num_envs, self.max_len, self.device
        self._raw = [batch.slice(i) for i in range(len(batch.nframes))]
        self.frames = torch.zeros(N * K, self.row, device=dev)
        self.length_starts = (torch.arange(N, dtype=torch.int32, device=dev) * K).contiguous()
        self.num_frames = torch.ones(N, dtype=torch.int32, device=dev)
        self._motion_dt = torch.ones(N, dtype=torch.float32, device=dev)
        self._motion_lengths = torch.zeros(N, dtype=torch.float32, device=dev)
        self.slot_table = torch.arange(N, dtype=torch.long, device=dev)          # slot i reads table entry i
        self._scratch = motion_ingest.build_scratch(self.skeleton, K, dev)
        self.crop_starts = torch.zeros(N, dtype=torch.long)
        self._fill_table(max(N, 2), 1, 1.0, 0.0)          # >= 2: the kernel reads the per-entry arrays, never the by-value single-clip meta

    def _build_slot_crops(self, crop_starts=None):
        """FK + filtered velocities of every slot's crop, written in place (the reference crops BEFORE FK, so the velocity filter sees the
        crop's own edges, motion_lib_base.py:420-434)."""
        import random

        rnd = getattr(self, "pyrand", None) or random
        N, K = self.num_envs, self.max_len
        clip_of = self.slot_clip.tolist()
        nf, dts, lens = [], [], []
        st = _lib.current_stream()
        for i in range(N):
            pose, trans, contact, fps = self._raw[clip_of[i]]
            F = pose.shape[0]
            if F < K:
                a, b = 0, F
            else:
                a = int(crop_starts[i]) if crop_starts is not None else rnd.randint(0, F - K)
                b = a + K
            self.crop_starts[i] = a
            n = b - a
            _lib.check(_lib.lib().pbhc_motion_build(C.byref(self._csk), _lib.ptr(pose[a:b]), _lib.ptr(trans[a:b]), _lib.ptr(contact[a:b]) if contact is not None else None,
                                                    n, 1.0 / fps, _lib.ptr(self.frames[i * K:i * K + n]), _lib.ptr(self._scratch), st), "pbhc_motion_build")
            nf.append(n); dts.append(1.0 / fps); lens.append(1.0 / fps * (n - 1))
        self.num_frames.copy_(torch.tensor(nf, dtype=torch.int32))
        self._motion_dt.copy_(torch.tensor(dts, dtype=torch.float32))
        self._motion_lengths.copy_(torch.tensor(lens, dtype=torch.float32))

    @classmethod
    def from_config(cls, mcfg, skeleton, num_envs, device, max_len=-1, robot=None):
        """mcfg = config.robot.motion (motion_file = .pkl / .npz / directory); max_len: see __init__.  mcfg.interpolation (absent by default):
        see motion_interp.Interpolation.from_config; robot = config.robot supplies its default joints and the dof names.  mcfg.augmentation
        (absent by default): see motion_augment.Augmentation.from_config.  mcfg.contact_detection, mcfg.screening (absent by default): see
        motion_screen.ContactDetection.from_config / Screening.from_config.  mcfg.retarget (absent by default): see
        motion_retarget.RetargetSettings.from_config; `limits: mjcf` reads the asset's MJCF."""
        path = str(mcfg.motion_file)
        if not os.path.isabs(path) and not os.path.exists(path):
            path = os.path.join(_lib.ROOT, path)
        clips = [c for _, c in load_motion_file(path)]
        if mcfg.get("motion_lib_type", "origin") == "WJX" and len(clips) != 1:
            raise _lib.PbhcError("Not Allowed to load more than one motion!")     # motion_lib_robot_WJX.py:202
        augmentation = Augmentation.from_config(mcfg.get("augmentation", None))      # (every from_config: None for an absent key)
        if augmentation is not None and augmentation.active and mcfg.get("motion_lib_type", "origin") == "WJX":
            raise _lib.PbhcError("robot.motion.augmentation with motion_lib_type WJX: a v1 library is ONE clip, the variants would make it "
                                 f"{augmentation.num_variants}")
        rnode, mjcf = mcfg.get("retarget", None), None
        if rnode is not None and rnode.get("enable", False) and rnode.get("limits", "mjcf") == "mjcf":
            mjcf = os.path.join(str(mcfg.asset.assetRoot), str(mcfg.asset.assetFileName))   # the asset the skeleton came from, when an MJCF
            if not os.path.isabs(mjcf) and not os.path.exists(mjcf):
                mjcf = os.path.join(_lib.ROOT, mjcf)
            mjcf = mjcf if mjcf.endswith(".xml") else None
        retarget = RetargetSettings.from_config(rnode, mjcf=mjcf)
        return cls(skeleton, clips, num_envs, device, max_len=max_len, augmentation=augmentation, retarget=retarget,
                   interpolation=Interpolation.from_config(mcfg.get("interpolation", None), skeleton.num_dof, robot=robot),
                   contact_detection=ContactDetection.from_config(mcfg.get("contact_detection", None)),
                   screening=Screening.from_config(mcfg.get("screening", None)))

    # ---- slot -> clip assignment (load_motions, motion_lib_base.py:293-305) -----------------
    def load_motions(self, random_sample=True, start_idx=0, max_len=-1, target_heading=None, sampling_prob=None, crop_starts=None):
        """Slot -> clip assignment; the per-clip FK tables were built once at construction (the reference re-runs FK for every slot here).
        With a library built for `max_len` crops, every slot's crop is re-drawn and its table rebuilt (crop_starts: fixed starts, tests).
        `target_heading` (xyzw quaternion): every clip is yawed so that its first frame faces that heading (root rotation and translation,
        motion_lib_base.py:445-456) and the tables are rebuilt in place."""
        if target_heading is not None:
            if self.max_len > 0:
                raise NotImplementedError("load_motions(target_heading) with max_len crops")
            if self.augmentation is not None and self.augmentation.mirror:
                raise _lib.PbhcError("load_motions(target_heading) with robot.motion.augmentation.mirror: the clips are rebased before the "
                                     "variants are made, so a mirrored variant would face the mirrored heading, not the target")
            self._build_unique_tables([rebase_heading(c, target_heading) for c in self._clips], into=self.frames)
        if max_len != -1 and max_len != self.max_len and (self.max_len != -1 or any(int(f) >= max_len for f in self.num_frames.tolist())):
            raise _lib.PbhcError(f"load_motions(max_len={max_len}): the library was built with max_len={self.max_len} (pass robot.motion.motion_max_len at construction)")
        # in place: the step kernel holds the pointer of this tensor
        if random_sample:
            prob = self._sampling_prob if sampling_prob is None else sampling_prob
            self.slot_clip.copy_(torch.multinomial(prob, num_samples=self.num_envs, replacement=True, generator=self.generator))
        else:
            self.slot_clip.copy_(torch.remainder(torch.arange(self.num_envs, device=self.device) + start_idx, self._num_unique_motions))
        self._curr_motion_ids = self.slot_clip
        if self.max_len > 0:
            self._build_slot_crops(crop_starts)
        return self.slot_clip

    # ---- failure-weighted clip sampling on the device (env.config.clip_sampling; csrc/pbhc_clip_stats.hip) ------
    def _cdf(self):
        if self._sampling_cdf is None:
            self._sampling_cdf = torch.zeros(self._num_unique_motions, dtype=torch.float64, device=self.device)
        return self._sampling_cdf

    def update_sampling_device(self, window, decay, prior_episodes, uniform_floor):
        """Fold `window` ([M,4] int64: episodes, failures, ...; cleared here) into the four sampling hooks and the CDF of `_sampling_prob`:
        E <- decay E + e, F <- decay F + f, r = (F + prior) / (E + prior), p = (1 - floor) r / sum(r) + floor / M."""
        M = self._num_unique_motions
        _lib.require_gpu_tensor(window, "window", torch.int64, (M, 4))
        _lib.check(_lib.lib().pbhc_clip_sampling_update(_lib.ptr(window), _lib.ptr(self._sampling_history), _lib.ptr(self._termination_history),
                                                        _lib.ptr(self._success_rate), _lib.ptr(self._sampling_prob), _lib.ptr(self._cdf()), M,
                                                        float(decay), float(prior_episodes), float(uniform_floor), _lib.current_stream()),
                   "pbhc_clip_sampling_update")

    def sample_slots_device(self, seed, draw_index):
        """The random slot -> clip assignment of load_motions drawn on the device from the CDF update_sampling_device left, restatable bit
        for bit: slot j takes the first clip whose CDF exceeds u_j * total, u_j = u01(philox4x32(seed; j, draw_index, 20, 0)[0]).  In place
        (the step kernel holds the pointer); crops are re-drawn as in load_motions."""
        if self._sampling_cdf is None:
            raise _lib.PbhcError("sample_slots_device before update_sampling_device")
        _lib.check(_lib.lib().pbhc_clip_sample_slots(_lib.ptr(self._sampling_cdf), self._num_unique_motions, int(seed), int(draw_index) & 0xFFFFFFFF,
                                                     _lib.ptr(self.slot_clip), self.num_envs, _lib.current_stream()), "pbhc_clip_sample_slots")
        self._curr_motion_ids = self.slot_clip
        if self.max_len > 0:
            self._build_slot_crops()
        return self.slot_clip

    # ---- failure-weighted start-time sampling on the device (env.config.start_sampling; csrc/pbhc_start_sampling.hip) ------
    def init_start_sampling(self, bins):
        """`_start_visits`, `_start_failures`, `_start_prob` [M,K] float32 and `_start_cdf` [M,K] double for K = `bins` phase bins per unique
        clip: empty histories, the uniform law.  Refused for a library of max_len crops: a slot's times are relative to ITS crop there."""
        if self.max_len > 0:
            raise _lib.PbhcError("env.config.start_sampling / start_statistics with robot.motion.motion_max_len crops: slot times are "
                                 "crop-relative, a phase bin of the clip means nothing there")
        M, K, dev = self._num_unique_motions, int(bins), self.device
        self._start_visits = torch.zeros(M, K, device=dev)
        self._start_failures = torch.zeros(M, K, device=dev)
        self._start_prob = torch.full((M, K), 1.0 / K, device=dev)
        self._start_cdf = torch.cumsum(self._start_prob.double(), dim=1).contiguous()

    def update_start_sampling_device(self, window, decay, prior_episodes, uniform_floor, lookahead_bins, lookahead_decay):
        """Fold `window` ([M,K,2] int64: visit differences, failures; cleared here) into the start-sampling tables: V <- decay V + visits,
        F <- decay F + failures, r = (F + prior) / (V + prior), w_b = sum_{u < H} lambda^u r_{b+u}, p = (1 - floor) w / sum(w) + floor / K."""
        if self._start_cdf is None:
            raise _lib.PbhcError("update_start_sampling_device before init_start_sampling")
        M, K = self._start_prob.shape
        _lib.require_gpu_tensor(window, "window", torch.int64, (M, K, 2))
        _lib.check(_lib.lib().pbhc_start_sampling_update(_lib.ptr(window), _lib.ptr(self._start_visits), _lib.ptr(self._start_failures),
                                                         _lib.ptr(self._start_prob), _lib.ptr(self._start_cdf), M, K, float(decay),
                                                         float(prior_episodes), float(uniform_floor), int(lookahead_bins), float(lookahead_decay),
                                                         _lib.current_stream()), "pbhc_start_sampling_update")

    def draw_start_times_device(self, start_time, seed, counter_ptr, salt, reset_buf=None, stream=None):
        """start_time[j] <- (bin + u2) / K * clip length of slot j, bin from `_start_cdf` (k_start_draw, Philox stream 21 keyed by the device
        step counter at `counter_ptr` and `salt`), for every slot, or for those with reset_buf != 0.  In place; capturable."""
        M, K = self._start_prob.shape
        _lib.check(_lib.lib().pbhc_start_draw(_lib.ptr(self._start_cdf), _lib.ptr(self._motion_lengths), _lib.ptr(self.slot_clip),
                                              None if reset_buf is None else _lib.ptr(reset_buf), None, self.num_envs, M, K, int(seed), counter_ptr,
                                              int(salt) & 0xFFFFFFFF, _lib.ptr(start_time), _lib.current_stream() if stream is None else stream),
                   "pbhc_start_draw")

    # ---- exact resume: the slot -> clip table with its crops, the sampling hooks, the start-time tables -----------------
    def _state_tensors(self):
        return {"slot_clip": self.slot_clip, "_sampling_prob": self._sampling_prob, "_termination_history": self._termination_history,
                "_success_rate": self._success_rate, "_sampling_history": self._sampling_history, "_start_visits": self._start_visits,
                "_start_failures": self._start_failures, "_start_prob": self._start_prob, "_start_cdf": self._start_cdf}

    def clip_frame_counts(self):
        """the frame count of every clip as the tables hold it (host list; one device -> host copy on first use)"""
        if getattr(self, "_clip_frames", None) is None:
            self._clip_frames = [int(r[0].shape[0]) for r in self._raw] if self.max_len > 0 else [int(f) for f in self.num_frames.tolist()]
        return self._clip_frames

    def state_dict(self):
        """What a resumed run needs of the library, as copies.  The built tables are a function of the config and are not saved; the
        per-slot crop tables are rebuilt from the saved crop starts."""
        sd = resume.snapshot(self._state_tensors())
        sd["_sampling_cdf"] = None if self._sampling_cdf is None else self._sampling_cdf.clone()
        sd["crop_starts"] = self.crop_starts.clone() if self.max_len > 0 else None
        pyrand = getattr(self, "pyrand", None)
        sd.update(version=resume.STATE_VERSION, num_envs=int(self.num_envs), num_clips=int(self._num_unique_motions), max_len=int(self.max_len),
                  pyrand=None if pyrand is None else rng_state.pack_python(pyrand.getstate()))
        return sd

    def check_state_dict(self, sd):
        """everything `load_state_dict` would refuse, without writing anything"""
        what = "MotionLib.load_state_dict"
        resume.check_version(sd, what)
        for k, here in (("num_envs", int(self.num_envs)), ("num_clips", int(self._num_unique_motions)), ("max_len", int(self.max_len))):
            resume.check_equal(what, k, int(sd[k]), here)
        resume.check_tensors(what, sd, self._state_tensors())
        if self.max_len > 0:
            resume.check_tensors(what, sd, {"crop_starts": self.crop_starts})
        if (sd["pyrand"] is None) != (getattr(self, "pyrand", None) is None):
            raise _lib.PbhcError(f"{what}: pyrand differs: the saved state has {'none' if sd['pyrand'] is None else 'a generator state'}, this "
                                 f"run has {'none' if getattr(self, 'pyrand', None) is None else 'a generator'} (another rank?)")

    def load_state_dict(self, sd):
        self.check_state_dict(sd)
        resume.restore(sd, self._state_tensors())
        if sd["_sampling_cdf"] is not None:
            self._cdf().copy_(sd["_sampling_cdf"].to(self.device))
        self._curr_motion_ids = self.slot_clip
        if self.max_len > 0:
            self._build_slot_crops(sd["crop_starts"].cpu())         # (fixed starts: nothing is drawn)
        if sd["pyrand"] is not None:
            self.pyrand.setstate(rng_state.unpack_python(sd["pyrand"]))

    def built_clip(self, clip_id):
        """clip `clip_id` of the library as a host clip dict: the source clip itself without `augmentation`, else that variant (with the
        lead-in / lead-out frames), fetched from the device once"""
        if self.augmentation is None:
            return self._clips[int(clip_id)]
        if self._built_clips is None:
            self._built_clips = self.extended_clips()
        return self._built_clips[int(clip_id)]

    def get_motion_length(self, slot_ids=None):
        if slot_ids is None:
            return self._motion_lengths[self.slot_table]
        return self._motion_lengths[self.slot_table[slot_ids]]

    def sample_time(self, slot_ids):
        # motion_lib_base.py:486-495
        phase = torch.rand(slot_ids.shape, device=self.device, generator=self.generator)
        return phase * self.get_motion_length(slot_ids)

    def get_motion_state(self, slot_ids, motion_times, offset=None):
        """motion_lib_base.py:123-259; returns the reference's dict keys (views of one packed buffer)."""
        n = slot_ids.shape[0]
        D, Bx, B = self.skeleton.num_dof, self.skeleton.num_bodies_ext, self.skeleton.num_bodies
        ids = self.slot_table[slot_ids].contiguous()
        times = motion_times.to(torch.float32).contiguous()
        off = None if offset is None else offset.to(torch.float32).contiguous()
        out = torch.empty(n, self.row, device=self.device)
        _lib.check(_lib.lib().pbhc_motion_state(C.byref(self.table), Bx, D, _lib.ptr(ids), _lib.ptr(times), _lib.ptr(off), n,
                                                _lib.ptr(out), _lib.current_stream()), "pbhc_motion_state")
        o_pos = 2 * D + 2
        o_rot, o_vel, o_ang = o_pos + 3 * Bx, o_pos + 7 * Bx, o_pos + 10 * Bx
        pos = out[:, o_pos:o_rot].view(n, Bx, 3)
        rot = out[:, o_rot:o_vel].view(n, Bx, 4)
        vel = out[:, o_vel:o_ang].view(n, Bx, 3)
        ang = out[:, o_ang:].view(n, Bx, 3)
        res = dict(root_pos=pos[:, 0], root_rot=rot[:, 0], dof_pos=out[:, :D], root_vel=vel[:, 0], root_ang_vel=ang[:, 0],
                   dof_vel=out[:, D:2 * D], rg_pos=pos[:, :B], rb_rot=rot[:, :B], body_vel=vel[:, :B], body_ang_vel=ang[:, :B],
                   rg_pos_t=pos, rg_rot_t=rot, body_vel_t=vel, body_ang_vel_t=ang)
        if self.has_contact_mask:
            res["contact_mask"] = out[:, 2 * D:2 * D + 2]
        return res
