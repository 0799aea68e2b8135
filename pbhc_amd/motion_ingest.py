"""The motion library's ingestion pipeline: host clip dicts -> one `ClipBatch` on the device -> packed table rows.

    [retarget] -> upload -> [screen] -> [augment] -> [extend] -> build

Every stage is a plain function from a batch to a batch (`build`: to the rows); the settings objects (`motion_screen`, `motion_augment`,
`motion_interp`) say what a stage does, this module is how its one launch is fed.  `MotionLib`, the export tools and the probes all run
these functions.  The host-only arithmetic (`clip_starts`, `augment_frames`, `extend_frames`, `derive_flags`, the checks of `upload`) needs no GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, motion_screen


def clip_starts(nframes):
    """first row of every clip in the concatenated arrays, and the total: int32 [M + 1]"""
    return np.concatenate([[0], np.cumsum(nframes)]).astype(np.int32)


def augment_frames(nframes, augmentation):
    """frames of the len(nframes) * V clips `augment` makes: clip src * V + v is variant v of clip src"""
    return [Fo for i, F in enumerate(nframes) for Fo in augmentation.variant_frames(int(F), f"clip {i}")]


def extend_frames(nframes, interpolation):
    """frames of the clips `extend` makes"""
    return [int(F) + interpolation.added for F in nframes]


def derive_flags(clips, contact_detection):
    """per clip: `screen` derives its contact mask (the clip ships none, or `overwrite`)"""
    cd = contact_detection
    return [cd is not None and (cd.overwrite or "contact_mask" not in c) for c in clips]


class ClipBatch:
    """The clips of a library, concatenated on the device: pose [total, Bx, 3], trans [total, 3], contact [total, 2] or None; nframes and
    fps are host lists, one int per clip; starts = clip_starts(nframes), `d_starts` its device copy (made on first use)."""

    def __init__(self, pose, trans, contact, nframes, fps):
        self.pose, self.trans, self.contact = pose, trans, contact
        self.nframes, self.fps = list(nframes), list(fps)
        self.starts = clip_starts(self.nframes)
        self._d_starts = None

    @property
    def d_starts(self):
        if self._d_starts is None:
            self._d_starts = torch.from_numpy(self.starts).to(self.pose.device)
        return self._d_starts

    def slice(self, i):
        """-> (pose, trans, contact or None, fps) of clip i: views"""
        a, b = int(self.starts[i]), int(self.starts[i + 1])
        return self.pose[a:b], self.trans[a:b], None if self.contact is None else self.contact[a:b], self.fps[i]

    def to_host_clips(self):
        """-> host clip dicts (root_trans_offset, pose_aa, fps, contact_mask if the batch has one): one copy per array, cut on the host"""
        host = ClipBatch(self.pose.cpu().numpy(), self.trans.cpu().numpy(), None if self.contact is None else self.contact.cpu().numpy(),
                         self.nframes, self.fps)
        out = []
        for i in range(len(self.nframes)):
            pose, trans, contact, fps = host.slice(i)
            out.append(dict(root_trans_offset=trans.copy(), pose_aa=pose.copy(), fps=fps))
            if contact is not None:
                out[-1]["contact_mask"] = contact.copy()
        return out


def retarget(clips, skeleton, device, settings):
    """The first stage, `robot.motion.retarget`: the clip dicts that hold `keypoints` and no `pose_aa` are fitted in ONE batch
    (`motion_retarget.fit`) and become ordinary clips (pose_aa, root_trans_offset, fps; no contact_mask, so that `contact_detection` can
    derive it); every other clip passes through as the object it is.  settings None or not enabled: the list as given, no launch.
    -> (clips, report or None); report: `clips` (indices of the fitted clips), `first_loss`, `last_loss` [fitted] in metres."""
    if settings is None or not settings.active:
        return clips, None
    todo = [i for i, c in enumerate(clips) if "keypoints" in c and "pose_aa" not in c]
    if not todo:
        return clips, dict(clips=np.zeros(0, np.int64), first_loss=np.zeros(0), last_loss=np.zeros(0))
    from . import motion_retarget

    batch, _, _, hist = motion_retarget.fit([clips[i] for i in todo], skeleton, settings, device)
    hist = hist.cpu().numpy().astype(np.float64)
    out = list(clips)
    for i, fitted in zip(todo, batch.to_host_clips()):
        out[i] = fitted
    return out, dict(clips=np.asarray(todo, np.int64), first_loss=hist[0], last_loss=hist[-1])


def _csk(skeleton):
    """a stage takes the Skeleton or its C struct (a caller with many launches converts once)"""
    return skeleton if isinstance(skeleton, _lib.PbhcSkeleton) else skeleton.to_c()


def _cat(clips, key, device, num_bodies_ext=None):
    arrs = [np.asarray(c[key], dtype=np.float32) for c in clips]
    if num_bodies_ext is not None:
        arrs = [a[:, :num_bodies_ext] for a in arrs]
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(arrs, axis=0))).to(device)


def upload(clips, skeleton, device, with_contact, batch=None):
    """THE place that checks (body count, contact-mask shape), concatenates and uploads host clips.  batch: the upload of these very clips
    without masks (`screen` returned it) — only the masks are added to it, in place."""
    Bx = skeleton.num_bodies_ext
    for c in clips:
        if np.asarray(c["pose_aa"]).shape[1] < Bx:
            raise _lib.PbhcError(f"pose_aa has {np.asarray(c['pose_aa']).shape[1]} bodies, skeleton needs {Bx}")
        if with_contact and tuple(np.asarray(c["contact_mask"]).shape) != (np.asarray(c["pose_aa"]).shape[0], 2):
            raise _lib.PbhcError(f"contact mask shape {tuple(np.asarray(c['contact_mask']).shape)} is not supported")
    if batch is None:
        batch = ClipBatch(_cat(clips, "pose_aa", device, Bx), _cat(clips, "root_trans_offset", device), None,
                          [np.asarray(c["pose_aa"]).shape[0] for c in clips], [int(c["fps"]) for c in clips])
    if with_contact:
        batch.contact = _cat(clips, "contact_mask", device)
    return batch


def screen(batch, skeleton, contact_detection, screening, derive):
    """The pre-pass of `contact_detection` and `screening` on the source clips: the per-frame launch (`pbhc_motion_screen_frames`: FK, the
    two foot positions, the stability distance) and the per-clip one (`pbhc_motion_screen_clips`: mask rows, report rows), two small
    results read back.  derive: per clip, make its mask.
    -> (the kept clips' batch, report or None, per-frame dist [total] or None, kept (new index -> old), masks)
    masks: per clip of `batch`, its derived mask as a host array [F, 2], or None; the caller attaches them to its clip dicts and uploads
    the library's masks from there (`upload(..., batch=)`), shipped and derived alike: the returned batch has none.
    report (screening only): stable, first_dist, last_dist, max_dist, unstable_share, max_gap [M] over the clips of `batch`, and kept.
    dist (screening only) is over the clips of `batch` as given, before `exclude`."""
    cd, scr, dev = contact_detection, screening, batch.pose.device
    derive = np.asarray(derive, dtype=np.int32)
    params = motion_screen.to_c(cd, scr, skeleton)         # (resolves the foot names: an unknown one is refused before any launch)
    d_mass = d_com = None
    if scr is not None:
        scr.check_skeleton(skeleton)
        d_mass, d_com = torch.from_numpy(skeleton.body_mass).to(dev), torch.from_numpy(np.ascontiguousarray(skeleton.body_com)).to(dev)
    M, starts, total = len(batch.nframes), batch.starts, int(batch.starts[-1])
    contact = cd is not None and bool(derive.any())
    d_foot = torch.empty(total, 2, 3, device=dev) if contact else None
    d_mask = torch.zeros(total, 2, device=dev) if contact else None
    d_dist = torch.empty(total, device=dev) if scr is not None else None
    d_ground = torch.empty(M, device=dev) if scr is not None else None
    d_report = torch.zeros(M, _lib.K["PBHC_SCREEN_REPORT"], device=dev) if scr is not None else None
    if contact or scr is not None:
        st, d_derive = _lib.current_stream(), torch.from_numpy(derive).to(dev)
        _lib.check(_lib.lib().pbhc_motion_screen_frames(C.byref(_csk(skeleton)), _lib.ptr(batch.pose), _lib.ptr(batch.trans), total, M, _lib.ptr(batch.d_starts),
                                                        params, _lib.ptr(d_mass), _lib.ptr(d_com), _lib.ptr(d_ground), _lib.ptr(d_foot), _lib.ptr(d_dist), st),
                   "pbhc_motion_screen_frames")
        _lib.check(_lib.lib().pbhc_motion_screen_clips(_lib.ptr(d_foot), _lib.ptr(d_dist), total, M, _lib.ptr(batch.d_starts), _lib.ptr(d_derive), params,
                                                       _lib.ptr(d_mask), _lib.ptr(d_report), st), "pbhc_motion_screen_clips")
    masks = [None] * M
    if contact:
        mask = d_mask.cpu().numpy()                        # (the copy synchronises: the staging tensors above may die with this scope)
        for i in np.flatnonzero(derive):
            masks[i] = mask[starts[i]:starts[i + 1]].copy()
    report, kept = None, list(range(M))
    if scr is not None:
        rep = d_report.cpu().numpy().astype(np.float64)
        kept = motion_screen.kept_clips(rep[:, 0] != 0.0, scr.action)
        report = dict(stable=rep[:, 0] != 0.0, first_dist=rep[:, 1], last_dist=rep[:, 2], max_dist=rep[:, 3], unstable_share=rep[:, 4],
                      max_gap=rep[:, 5].astype(np.int64), kept=np.asarray(kept, dtype=np.int64))
    if len(kept) < M:                                      # the kept clips' frames, gathered on the device
        rows = torch.from_numpy(np.concatenate([np.arange(starts[i], starts[i + 1]) for i in kept])).to(dev)
        batch = ClipBatch(batch.pose.index_select(0, rows), batch.trans.index_select(0, rows), None, [batch.nframes[i] for i in kept],
                          [batch.fps[i] for i in kept])
    return batch, report, d_dist, kept, masks


def _resample(entry, what, batch, skeleton, out_nframes, out_fps, params, *extra):
    """the launch `augment` and `extend` share: clip-wise maps of the concatenated arrays, (in, out) start arrays, one parameter struct"""
    dev, total_out = batch.pose.device, sum(out_nframes)
    out = ClipBatch(torch.empty(total_out, skeleton.num_bodies_ext, 3, device=dev), torch.empty(total_out, 3, device=dev),
                    torch.empty(total_out, 2, device=dev) if batch.contact is not None else None, out_nframes, out_fps)
    _lib.check(entry(C.byref(_csk(skeleton)), _lib.ptr(batch.pose), _lib.ptr(batch.trans), _lib.ptr(batch.contact), int(batch.starts[-1]), len(batch.nframes),
                     _lib.ptr(batch.d_starts), _lib.ptr(out.d_starts), total_out, params, *extra, _lib.ptr(out.pose), _lib.ptr(out.trans),
                     _lib.ptr(out.contact), _lib.current_stream()), what)
    # no synchronisation: the inputs, the start arrays and the default joints die with the caller's scope, and the caching allocator hands
    # their memory out again on this same stream only, behind the launch
    return out


def augment(batch, skeleton, augmentation, perm):
    """Every variant of every clip in ONE launch (`pbhc_motion_augment_batch`) -> the len(batch.nframes) * V clips.
    perm: `mirror_tables(...).body_perm` as int32 on the device (None without the mirror)."""
    V = augmentation.num_variants
    return _resample(_lib.lib().pbhc_motion_augment_batch, "pbhc_motion_augment_batch", batch, skeleton, augment_frames(batch.nframes, augmentation),
                     [f for f in batch.fps for _ in range(V)], augmentation.to_c(), _lib.ptr(perm))


def extend(batch, skeleton, interpolation):
    """The lead-in / lead-out frames of every clip in ONE launch (`pbhc_motion_extend_batch`) -> the extended clips"""
    params, d_dof = interpolation.to_c(batch.pose.device)  # (d_dof: the default joints the struct points to, alive across the launch)
    return _resample(_lib.lib().pbhc_motion_extend_batch, "pbhc_motion_extend_batch", batch, skeleton, extend_frames(batch.nframes, interpolation),
                     batch.fps, params)


def ingest(clips_or_batch, skeleton, device, with_contact, augmentation=None, perm=None, interpolation=None):
    """upload -> augment -> extend: the clips as the tables hold them.  A `ClipBatch` (the screen's) is taken as the upload; the settings
    are None for a stage that is off."""
    batch = clips_or_batch if isinstance(clips_or_batch, ClipBatch) else upload(clips_or_batch, skeleton, device, with_contact)
    if augmentation is not None:                           # variants first: the lead-in / lead-out frames are added to each at full length
        batch = augment(batch, skeleton, augmentation, perm)
    if interpolation is not None:                          # lead-in / lead-out frames: the build sees the extended clips
        batch = extend(batch, skeleton, interpolation)
    return batch


def row_width(skeleton):
    """floats of a packed row: [dof_pos D | dof_vel D | contact 2 | pos Bx*3 | rot Bx*4 | vel Bx*3 | ang Bx*3]"""
    return 2 * skeleton.num_dof + 2 + 13 * skeleton.num_bodies_ext


def build_scratch(skeleton, num_frames, device):
    """the scratch `pbhc_motion_build` / `pbhc_motion_build_batch` need for `num_frames` frames"""
    return torch.empty(num_frames * skeleton.num_bodies_ext * 14, device=device)


def build(batch, skeleton, out=None):
    """FK + filtered velocities of EVERY clip in one launch set (`pbhc_motion_build_batch`): the kernels stop velocities / the Gaussian
    filter at clip boundaries — no per-clip launch, copy or synchronisation (the reference runs a Python FK per env slot).
    out: rows to write in place ([total, row_width]).  -> (rows, dt per clip [M], length in seconds per clip [M])"""
    dev, M, total = batch.pose.device, len(batch.nframes), int(batch.starts[-1])
    dts = [1.0 / f for f in batch.fps]
    d_fc = torch.from_numpy(np.repeat(np.arange(M, dtype=np.int32), batch.nframes)).to(dev)                     # the clip of every frame
    d_dt = torch.tensor(dts, dtype=torch.float32, device=dev)
    rows = torch.empty(total, row_width(skeleton), device=dev) if out is None else out
    assert rows.shape[0] == total
    scratch = build_scratch(skeleton, total, dev)
    _lib.check(_lib.lib().pbhc_motion_build_batch(C.byref(_csk(skeleton)), _lib.ptr(batch.pose), _lib.ptr(batch.trans), _lib.ptr(batch.contact), total, M,
                                                  _lib.ptr(d_fc), _lib.ptr(batch.d_starts), _lib.ptr(d_dt), _lib.ptr(rows), _lib.ptr(scratch),
                                                  _lib.current_stream()), "pbhc_motion_build_batch")
    torch.cuda.current_stream().synchronize()              # ONE synchronisation: the staging tensors above die with this scope
    return rows, d_dt, torch.tensor([dt * (F - 1) for dt, F in zip(dts, batch.nframes)], dtype=torch.float32, device=dev)
