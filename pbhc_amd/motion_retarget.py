"""`robot.motion.retarget`: key-point trajectories -> robot joint angles, on the device, as the first stage of the ingestion pipeline.

The reference does this offline, one clip at a time on the CPU (smpl_retarget/phc_retarget/fit_smpl_motion.py:137-179): gradient descent
through `Humanoid_Batch.fk_batch` on the distance between matched robot bodies and SMPL key points already scaled to the robot.  Here the
whole library is fitted at once (`pbhc_retarget_fit`, csrc/pbhc_retarget.hip; the definition and the two differences from the reference —
the filter's edge rule, no mesh-based height shift — are in DESIGN §8 "Retargeting").  The SMPL body model itself is out of scope: the input
is the key-point array the reference calls `joints` after its scaling.

A key-point clip is a dict with `keypoints` [F, K, 3] (world frame), `fps`, and optionally `root_trans_offset` [F, 3] (default: the key
point matched to the root body), `root_rot_init` [F, 3] rotation vectors (default: yaw only, from `heading_from`) and `keypoint_names` [K].

This module is the host side: the parsed settings, the MJCF joint limits, the heading rule and the launches.  There is no CPU implementation
of the fit.
"""
from __future__ import annotations

import ctypes as C
import math
import xml.etree.ElementTree as ET
from dataclasses import dataclass, field

import numpy as np

from . import _lib

KEY = "robot.motion.retarget"
KEYS = ("enable", "joint_matches", "iterations", "dof_lr", "root_lr", "filter", "filter_sigma", "limits", "heading_from", "ground")
GROUNDS = ("none", "first_frame_min_body")
UNLIMITED = 1.0e30                                 # a hinge without a `range` (MuJoCo: not limited)


def mjcf_limits(path, skeleton):
    """The hinge `range` attributes of an MJCF as [D, 2] float64 radians in the skeleton's dof order (the joints `Skeleton.from_mjcf` takes
    the axes from); a hinge without a range is (-UNLIMITED, UNLIMITED).  `<compiler angle=...>` other than "radian" means degrees (MuJoCo's
    default).  Only the joint element's own `range` / `limited` attributes are read: a range inherited from a `<default>` class is not seen
    (the hinge counts as unlimited), and a `range` without `limited` counts as limited whatever `<compiler autolimits>` says."""
    root = ET.parse(path).getroot()
    world = root.find("worldbody")
    if world is None:
        raise _lib.PbhcError(f"{path}: no <worldbody>")
    joints = world.findall(".//joint")
    first = joints[0].attrib if joints else {}
    hinge = joints[1:] if first.get("type") == "free" else (joints if "type" not in first else joints[6:])
    if len(hinge) != skeleton.num_dof:
        raise _lib.PbhcError(f"{path}: {len(hinge)} hinge joints, the skeleton has {skeleton.num_dof} dofs")
    compiler = root.find("compiler")
    scale = 1.0 if compiler is not None and compiler.attrib.get("angle", "degree") == "radian" else math.pi / 180.0
    out = np.empty((len(hinge), 2), np.float64)
    for d, j in enumerate(hinge):
        if "range" in j.attrib and j.attrib.get("limited", "true") != "false":
            lo, hi = (float(x) * scale for x in j.attrib["range"].split())
            if lo > hi:
                raise _lib.PbhcError(f"{path}: joint {j.attrib.get('name')!r} has range {lo} > {hi}")
            out[d] = lo, hi
        else:
            out[d] = -UNLIMITED, UNLIMITED
    return out


def heading_rotvec(left, right):
    """Yaw-only root rotation vectors [F, 3] (float64) from two key points [F, 3] each: the robot's +y points from `right` to `left`,
    projected to the ground plane.  +y of a yaw psi is (-sin psi, cos psi), so psi = atan2(-dx, dy) of d = left - right."""
    d = np.asarray(left, np.float64) - np.asarray(right, np.float64)
    if bool((np.hypot(d[:, 0], d[:, 1]) < 1e-9).any()):
        raise _lib.PbhcError(f"{KEY}: heading_from points coincide on the ground plane in some frame")
    out = np.zeros_like(d)
    out[:, 2] = np.arctan2(-d[:, 0], d[:, 1])
    return out


@dataclass
class RetargetSettings:
    """Validated settings; the defaults are the reference's constants (1000 iterations, Adadelta lr 100, Adam lr 0.01, sigma 0.75)."""
    enable: bool = False
    joint_matches: list = field(default_factory=list)       # [[robot body name, key-point name or index], ...]
    iterations: int = 1000
    dof_lr: float = 100.0
    root_lr: float = 0.01
    filter: bool = True
    filter_sigma: float = 0.75
    limits: object = "mjcf"                                 # "mjcf" or a [D, 2] list
    heading_from: list = None                               # [left body, right body]: two bodies of joint_matches
    ground: str = "none"
    mjcf: str = None                                        # path of the robot's MJCF (for limits: "mjcf")
    rho: float = 0.9
    adadelta_eps: float = 1e-6
    betas: tuple = (0.9, 0.999)
    adam_eps: float = 1e-8

    def __post_init__(self):
        self.enable, self.filter, self.ground = bool(self.enable), bool(self.filter), str(self.ground)
        if int(self.iterations) != self.iterations or int(self.iterations) < 1:
            raise _lib.PbhcError(f"{KEY}: iterations {self.iterations} must be an integer >= 1")
        self.iterations = int(self.iterations)
        self.dof_lr, self.root_lr, self.filter_sigma = float(self.dof_lr), float(self.root_lr), float(self.filter_sigma)
        if not (self.dof_lr >= 0.0 and math.isfinite(self.dof_lr) and self.root_lr >= 0.0 and math.isfinite(self.root_lr)):
            raise _lib.PbhcError(f"{KEY}: dof_lr {self.dof_lr} and root_lr {self.root_lr} must be >= 0")
        if not (self.filter_sigma > 0.0 and math.isfinite(self.filter_sigma)):
            raise _lib.PbhcError(f"{KEY}: filter_sigma {self.filter_sigma} must be > 0")
        if self.ground not in GROUNDS:
            raise _lib.PbhcError(f"{KEY}: ground {self.ground!r}; known: {list(GROUNDS)}")
        matches = []
        for m in self.joint_matches:
            m = list(m)
            if len(m) != 2:
                raise _lib.PbhcError(f"{KEY}: joint_matches entry {m} is not a [robot body, key point] pair")
            matches.append([str(m[0]), m[1] if isinstance(m[1], str) else int(m[1])])
        self.joint_matches = matches
        if self.enable and not matches:
            raise _lib.PbhcError(f"{KEY}: joint_matches is empty")
        if len(matches) > _lib.K["PBHC_MAX_BODIES"]:
            raise _lib.PbhcError(f"{KEY}: {len(matches)} joint_matches, at most {_lib.K['PBHC_MAX_BODIES']}")
        if self.heading_from is not None:
            self.heading_from = [str(n) for n in self.heading_from]
            bodies = [m[0] for m in matches]
            if len(self.heading_from) != 2 or self.heading_from[0] == self.heading_from[1] or any(n not in bodies for n in self.heading_from):
                raise _lib.PbhcError(f"{KEY}: heading_from {self.heading_from} must name two different bodies of joint_matches ({bodies})")
        if isinstance(self.limits, str):
            if self.limits != "mjcf":
                raise _lib.PbhcError(f"{KEY}: limits {self.limits!r}; known: 'mjcf' or a [D, 2] list")
            if self.enable and self.mjcf is None:
                raise _lib.PbhcError(f"{KEY}: limits 'mjcf' needs the robot's MJCF path (the skeleton came from a JSON file?); give limits as a [D, 2] list")
        else:
            lim = np.asarray(self.limits, np.float64)
            if lim.ndim != 2 or lim.shape[1] != 2 or bool((lim[:, 0] > lim[:, 1]).any()) or not bool(np.isfinite(lim).all()):
                raise _lib.PbhcError(f"{KEY}: limits must be a [D, 2] list of finite lo <= hi, got shape {lim.shape}")
            self.limits = lim

    @property
    def active(self):
        return self.enable

    @classmethod
    def from_config(cls, node, mjcf=None):
        """node = config.robot.motion.retarget (None / absent: returns None); mjcf: the robot's MJCF path, if there is one"""
        if node is None:
            return None
        node = dict(node)
        unknown = sorted(set(node) - set(KEYS))
        if unknown:
            raise _lib.PbhcError(f"{KEY}: unknown key(s) {unknown}; known: {list(KEYS)}")
        lim = node.get("limits", "mjcf")
        hf = node.get("heading_from", None)
        return cls(enable=node.get("enable", False), joint_matches=[list(m) for m in node.get("joint_matches", None) or []],
                   iterations=node.get("iterations", 1000), dof_lr=node.get("dof_lr", 100.0), root_lr=node.get("root_lr", 0.01),
                   filter=node.get("filter", True), filter_sigma=node.get("filter_sigma", 0.75),
                   limits=lim if isinstance(lim, str) else [list(r) for r in lim], heading_from=list(hf) if hf is not None else None,
                   ground=node.get("ground", "none"), mjcf=mjcf)

    def picks(self, skeleton):
        """the matched bodies as indices into the skeleton's extended body list; an unknown one is refused by name"""
        names = [str(n) for n in skeleton.body_names_ext]
        for body, _ in self.joint_matches:
            if body not in names:
                raise _lib.PbhcError(f"{KEY}: joint_matches body {body!r} is not a body of the skeleton ({names})")
        return [names.index(body) for body, _ in self.joint_matches]

    def keypoint_columns(self, num_keypoints, keypoint_names=None):
        """the matched key points as columns of a clip's `keypoints` array"""
        names = None if keypoint_names is None else [str(n) for n in keypoint_names]
        cols = []
        for body, kp in self.joint_matches:
            if isinstance(kp, str):
                if names is None or kp not in names:
                    raise _lib.PbhcError(f"{KEY}: key point {kp!r} (matched to {body!r}) is not among the clip's keypoint_names ({names})")
                kp = names.index(kp)
            if not 0 <= kp < num_keypoints:
                raise _lib.PbhcError(f"{KEY}: key point {kp} (matched to {body!r}) outside [0, {num_keypoints})")
            cols.append(kp)
        return cols

    def limits_array(self, skeleton):
        lim = mjcf_limits(self.mjcf, skeleton) if isinstance(self.limits, str) else self.limits
        if lim.shape != (skeleton.num_dof, 2):
            raise _lib.PbhcError(f"{KEY}: limits of shape {lim.shape}, the skeleton has {skeleton.num_dof} dofs")
        return lim

    def to_c(self, skeleton):
        p = _lib.PbhcRetargetParams()
        picks = self.picks(skeleton)
        p.num_picks = len(picks)
        for l, b in enumerate(picks):
            p.pick[l] = b
        p.dof_lr, p.root_lr, p.rho, p.adadelta_eps = self.dof_lr, self.root_lr, self.rho, self.adadelta_eps
        p.beta1, p.beta2, p.adam_eps = self.betas[0], self.betas[1], self.adam_eps
        p.filter_taps, p.filter_sigma = (5 if self.filter else 0), self.filter_sigma
        for d, (lo, hi) in enumerate(self.limits_array(skeleton)):
            p.limits[d][0], p.limits[d][1] = lo, hi
        return p


def prepare_targets(clips, skeleton, settings):
    """host side of `fit`: -> (keypoints [total, P, 3], trans [total, 3], root_rot_init [total, 3] as float32, nframes, fps)"""
    picks = settings.picks(skeleton)
    bodies = [m[0] for m in settings.joint_matches]
    kps, trans, rots, nframes, fps = [], [], [], [], []
    for i, c in enumerate(clips):
        kp = np.asarray(c["keypoints"], np.float64)
        if kp.ndim != 3 or kp.shape[2] != 3 or kp.shape[0] < 1:
            raise _lib.PbhcError(f"{KEY}: clip {i}: keypoints of shape {kp.shape}, expected [F >= 1, K, 3]")
        kp = kp[:, settings.keypoint_columns(kp.shape[1], c.get("keypoint_names", None))]
        if "root_trans_offset" in c:
            tr = np.asarray(c["root_trans_offset"], np.float64)
        elif 0 in picks:
            tr = kp[:, picks.index(0)]
        else:
            raise _lib.PbhcError(f"{KEY}: clip {i} ships no root_trans_offset and no key point is matched to the root body")
        if "root_rot_init" in c:
            rr = np.asarray(c["root_rot_init"], np.float64)
        elif settings.heading_from is not None:
            rr = heading_rotvec(kp[:, bodies.index(settings.heading_from[0])], kp[:, bodies.index(settings.heading_from[1])])
        else:
            raise _lib.PbhcError(f"{KEY}: clip {i} ships no root_rot_init and heading_from is not set")
        if tr.shape != (kp.shape[0], 3) or rr.shape != (kp.shape[0], 3):
            raise _lib.PbhcError(f"{KEY}: clip {i}: root_trans_offset {tr.shape} / root_rot_init {rr.shape}, expected ({kp.shape[0]}, 3)")
        kps.append(kp); trans.append(tr); rots.append(rr); nframes.append(kp.shape[0]); fps.append(int(c["fps"]))
    cat = lambda a: np.ascontiguousarray(np.concatenate(a, axis=0).astype(np.float32))
    return cat(kps), cat(trans), cat(rots), nframes, fps


class Fitter:
    """The device state of one fit (joints, root rotation, root offset and their optimiser state) and its launches; `run(k)` continues from
    where the last call stopped, so run(k) + run(n - k) is run(n)."""

    def __init__(self, skeleton, params, keypoints, trans, root_rot_init, nframes, device):
        import torch

        self.skeleton, self.params, self.csk = skeleton, params, skeleton.to_c()
        self.nframes = [int(n) for n in nframes]
        self.starts = np.concatenate([[0], np.cumsum(self.nframes)]).astype(np.int32)
        self.total, self.M, D = int(self.starts[-1]), len(self.nframes), skeleton.num_dof
        up = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(device)
        self.kp, self.trans = up(keypoints), up(trans)
        if tuple(self.kp.shape) != (self.total, params.num_picks, 3) or tuple(self.trans.shape) != (self.total, 3):
            raise _lib.PbhcError(f"{KEY}: keypoints {tuple(self.kp.shape)} / trans {tuple(self.trans.shape)} for {self.total} frames, {params.num_picks} picks")
        self.d_starts = torch.from_numpy(self.starts).to(device)
        z = lambda *s: torch.zeros(*s, device=device)
        self.dof, self.dof_sq, self.dof_acc = z(self.total, D), z(self.total, D), z(self.total, D)
        self.root_rot, self.root_m, self.root_v = up(root_rot_init).clone(), z(self.total, 3), z(self.total, 3)
        self.root_off, self.off_m, self.off_v = z(self.M, 3), z(self.M, 3), z(self.M, 3)
        self.scratch = torch.empty((D + 4) * self.total, device=device)
        st = self.state = _lib.PbhcRetargetState()
        for name in ("dof", "dof_sq", "dof_acc", "root_rot", "root_m", "root_v", "root_off", "off_m", "off_v", "scratch"):
            setattr(st, name, getattr(self, name).data_ptr())
        st.step = 0

    def _starts(self):
        return self.starts.ctypes.data_as(C.c_void_p)

    def run(self, iterations):
        """-> loss_history [iterations, M] on the device (the loss before each update); no synchronisation"""
        import torch

        hist = torch.empty(int(iterations), self.M, device=self.kp.device)
        _lib.check(_lib.lib().pbhc_retarget_fit(C.byref(self.csk), C.byref(self.params), _lib.ptr(self.kp), _lib.ptr(self.trans), self.total, self.M,
                                                self._starts(), _lib.ptr(self.d_starts), C.byref(self.state), int(iterations), _lib.ptr(hist),
                                                _lib.current_stream()), "pbhc_retarget_fit")
        return hist

    def loss_grad(self, body_pos=False):
        """loss and analytic gradients at the current state, no update -> (loss [M], g_dof, g_root_rot, g_root_off, body_pos or None)"""
        import torch

        dev, Bx = self.kp.device, self.skeleton.num_bodies_ext
        loss, g_dof, g_rr, g_off = torch.empty(self.M, device=dev), torch.empty_like(self.dof), torch.empty_like(self.root_rot), torch.empty_like(self.root_off)
        pos = torch.empty(self.total, Bx, 3, device=dev) if body_pos else None
        _lib.check(_lib.lib().pbhc_retarget_loss_grad(C.byref(self.csk), C.byref(self.params), _lib.ptr(self.kp), _lib.ptr(self.trans), _lib.ptr(self.dof),
                                                      _lib.ptr(self.root_rot), _lib.ptr(self.root_off), self.total, self.M, self._starts(),
                                                      _lib.ptr(self.d_starts), _lib.ptr(loss), _lib.ptr(g_dof), _lib.ptr(g_rr), _lib.ptr(g_off), _lib.ptr(pos),
                                                      _lib.ptr(self.scratch), _lib.current_stream()), "pbhc_retarget_loss_grad")
        return loss, g_dof, g_rr, g_off, pos

    def finish(self):
        """the final clamp of the joints (in place) -> (pose_aa [total, Bx, 3], root_trans_offset [total, 3], root quaternion xyzw [total, 4])"""
        import torch

        dev, Bx = self.kp.device, self.skeleton.num_bodies_ext
        pose, tr, quat = torch.empty(self.total, Bx, 3, device=dev), torch.empty(self.total, 3, device=dev), torch.empty(self.total, 4, device=dev)
        _lib.check(_lib.lib().pbhc_retarget_finish(C.byref(self.csk), C.byref(self.params), _lib.ptr(self.trans), self.total, self.M, self._starts(),
                                                   _lib.ptr(self.d_starts), C.byref(self.state), _lib.ptr(pose), _lib.ptr(tr), _lib.ptr(quat),
                                                   _lib.current_stream()), "pbhc_retarget_finish")
        return pose, tr, quat


def fit(batch_of_targets, skeleton, settings, device="cuda:0"):
    """Fit every key-point clip of the list in one batch.  -> (ClipBatch of the fitted clips (pose, trans; no contact mask), dof [total, D],
    root_rot [total, 4] xyzw, loss_history [iterations, M]), all on the device; the stream is synchronised once, at the end."""
    import torch

    from .motion_ingest import ClipBatch

    kp, trans, rot, nframes, fps = prepare_targets(batch_of_targets, skeleton, settings)
    fitter = Fitter(skeleton, settings.to_c(skeleton), kp, trans, rot, nframes, device)
    hist = fitter.run(settings.iterations)
    pose, tr, quat = fitter.finish()
    if settings.ground == "first_frame_min_body":      # the lowest body origin of each clip's first frame comes to height 0
        pos = fitter.loss_grad(body_pos=True)[4]        # (only the body positions of this call are used)
        low = pos[fitter.d_starts[:-1].long(), :, 2].min(dim=1).values
        tr[:, 2] -= torch.repeat_interleave(low, torch.tensor(nframes, device=tr.device))
    torch.cuda.current_stream().synchronize()           # the fitter's buffers die with this scope
    return ClipBatch(pose, tr, None, nframes, fps), fitter.dof, quat, hist
