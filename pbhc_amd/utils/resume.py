"""What exact resume (DESIGN.md §8 "Exact resume") shares between the env, the simulator stub, the motion library and the agents: the version
of the training state, the fingerprint of an env's resolved config, and the checks a `load_state_dict` makes BEFORE it writes anything.
"""
from __future__ import annotations

import ctypes as C
import hashlib

import torch

from .. import _lib

STATE_VERSION = 1            # of the "training_state" entry of a checkpoint and of every state_dict() inside it
RESUME_POINTS = ("in_loop", "after_loop")


def _text(v, ct):
    """canonical text of a ctypes value of type `ct` (the form tools/gen_env_config_snapshot.py digests): floats as their exact hex, a
    pointer only as null / nonnull — no address ever enters it"""
    if issubclass(ct, C.Structure):
        return "{" + ";".join(f"{name}={_text(getattr(v, name), ft)}" for name, ft in ct._fields_) + "}"
    if issubclass(ct, C.Array):
        return "[" + ",".join(_text(v[i], ct._type_) for i in range(ct._length_)) + "]"
    if ct is C.c_void_p or ct is C.c_char_p or issubclass(ct, C._Pointer):
        return "null" if not v else "nonnull"
    return float(v).hex() if isinstance(v, float) else str(int(v))


def _short(text, limit=48):
    return text if len(text) <= limit else "sha256:" + hashlib.sha256(text.encode()).hexdigest()[:16]


def config_fingerprint(c, num_clips=None, clip_frames=None):
    """{member of PbhcEnvConfig: its canonical text, or a digest of it when it is long} of a resolved config `c` (+ the motion table's clip
    count and frame counts): two envs whose fingerprints agree run the same step on the same Philox key"""
    fp = {name: _short(_text(getattr(c, name), ft)) for name, ft in type(c)._fields_}
    if num_clips is not None:
        fp["motion.num_clips"] = str(int(num_clips))
    if clip_frames is not None:
        fp["motion.clip_frames"] = _short(",".join(str(int(f)) for f in clip_frames))
    return fp


def check_version(sd, what):
    v = sd.get("version", None) if hasattr(sd, "get") else None
    if v != STATE_VERSION:
        raise _lib.PbhcError(f"{what}: version {v!r} of the saved state, this build reads version {STATE_VERSION}")


def check_equal(what, name, saved, here):
    if saved != here:
        raise _lib.PbhcError(f"{what}: {name} differs: the saved state has {saved!r}, this run has {here!r}")


def check_fingerprint(what, saved, here):
    for k in sorted(set(saved) | set(here)):
        if saved.get(k) != here.get(k):
            raise _lib.PbhcError(f"{what}: the env config differs in {k}: the saved state has {saved.get(k)!r}, this run has {here.get(k)!r}")


def check_tensors(what, saved, targets):
    """every target tensor has a saved counterpart of its shape and dtype (`targets`: {name: tensor or None}; None on both sides is fine)"""
    for name, t in targets.items():
        s = saved.get(name, None)
        if (t is None) != (s is None):
            raise _lib.PbhcError(f"{what}: {name} differs: the saved state has {'none' if s is None else 'a tensor'}, this run has "
                                 f"{'none' if t is None else 'a tensor'} (another config?)")
        if t is not None and (not isinstance(s, torch.Tensor) or tuple(s.shape) != tuple(t.shape) or s.dtype != t.dtype):
            got = (tuple(s.shape), s.dtype) if isinstance(s, torch.Tensor) else type(s).__name__
            raise _lib.PbhcError(f"{what}: {name} differs: the saved state has {got}, this run has {(tuple(t.shape), t.dtype)}")


def snapshot(targets):
    """{name: a copy of the tensor, or None} — contiguous, on the tensor's own device"""
    return {name: None if t is None else t.detach().clone(memory_format=torch.contiguous_format) for name, t in targets.items()}


def restore(saved, targets):
    """in place (`copy_`): the step's io struct, the riders and the captured graphs hold these addresses"""
    for name, t in targets.items():
        if t is not None:
            t.copy_(saved[name].to(t.device))


def leaves(tree, prefix=""):
    """(path, leaf) of every leaf of a nested dict / list / tuple, in a fixed order: what the resume tests compare and digest"""
    if isinstance(tree, dict):
        for k in sorted(tree, key=str):
            yield from leaves(tree[k], f"{prefix}{k}.")
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            yield from leaves(v, f"{prefix}{i}.")
    else:
        yield prefix[:-1], tree
