"""Generator states as what a checkpoint may hold.

A checkpoint is read with `torch.load(weights_only=True)` (agents/base.py `_load_checkpoint`): tensors, numbers, strings, lists, tuples,
dicts and None.  `torch.Generator.get_state()` is a uint8 tensor already; `random.Random.getstate()` is a tuple of a version, a tuple of 625
ints and None or a float; `numpy.random.get_state()` is a tuple that holds a uint32 array.  pack_* turn them into such containers,
unpack_* back; a packed state is a copy, on the CPU, whatever device the checkpoint was mapped to in between.
"""
from __future__ import annotations

import random

import numpy as np
import torch


def pack_torch(state):
    """`torch.get_rng_state()` / `torch.cuda.get_rng_state(dev)` / `generator.get_state()` -> a uint8 CPU tensor of its own"""
    return state.detach().to("cpu", torch.uint8).clone()


def unpack_torch(packed):
    """-> what `set_rng_state` / `set_state` take (a ByteTensor on the CPU)"""
    return packed.detach().to("cpu", torch.uint8).contiguous()


def pack_python(state):
    """`random.getstate()` / `random.Random.getstate()` -> [version, int64 tensor of the 625 words, gauss_next]"""
    version, words, gauss_next = state
    return [int(version), torch.tensor(list(words), dtype=torch.int64), None if gauss_next is None else float(gauss_next)]


def unpack_python(packed):
    version, words, gauss_next = packed
    return (int(version), tuple(int(w) for w in words.cpu().tolist()), None if gauss_next is None else float(gauss_next))


def pack_numpy(state):
    """`numpy.random.get_state()` (the legacy MT19937 tuple) -> [name, int64 tensor of the key, pos, has_gauss, cached_gaussian]"""
    name, key, pos, has_gauss, cached = state
    return [str(name), torch.from_numpy(np.asarray(key, dtype=np.int64).copy()), int(pos), int(has_gauss), float(cached)]


def unpack_numpy(packed):
    name, key, pos, has_gauss, cached = packed
    return (str(name), key.cpu().numpy().astype(np.uint32), int(pos), int(has_gauss), float(cached))


def capture_globals(device):
    """the four process-wide generators training draws from: torch's CPU generator, the device generator of `device` (the minibatch
    permutation, `init_at_random_ep_len`), Python's `random` module (the crop draws), numpy's global state (ReinitSchedule)"""
    return {"torch_cpu": pack_torch(torch.get_rng_state()), "torch_device": pack_torch(torch.cuda.get_rng_state(device)),
            "python": pack_python(random.getstate()), "numpy": pack_numpy(np.random.get_state())}


def restore_globals(packed, device):
    torch.set_rng_state(unpack_torch(packed["torch_cpu"]))
    torch.cuda.set_rng_state(unpack_torch(packed["torch_device"]), device)
    random.setstate(unpack_python(packed["python"]))
    np.random.set_state(unpack_numpy(packed["numpy"]))
