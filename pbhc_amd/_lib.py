"""ctypes binding of libpbhc_hip.so (include/pbhc_hip.h).

Everything the binding knows about the ABI comes from one parse of the header text: the constants, the ctypes Structures, the
prototype (restype, argtypes) of every declared function, the list of exports and the `pbhc_sizeof_*()` / struct pairs that are
compared at load.  A declaration the parser does not understand raises at import; nothing is skipped.  tests/test_abi.py holds the
derived prototypes and struct layouts against a C++ compiler's view of the same header.
There is no fallback: if the library is missing or was built for another ABI, using the product raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
HEADER = os.path.join(ROOT, "include", "pbhc_hip.h")
LIB_PATH = os.environ.get("PBHC_LIB", os.path.join(_HERE, "libpbhc_hip.so"))   # PBHC_LIB: diagnostic builds only

_CTYPES = {
    "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
    "float": C.c_float, "double": C.c_double, "uint8_t": C.c_uint8, "int": C.c_int,
    "size_t": C.c_size_t, "long long": C.c_longlong,
}


def _strip_comments(t):
    t = re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    return re.sub(r"//[^\n]*", "", t)


def _ctype(decl, structs, opaque, fn):
    """The mapping rule: one return type or parameter of the declaration of `fn` -> its ctypes type (None for void).
    Scalars and structs by value map to themselves, `const char*` to c_char_p, one level of pointer to a struct with a body to
    POINTER(that class) (so the wrong struct raises on the host), every other pointer to a known type to c_void_p (callers pass
    tensor.data_ptr() integers, byref, arrays or None).  Anything else raises."""
    m = re.fullmatch(r"(const\s+)?(long long|\w+)((?:\s*\*(?:\s*const\b)?)*)\s*(\w+)?", " ".join(decl.split()))
    if m:
        const, base, stars = m.group(1), m.group(2), m.group(3).count("*")
        if stars == 0:
            if base == "void" and not m.group(4):
                return None
            if base in _CTYPES:
                return _CTYPES[base]
            if base in structs:
                return structs[base]
        elif base in structs:
            if stars == 1:
                return C.POINTER(structs[base])
        elif base == "char" and const and stars == 1:
            return C.c_char_p
        elif base in _CTYPES or base in opaque or base in ("void", "char"):
            return C.c_void_p
    raise ValueError(f"{fn}: no ctypes mapping for '{decl.strip()}' in include/pbhc_hip.h")


def _parse_header(text):
    """header text -> (constants, Structures by name, {function: (restype, [argtypes])}, {pbhc_sizeof_* function: its Structure})"""
    text = _strip_comments(text)
    consts = {}
    for m in re.finditer(r"#define\s+(PBHC_\w+)\s+\(?(-?\d+)\)?", text):
        consts[m.group(1)] = int(m.group(2))
    for m in re.finditer(r"enum\s+(\w+)\s*\{(.*?)\}", text, flags=re.S):
        val = -1
        for item in m.group(2).split(","):
            item = item.strip()
            if not item:
                continue
            if "=" in item:
                name, v = [x.strip() for x in item.split("=")]
                val = int(eval(v, {}, consts))
            else:
                name, val = item, val + 1
            consts[name] = val
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S):
        name, body = m.group(1), m.group(2)
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            mm = re.match(r"^(const\s+)?(\w+)\s*(\*?)\s*(.*)$", decl)
            base, first_ptr, rest = mm.group(2), mm.group(3), mm.group(4)
            variables = [v.strip() for v in rest.split(",")]
            variables[0] = first_ptr + variables[0]
            for var in variables:
                is_ptr = var.startswith("*")
                var = var.lstrip("* ")
                dims = [int(eval(d, {}, consts)) for d in re.findall(r"\[([^\]]+)\]", var)]
                vname = re.match(r"^(\w+)", var).group(1)
                if is_ptr:
                    ct = C.c_void_p
                elif base in _CTYPES:
                    ct = _CTYPES[base]
                elif base in structs:
                    ct = structs[base]
                else:
                    raise ValueError(f"unknown type {base} in {name}")
                for d in reversed(dims):
                    ct = ct * d
                fields.append((vname, ct))
        structs[name] = type(name, (C.Structure,), {"_fields_": fields})
    opaque = set(re.findall(r"typedef\s+struct\s+(\w+)\s+\1\s*;", text))
    protos = {}
    for m in re.finditer(r"^[ \t]*([\w \t*]+?)\s*\b(pbhc_\w+)\s*\(([^;{}]*)\)\s*;", text, flags=re.M):
        ret, fn, params = m.groups()
        args = [] if params.strip() in ("", "void") else [_ctype(p, structs, opaque, fn) for p in params.split(",")]
        if None in args:
            raise ValueError(f"{fn}: a parameter of type void in include/pbhc_hip.h")
        protos[fn] = (_ctype(ret, structs, opaque, fn), args)
    missing = set(re.findall(r"\b(pbhc_\w+)\s*\(", text)) - set(protos)
    if missing:
        raise ValueError(f"include/pbhc_hip.h names functions whose declarations were not parsed: {sorted(missing)}")
    squash = {s.replace("_", "").lower(): cls for s, cls in structs.items()}
    sizeofs = {}
    for fn in protos:
        if fn.startswith("pbhc_sizeof_"):
            key = "pbhc" + fn[len("pbhc_sizeof_"):].replace("_", "")
            if key not in squash:
                raise ValueError(f"{fn}: include/pbhc_hip.h defines no struct of that name")
            sizeofs[fn] = squash[key]
    return consts, structs, protos, sizeofs


K, _S, _PROTOS, _SIZEOFS = _parse_header(open(HEADER).read())
globals().update(_S)   # every struct of the header by its name: PbhcSkeleton, PbhcEnvConfig, PbhcStepIO, ...
EXPORTS = list(_PROTOS)


class PbhcError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise PbhcError(
            f"{LIB_PATH} not found: the HIP extension is required (there is no CPU fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C pbhc_amd/csrc`."
        )
    lib = C.CDLL(LIB_PATH)
    if lib.pbhc_abi_version() != K["PBHC_ABI_VERSION"]:
        raise PbhcError("libpbhc_hip.so ABI version does not match include/pbhc_hip.h")
    for name, (restype, argtypes) in _PROTOS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    for name, struct in _SIZEOFS.items():
        if getattr(lib, name)() != C.sizeof(struct):
            raise PbhcError(f"struct layout mismatch between libpbhc_hip.so and include/pbhc_hip.h ({struct.__name__}) — rebuild")
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def check(rc, what=""):
    if rc != 0:
        raise PbhcError(f"{what} failed ({rc}): {lib().pbhc_last_error().decode()}")


def ptr(t):
    """raw device pointer of a torch tensor; None -> NULL"""
    return None if t is None else t.data_ptr()


def current_stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def padded_width(dim):
    """Row pitch (floats) of the [N, dim] tensors the env kernel writes: a multiple of 32 floats (rows start on 128-byte lines) with at
    least two floats of padding (lanes past the end of a row store there instead of being predicated off)."""
    return (dim + 2 + 31) // 32 * 32


def require_gpu_rows(t, name, dtype=None, shape=None):
    """as require_gpu_tensor, but rows may be padded: [N, C] with stride (pitch >= C, 1)"""
    import torch

    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
        raise PbhcError(f"{name}: expected a CUDA(HIP) [N, C] tensor with unit inner stride")
    if dtype is not None and t.dtype != dtype:
        raise PbhcError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise PbhcError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def require_gpu_tensor(t, name, dtype=None, shape=None):
    """host-side shape/dtype/device check before a raw pointer crosses the ABI"""
    import torch

    if not (torch.is_tensor(t) and t.is_cuda and t.is_contiguous()):
        raise PbhcError(f"{name}: expected a contiguous CUDA(HIP) tensor")
    if dtype is not None and t.dtype != dtype:
        raise PbhcError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise PbhcError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t
