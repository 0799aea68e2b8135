"""The C-ABI library loads and exports every symbol include/pbhc_hip.h declares, and the binding pbhc_amd/_lib.py derives from the header
(prototypes, struct layouts) is what a C++ compiler reads in it (no compute, no GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from pbhc_amd import _lib


def test_header_symbols_are_exported():
    text = _lib._strip_comments(open(_lib.HEADER).read())
    declared = set(re.findall(r"\b(pbhc_\w+)\s*\(", text))
    assert declared, "no declarations parsed"
    lib = _lib.lib()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in pbhc_hip.h but not exported"
    assert declared == set(_lib.EXPORTS)


def test_struct_sizes_agree():
    lib = _lib.lib()
    assert lib.pbhc_sizeof_env_config() == C.sizeof(_lib.PbhcEnvConfig)
    assert lib.pbhc_sizeof_step_io() == C.sizeof(_lib.PbhcStepIO)
    assert lib.pbhc_abi_version() == _lib.K["PBHC_ABI_VERSION"]


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib.lib()
    assert lib.pbhc_env_step(None, None, None) == _lib.K["PBHC_EINVAL"]
    sk = _lib.PbhcSkeleton()
    sk.num_bodies = 100
    assert lib.pbhc_sim_fk(C.byref(sk), None, None, None, 1, 0, None, None) == _lib.K["PBHC_EINVAL"]
    assert b"bad argument" in lib.pbhc_last_error()


def test_product_does_not_import_the_oracle():
    root = os.path.join(_lib.ROOT, "pbhc_amd")
    for dp, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), f"{f} imports the oracle"


# ---- the derived binding against a compiler's reading of the header ----------------------------------------------------------------

_CXX_PRELUDE = r"""
#include "pbhc_hip.h"
#include <cstddef>
#include <cstdio>
#include <string>
#include <type_traits>
template <class T> std::string cls() {
  if constexpr (std::is_void_v<T>) return "void";
  else if constexpr (std::is_pointer_v<T>) return "ptr";
  else if constexpr (std::is_class_v<T>) return "struct" + std::to_string(sizeof(T));
  else if constexpr (std::is_floating_point_v<T>) return "float" + std::to_string(sizeof(T));
  else if constexpr (std::is_integral_v<T>) return (std::is_signed_v<T> ? "signed" : "unsigned") + std::to_string(sizeof(T));
  else return "other";
}
template <class R, class... A> std::string sig(R (*)(A...)) { std::string s = cls<R>() + "("; ((s += cls<A>() + ","), ...); return s + ")"; }
static int checked = 0, mismatches = 0;
static void expect(const char* what, const std::string& compiler, const std::string& binding) {
  ++checked;
  if (compiler != binding) { ++mismatches; std::printf("MISMATCH %s: compiler %s, binding %s\n", what, compiler.c_str(), binding.c_str()); }
}
"""


def _compile_and_run(tmp_path, body, groups):
    """C++17 program: prelude + main(){body}; prints `groups checked mismatches`.  Returns its output after asserting it ran."""
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", rocm_clang) if shutil.which(c)), None)
    assert cxx, "no C++ compiler found ($CXX, c++, g++, ROCm's clang++): the build needs one"
    src = tmp_path / "abi_check.cpp"
    src.write_text(_CXX_PRELUDE + "int main() {\n" + body + f'  std::printf("%d %d %d\\n", {groups}, checked, mismatches);\n  return 0;\n}}\n')
    exe = tmp_path / "abi_check"
    cc = subprocess.run([cxx, "-std=c++17", "-I", os.path.dirname(_lib.HEADER), "-o", str(exe), str(src)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout


def _class_of(ct):
    """the compiler-side class string (cls<T>() above) of a ctypes type"""
    if ct is None:
        return "void"
    if issubclass(ct, C.Structure):
        return f"struct{C.sizeof(ct)}"
    if issubclass(ct, (C._Pointer, C.c_void_p, C.c_char_p)):
        return "ptr"
    code = ct._type_
    kind = "float" if code in "fdg" else "signed" if code in "bhilq" else "unsigned" if code in "BHILQ" else "other"
    return f"{kind}{C.sizeof(ct)}"


def test_prototypes_match_the_compiler(tmp_path):
    lib = _lib.lib()
    body = ""
    for name in _lib.EXPORTS:
        fn = getattr(lib, name)
        assert fn.argtypes is not None, f"{name}: argtypes unset"
        binding = _class_of(fn.restype) + "(" + "".join(_class_of(a) + "," for a in fn.argtypes) + ")"
        body += f'  expect("{name}", sig(decltype(&{name}){{}}), "{binding}");\n'
    out = _compile_and_run(tmp_path, body, len(_lib.EXPORTS))
    print(out)
    assert out.splitlines()[-1] == f"{len(_lib.EXPORTS)} {len(_lib.EXPORTS)} 0", out


def test_struct_layouts_match_the_compiler(tmp_path):
    body, n = "", 0
    for name, cls in _lib._S.items():
        body += f'  expect("sizeof({name})", std::to_string(sizeof({name})), "{C.sizeof(cls)}");\n'
        n += 1
        for fname, ftype in cls._fields_:
            body += f'  expect("offsetof({name}, {fname})", std::to_string(offsetof({name}, {fname})), "{getattr(cls, fname).offset}");\n'
            body += f'  expect("sizeof({name}::{fname})", std::to_string(sizeof({name}::{fname})), "{C.sizeof(ftype)}");\n'
            n += 2
    out = _compile_and_run(tmp_path, body, len(_lib._S))
    print(out)
    assert len(_lib._S) == len(re.findall(r"typedef\s+struct\s+\w+\s*\{", _lib._strip_comments(open(_lib.HEADER).read())))
    assert out.splitlines()[-1] == f"{len(_lib._S)} {n} 0", out


_SYNTHETIC = """
#define PBHC_MAX_THINGS 4
typedef struct PbhcThing { int32_t n; float w[PBHC_MAX_THINGS]; const float* data; } PbhcThing;
typedef struct PbhcHandle PbhcHandle;
int pbhc_sizeof_thing(void);
size_t pbhc_thing_bytes(const PbhcThing* t, PbhcThing by_value, PbhcHandle** out, const float* const* rows, long long stride,
                        const char* name, char* buf, void* stream);
void pbhc_thing_reset(PbhcHandle* h);
"""


def test_parser_reads_a_synthetic_header():
    consts, structs, protos, sizeofs = _lib._parse_header(_SYNTHETIC)
    thing = structs["PbhcThing"]
    assert consts["PBHC_MAX_THINGS"] == 4 and sizeofs == {"pbhc_sizeof_thing": thing}
    assert protos["pbhc_sizeof_thing"] == (C.c_int, [])
    assert protos["pbhc_thing_reset"] == (None, [C.c_void_p])
    restype, args = protos["pbhc_thing_bytes"]
    assert restype is C.c_size_t
    assert args == [C.POINTER(thing), thing, C.c_void_p, C.c_void_p, C.c_longlong, C.c_char_p, C.c_void_p, C.c_void_p]


@pytest.mark.parametrize("name, decl", [
    ("pbhc_unknown_type", "int pbhc_unknown_type(const PbhcMystery* m, int n);"),
    ("pbhc_unknown_scalar", "int pbhc_unknown_scalar(unsigned int n);"),
    ("pbhc_unknown_return", "short pbhc_unknown_return(int n);"),
    ("pbhc_callback", "int pbhc_callback(void (*fn)(int), int n);"),
    ("pbhc_variadic", "int pbhc_variadic(const char* fmt, ...);"),
    ("pbhc_struct_pp", "int pbhc_struct_pp(PbhcThing** out);"),
    ("pbhc_not_a_declaration", "#define PBHC_CALL(x) pbhc_not_a_declaration(x)"),
    ("pbhc_sizeof_nothing", "int pbhc_sizeof_nothing(void);"),
])
def test_parser_refuses_what_it_does_not_understand(name, decl):
    with pytest.raises(ValueError, match=name):
        _lib._parse_header(_SYNTHETIC + decl + "\n")


def test_argument_conversions():
    """what each derived argtype accepts and refuses, by its from_param: no call is made"""
    lib = _lib.lib()
    assert lib.pbhc_abi_version.argtypes == []
    jobs = lib.pbhc_colsum_final.argtypes[0]              # const PbhcColsumJob* jobs
    assert jobs is C.POINTER(_lib.PbhcColsumJob)
    with pytest.raises((TypeError, C.ArgumentError)):
        jobs.from_param(C.byref(_lib.PbhcSkeleton()))
    jobs.from_param((_lib.PbhcColsumJob * 3)())
    jobs.from_param(None)
    pose = lib.pbhc_motion_build.argtypes[1]              # const float* pose_aa
    pose.from_param(0x7F0000001000)
    blocks = lib.pbhc_act_bwd_partials.argtypes[7]        # int* num_row_blocks
    weights = lib.pbhc_mlp_fwd.argtypes[2]                # const float* const* weights
    assert pose is C.c_void_p and blocks is C.c_void_p and weights is C.c_void_p
    for arg in (blocks, weights):
        for value in (C.byref(C.c_int()), (C.c_int * 3)(), (C.c_void_p * 2)(), None):
            arg.from_param(value)
