"""Where the fused fp32-MFMA GEMM's time goes: the K loop with parts switched off (diagnosis only; results are wrong with parts off).

python tools/gemm_ablation.py [VARIANT] [--brief]
VARIANT: pbhc_gemm_debug_force_shape's staging variant (0 the shipped kernel, 1 register staging, 2 BK 16 x 3 stages).
--brief: the rows "full", "no LDS-DMA in the loop" and "no epilogue" on the update's four tile / shape classes only (A/B runs of
the K loop: one process per build, `PBHC_LIB` naming the build)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pbhc_amd import _lib   # noqa: E402

lib = _lib.lib()
M = 24576
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
VARIANT = int(ARGS[0]) if ARGS else 0
BRIEF = "--brief" in sys.argv


def timeit(fn, n=40, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


BRIEF_CASES = [(0, "full"), (1, "no LDS-DMA in the loop"), (16, "no epilogue")]
FULL_CASES = BRIEF_CASES + [(17, "no DMA, no epilogue"), (2, "epilogue without global stores"), (4, "C as streaming (nt) stores")]


def rows(tag, shape, cases, call, out, flop):
    for dbg, name in cases:
        lib.pbhc_gemm_debug_force_shape(shape | (dbg << 8) | (VARIANT << 16))
        t = timeit(call)
        lib.pbhc_gemm_debug_force_shape(shape | ((dbg | 8) << 8) | (VARIANT << 16))      # 8: one tile's cycle and wall-clock counts into out[0:2]
        call()
        torch.cuda.synchronize()
        cw = out.view(-1)[:6].tolist()
        print(f"{tag} shape {shape} {name:32s} {t:7.1f} us  {flop / t / 1e6:6.1f} TF/s-equivalent   one tile: {cw[1] / 100:.1f} us at {cw[0] / max(cw[1], 1) * 100:.0f} MHz",
              flush=True)


st = _lib.current_stream()
for N, K, shapes in [(512, 768, (2, 1)), (768, 630, (2, 1)), (128, 512, (4,) if BRIEF else (2, 1, 4))]:
    x = torch.randn(M, K, device="cuda")
    w = torch.randn(N, K, device="cuda")
    b = torch.randn(N, device="cuda")
    y = torch.empty(M, N, device="cuda")
    for shape in shapes[:1] if BRIEF else shapes:
        cases = list(BRIEF_CASES if BRIEF else FULL_CASES)
        if shape == 2 and not BRIEF:
            cases += [(d << 5, f"co-resident workgroups de-phased by {4 * d} us") for d in (2, 4, 5, 7)]
        rows(f"{N}x{K}", shape, cases, lambda: lib.pbhc_linear_act_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), None, M, N, K, 1, st), y, 2.0 * M * N * K)

# the input gradient of the 512 -> 768 layer: dx[M, 512] = dy[M, 768] . W[768, 512], times the lower layer's ELU derivative
N, K = 512, 768
dy = torch.randn(M, K, device="cuda")
w = torch.randn(K, N, device="cuda")
saved = torch.randn(M, N, device="cuda")
dx = torch.empty(M, N, device="cuda")
rows(f"dgrad {N}<-{K}", 2, BRIEF_CASES if BRIEF else FULL_CASES,
     lambda: lib.pbhc_linear_dgrad_act(dy.data_ptr(), w.data_ptr(), saved.data_ptr(), dx.data_ptr(), None, None, M, N, K, 1, st), dx, 2.0 * M * N * K)
lib.pbhc_gemm_debug_force_shape(-1)
