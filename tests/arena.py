"""Operands with poisoned surroundings, for the tests that pin what a kernel does to memory AROUND its operands (tests/test_gpu_mlp_edges.py,
tests/test_gpu_gemm_memory.py), and the float64 restatement of the one-launch ConvEncoder those tests compare against.

`arena(rows, cols, ...)` puts a [rows, cols] operand into a 1-D buffer at a chosen float offset and row pitch, with MARGIN floats before
and behind it.  An INPUT arena is NaN wherever the kernel's contract says it must not depend on — margins and inter-row padding — so a
read that leaks into a result makes the result non-finite; an OUTPUT arena is SENT everywhere, an exactly representable value no kernel
produces, so a store outside the operand's logical elements — the columns between N and the pitch included — is found by `intact`.
The margins also bound what a wrong kernel can reach: a few floats past an operand are still inside the buffer."""
import torch

MARGIN = 256                       # floats before and behind every operand (1 KiB: the buffer's base stays 16-byte aligned + offset)
SENT = -777.25                     # as tests/test_gpu_ppo_kernels.py: exactly representable, never produced


class Arena:
    """buf: the 1-D buffer; view: the [rows, cols] operand inside it (row pitch `pitch`, first element at float MARGIN + offset)"""

    def __init__(self, buf, view, fill):
        self.buf, self.view, self.fill = buf, view, fill

    def ptr(self):
        return self.view.data_ptr()

    def outside(self):
        """the buffer's elements that are not logical elements of the operand"""
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        rows, cols = self.view.shape
        start = self.view.storage_offset()
        idx = start + torch.arange(rows, device=self.buf.device)[:, None] * self.view.stride(0) + torch.arange(cols, device=self.buf.device)[None, :]
        mask[idx.reshape(-1)] = False
        return self.buf[mask]

    def intact(self):
        """everything outside the operand still holds the fill value (NaN compares by isnan)"""
        out = self.outside()
        return bool(torch.isnan(out).all()) if self.fill != self.fill else bool((out == self.fill).all())

    def untouched(self):
        """the WHOLE buffer still holds the fill value (a refused call)"""
        return bool(torch.isnan(self.buf).all()) if self.fill != self.fill else bool((self.buf == self.fill).all())


def arena(rows, cols, pitch=None, offset=0, fill=float("nan"), data=None, device="cpu", dtype=torch.float32):
    """[rows, cols] operand at float offset `offset` behind a 16-byte boundary, rows `pitch` (default cols) floats apart, everything else
    `fill`; `data` ([rows, cols] or broadcastable) is copied into the operand, which otherwise holds `fill` too."""
    pitch = cols if pitch is None else pitch
    assert pitch >= cols and rows >= 1 and cols >= 1 and offset >= 0
    buf = torch.full((2 * MARGIN + offset + rows * pitch,), fill, dtype=dtype, device=device)
    view = buf.as_strided((rows, cols), (pitch, 1), MARGIN + offset)
    if data is not None:
        view.copy_(data)
    return Arena(buf, view, fill)


def act64(act, z):
    import torch.nn.functional as F

    return {0: z, 1: F.elu(z), 2: F.silu(z), 3: F.relu(z)}[act]


def conv_encoder_ref(x, w1, b1, wc1, bc1, wc2, bc2, wo, bo, T, d, k1, s1, k2, s2, act):
    """pbhc_conv_encoder_fwd on the raw matrices of its ABI, in the dtype of its arguments (float64 for the reference): x [M, T * d];
    w1 [H, d] Linear + ReLU per time step; wc1 [O1, k1 * H], wc2 [O2, k2 * O1] windowed Linear + act with the kernel tap OUTER (a window of
    the time-major activations is k * C contiguous floats); wo [E, L2 * O2] on the (position, channel) columns."""
    M = x.shape[0]
    h = torch.relu(x.reshape(M, T, d) @ w1.t() + b1)                                     # [M, T, H]
    for w, b, k, s in ((wc1, bc1, k1, s1), (wc2, bc2, k2, s2)):
        L = (h.shape[1] - k) // s + 1
        h = torch.stack([act64(act, h[:, l * s:l * s + k, :].reshape(M, -1) @ w.t() + b) for l in range(L)], dim=1)      # [M, L, O]
    return h.reshape(M, -1) @ wo.t() + bo
