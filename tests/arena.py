"""Operands with poisoned surroundings, for the tests that pin what a kernel does to memory AROUND its operands (tests/test_gpu_mlp_edges.py,
tests/test_gpu_gemm_memory.py, tests/test_gpu_step_memory.py), and the float64 restatement of the one-launch ConvEncoder those tests compare
against.

`arena(rows, cols, ...)` puts a [rows, cols] operand into a 1-D buffer at a chosen element offset and row pitch, with MARGIN elements before
and behind it.  An INPUT arena is NaN wherever the kernel's contract says it must not depend on — margins and inter-row padding — so a
read that leaks into a result makes the result non-finite; an OUTPUT arena is SENT everywhere, an exactly representable value no kernel
produces, so a store outside the operand's logical elements — the columns between N and the pitch included — is found by `intact`.
The margins also bound what a wrong kernel can reach: a few floats past an operand are still inside the buffer.

`fill=POISON` serves a buffer that is read AND written (the env step's state): the surroundings hold a NaN with a fixed payload
(POISON_BITS) and are compared BIT FOR BIT through an integer view — a leaked read still makes a result non-finite, and any store, a NaN of
another payload included, changes the bits.  Integer operands (i64, i32, u8) take an integer `fill`; it is the caller's to choose one that is
harmless as data (a valid index, an in-range count): a leaked read then shows as a wrong value and can never become an address."""
import torch

MARGIN = 256                       # elements before and behind every operand (f32: 1 KiB, the buffer's base stays 16-byte aligned + offset)
SENT = -777.25                     # as tests/test_gpu_ppo_kernels.py: exactly representable, never produced
POISON = "poison"                  # fill=POISON: the NaN of POISON_BITS (floating dtypes only)
POISON_BITS = {torch.float32: 0x7FC0A5A5, torch.float64: 0x7FF8A5A5A5A5A5A5}
_INT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bool: torch.uint8}


def bits(t):
    """`t` through an integer view of the same element size (integer tensors: themselves)"""
    return t.view(_INT_VIEW[t.dtype]) if t.dtype in _INT_VIEW else t


class Arena:
    """buf: the 1-D buffer; view: the [rows, cols] operand inside it (row pitch `pitch`, first element at MARGIN + offset); name: what a
    failure report calls it"""

    def __init__(self, buf, view, fill, name="operand"):
        self.buf, self.view, self.fill, self.name = buf, view, fill, name
        self.by_nan = isinstance(fill, float) and fill != fill          # fill=nan: any NaN counts as untouched, as it always did
        self.fill_bits = bits(buf)[:1].clone()                            # (taken before any data goes in: element 0 is margin)

    def ptr(self):
        return self.view.data_ptr()

    def _logical(self, cols=None):
        """mask over the buffer: True on the operand's logical elements (`cols`: a width other than the operand's own)"""
        rows = self.view.shape[0]
        cols = self.view.shape[1] if cols is None else cols
        dev = self.buf.device
        mask = torch.zeros(self.buf.numel(), dtype=torch.bool, device=dev)
        idx = self.view.storage_offset() + torch.arange(rows, device=dev)[:, None] * self.view.stride(0) + torch.arange(cols, device=dev)[None, :]
        mask[idx.reshape(-1)] = True
        return mask

    def outside(self):
        """the buffer's elements that are not logical elements of the operand"""
        return self.buf[~self._logical()]

    def _damaged(self):
        """mask over the buffer: True where an element no longer holds the fill"""
        return ~torch.isnan(self.buf) if self.by_nan else bits(self.buf) != self.fill_bits

    def damage(self, cols=None):
        """None, or where the first element outside the operand that no longer holds the fill lies: "<name>: <before the operand | behind
        the operand | in row padding> at (row r, column c)", row and column counted from the operand's first element in units of its
        pitch (so a store one past the last row reads row `rows`, column 0).  `cols` declares another logical width than the operand's."""
        bad = (self._damaged() & ~self._logical(cols)).nonzero()
        if bad.numel() == 0:
            return None
        i = int(bad[0]) - self.view.storage_offset()
        rows, pitch = self.view.shape[0], self.view.stride(0)
        cols = self.view.shape[1] if cols is None else cols
        where = "before the operand" if i < 0 else ("behind the operand" if i >= (rows - 1) * pitch + cols else "in row padding")
        return f"{self.name}: {where} at (row {i // pitch}, column {i % pitch}), {int(bad.numel())} element(s) in all"

    def intact(self):
        """everything outside the operand still holds the fill value (fill=nan compares by isnan, everything else bit for bit)"""
        return self.damage() is None

    def untouched(self):
        """the WHOLE buffer still holds the fill value (a refused call)"""
        return not bool(self._damaged().any())


def arena(rows, cols, pitch=None, offset=0, fill=float("nan"), data=None, device="cpu", dtype=torch.float32, name="operand"):
    """[rows, cols] operand at element offset `offset` behind a 16-byte boundary, rows `pitch` (default cols) elements apart, everything else
    `fill`; `data` ([rows, cols] or broadcastable) is copied into the operand, which otherwise holds `fill` too."""
    pitch = cols if pitch is None else pitch
    assert pitch >= cols and rows >= 1 and cols >= 1 and offset >= 0
    n = 2 * MARGIN + offset + rows * pitch
    if isinstance(fill, str):
        assert fill == POISON and dtype in POISON_BITS, (fill, dtype)
        buf = torch.full((n,), POISON_BITS[dtype], dtype=_INT_VIEW[dtype], device=device).view(dtype)
    elif dtype == torch.bool:                      # a byte buffer seen as bool inside the operand only (a margin byte is no valid bool)
        buf = torch.full((n,), fill, dtype=torch.uint8, device=device)
    else:
        buf = torch.full((n,), fill, dtype=dtype, device=device)
    view = buf.as_strided((rows, cols), (pitch, 1), MARGIN + offset)
    a = Arena(buf, view, fill, name)
    if dtype == torch.bool:
        view.copy_(torch.zeros((), dtype=torch.uint8) if data is None else torch.as_tensor(data).to(torch.uint8))
        a.view = view.view(torch.bool)
    elif data is not None:
        view.copy_(data)
    return a


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
