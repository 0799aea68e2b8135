"""The yardsticks of tests/test_gpu_mlp_edges.py and tests/test_gpu_gemm_memory.py, checked where no GPU is needed: the float64 restatement
of the one-launch ConvEncoder (tests/arena.py: conv_encoder_ref, on the raw matrices of pbhc_conv_encoder_fwd's ABI) equals the module's
nn.Conv1d form (agents/agent_modules.ConvEncoder, encoder_modules.py:22-107 of the reference) with the weights re-laid-out as the module's
own `_layout_weights` does, and the arena helper returns views with the offset, pitch and poison it promises."""
import math

import pytest
import torch

from tests.arena import MARGIN, SENT, arena, conv_encoder_ref


@pytest.mark.parametrize("act", ["ReLU", "SiLU", "ELU"])
@pytest.mark.parametrize("T", [5, 10, 20])
def test_conv_encoder_restatement_equals_the_module(T, act):
    from pbhc_amd.agents import agent_modules as am

    torch.manual_seed(T)
    d, H, E, M = 13, 24, 19, 7
    enc = am.ConvEncoder({"x": d}, {"input_dim": ["x"], "hidden_dim": H, "output_dim": E, "layer_config": {"type": "Conv1d", "activation": act}}, T).double()
    enc.unfold_gemm = False                                     # the nn.Conv1d form
    x = torch.randn(M, T * d, dtype=torch.float64)
    with torch.no_grad():
        want = enc(x)
        wc1, wc2, wo = enc._layout_weights()
        (k1, k2), (s1, s2) = am._CONV_TABLE[T][1], am._CONV_TABLE[T][2]
        c1, c2 = enc.conv_module[0], enc.conv_module[2]
        got = conv_encoder_ref(x, enc.encoder[0].weight, enc.encoder[0].bias, wc1, c1.bias, wc2, c2.bias, wo, enc.output_layer.bias, T, d, k1, s1, k2, s2,
                               {"ELU": 1, "SiLU": 2, "ReLU": 3}[act])
    assert got.shape == want.shape == (M, E)
    err = (got - want).abs().max().item()
    print(f"ERR encoder restatement T={T} {act}: {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("fill", [float("nan"), SENT])
@pytest.mark.parametrize("rows,cols,pitch,offset", [(1, 1, None, 0), (5, 13, 16, 1), (3, 7, 7, 3), (4, 8, 20, 4)])
def test_arena_views_have_the_offset_pitch_and_poison_they_promise(rows, cols, pitch, offset, fill):
    data = torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols)
    a = arena(rows, cols, pitch, offset, fill, data)
    p = cols if pitch is None else pitch
    same = (lambda t: torch.isnan(t).all()) if math.isnan(fill) else (lambda t: (t == fill).all())
    assert a.view.shape == (rows, cols) and a.view.stride() == (p, 1) and a.view.storage_offset() == MARGIN + offset
    assert a.buf.data_ptr() % 16 == 0 and (a.ptr() - a.buf.data_ptr()) == 4 * (MARGIN + offset)
    assert a.buf.numel() >= MARGIN + offset + (rows - 1) * p + cols + MARGIN
    assert torch.equal(a.view, data)
    assert same(a.buf[:MARGIN + offset]) and same(a.buf[MARGIN + offset + (rows - 1) * p + cols:])
    for r in range(rows - 1):
        assert same(a.buf[MARGIN + offset + r * p + cols:MARGIN + offset + (r + 1) * p])
    assert a.outside().numel() == a.buf.numel() - rows * cols and a.intact() and not a.untouched()
    # a store one float outside the operand — before it, behind a row, behind the last row — is seen; one inside is not
    for pos in (MARGIN + offset - 1, MARGIN + offset + cols if p > cols or rows == 1 else None, MARGIN + offset + (rows - 1) * p + cols):
        if pos is None:
            continue
        keep = a.buf[pos].clone()
        a.buf[pos] = 1.0
        assert not a.intact()
        a.buf[pos] = keep
        assert a.intact()
    a.view[rows - 1, cols - 1] = 2.0
    assert a.intact()
    assert arena(rows, cols, pitch, offset, fill).untouched()
