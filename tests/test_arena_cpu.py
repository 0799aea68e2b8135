"""tests/arena.py itself, on the CPU: what the memory-edge tests rely on when they call `intact()` / `damage()` / `untouched()` — bit-exact
poison, row padding, integer operands and the failure report."""
import pytest
import torch

from tests.arena import MARGIN, POISON, POISON_BITS, SENT, arena, bits


def test_poison_is_a_nan_with_the_fixed_payload_and_a_fresh_arena_is_untouched():
    a = arena(3, 5, pitch=8, fill=POISON, name="x")
    assert bool(torch.isnan(a.buf).all())
    assert int(bits(a.buf)[0]) == POISON_BITS[torch.float32] == 0x7FC0A5A5
    assert a.untouched() and a.intact() and a.damage() is None
    d = arena(2, 3, fill=POISON, dtype=torch.float64)
    assert int(bits(d.buf)[0]) == POISON_BITS[torch.float64] and bool(torch.isnan(d.buf).all()) and d.untouched()


def test_a_nan_of_another_payload_in_a_margin_is_found_under_poison_and_not_under_plain_nan():
    other = torch.tensor([0x7FC00001], dtype=torch.int32).view(torch.float32)          # a quiet NaN, another payload
    a = arena(3, 5, pitch=8, fill=POISON, data=torch.zeros(3, 5), name="state")
    assert a.intact()
    a.buf[MARGIN - 1:MARGIN] = other
    assert bool(torch.isnan(a.buf[MARGIN - 1]))
    assert not a.intact() and not a.untouched()
    assert a.damage() == "state: before the operand at (row -1, column 7), 1 element(s) in all"
    # the arena the GEMM / MLP tests use (fill=nan) keeps its rule: any NaN counts as untouched
    b = arena(3, 5, pitch=8, data=torch.zeros(3, 5))
    b.buf[MARGIN - 1:MARGIN] = other
    assert b.intact()
    b.buf[MARGIN - 1] = 0.0
    assert not b.intact()


@pytest.mark.parametrize("fill", [POISON, SENT, float("nan")])
def test_a_store_into_row_padding_is_found_and_a_store_into_a_logical_element_is_not(fill):
    a = arena(4, 5, pitch=8, offset=3, fill=fill, name="obs")
    a.view[2, 4] = 1.5                                   # the last logical column
    a.view[0, 0] = float("nan")                          # any value may be stored inside the operand, a NaN included
    assert a.intact() and a.damage() is None and not a.untouched()
    a.buf[MARGIN + 3 + 2 * 8 + 5] = 1.5                  # row 2, first padding column
    assert not a.intact()
    assert a.damage() == "obs: in row padding at (row 2, column 5), 1 element(s) in all"


def test_the_report_tells_before_behind_and_padding_apart_and_names_the_first_element():
    a = arena(3, 4, pitch=6, fill=SENT, name="y")
    last = MARGIN + 2 * 6 + 4                            # one past the last logical element
    a.buf[last] = 0.0
    a.buf[last + 7] = 0.0
    assert a.damage() == "y: behind the operand at (row 2, column 4), 2 element(s) in all"
    a = arena(3, 4, pitch=6, fill=SENT, name="y")
    a.buf[MARGIN + 3 * 6] = 0.0
    assert a.damage() == "y: behind the operand at (row 3, column 0), 1 element(s) in all"
    a = arena(3, 4, pitch=6, fill=SENT, name="y")
    a.buf[0] = 0.0
    assert a.damage().startswith("y: before the operand at (row ")


def test_a_narrower_declared_width_turns_the_last_column_into_padding():
    a = arena(3, 4, pitch=6, fill=POISON, name="torques")
    a.view.copy_(torch.ones(3, 4))
    assert a.damage() is None
    assert a.damage(cols=3) == "torques: in row padding at (row 0, column 3), 3 element(s) in all"
    dense = arena(3, 4, fill=POISON, name="torques")
    dense.view.copy_(torch.ones(3, 4))
    assert dense.damage(cols=3).startswith("torques: in row padding at (row 0, column 3)")


@pytest.mark.parametrize("dtype,fill", [(torch.int64, 1 << 20), (torch.int32, 0), (torch.uint8, 0xA5), (torch.float64, POISON)])
def test_integer_and_f64_arenas(dtype, fill):
    data = torch.arange(6).reshape(1, 6).to(dtype)
    a = arena(1, 6, fill=fill, data=data, dtype=dtype, name="ids")
    assert a.view.dtype == dtype and torch.equal(a.view, data)
    assert a.buf.numel() == 2 * MARGIN + 6 and a.outside().numel() == 2 * MARGIN
    assert a.intact() and not a.untouched()
    if fill is not POISON:
        assert bool((a.outside() == fill).all())
    a.view[0, 5] = 3
    assert a.intact()
    a.buf[MARGIN + 6] = 1
    assert a.damage() == "ids: behind the operand at (row 1, column 0), 1 element(s) in all"   # dense rows: one past the end is row 1
    fresh = arena(2, 3, pitch=4, fill=fill, dtype=dtype)
    assert fresh.untouched()
    fresh.buf[MARGIN + 3] = 1
    assert fresh.damage() == "operand: in row padding at (row 0, column 3), 1 element(s) in all"


def test_bool_arena_is_a_byte_buffer_seen_as_bool_inside_the_operand():
    a = arena(1, 5, fill=0xA5, dtype=torch.bool, data=torch.tensor([[1, 0, 1, 0, 0]]), name="time_out_buf")
    assert a.view.dtype == torch.bool and a.view[0].tolist() == [True, False, True, False, False]
    assert a.buf.dtype == torch.uint8 and a.intact()
    a.view[0, 1] = True
    assert a.intact()
    a.buf[MARGIN + 5] = 1                                # a stray `true` behind the operand
    assert a.damage() == "time_out_buf: behind the operand at (row 1, column 0), 1 element(s) in all"
