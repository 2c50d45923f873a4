"""The guarded buffers of tests/guarded.py, held to what the GPU suites rely on - on `cpu` tensors, with writes planted by hand: a
one-word write in either band is reported, an output element left unwritten is reported, a fully written output is not, and two
identical fills have equal bits.  This is the proof that a guard trips; no GPU test makes a kernel overrun to show it."""
import pytest
import torch

from tests import cnn_cases as cc
from tests import guarded as gd
from tests.gemm_ref import GUARD, SENTINEL

DTYPES = [torch.float32, torch.float16, torch.int32, torch.uint8]


def _value(dtype):
    return 3 if dtype in (torch.int32, torch.uint8) else 1.5


def test_cnn_cases_reexports_the_same_objects():
    assert cc.Guarded is gd.Guarded and cc.workspace is gd.workspace


def test_the_poison_word_is_below_every_integer_a_contract_names():
    assert gd.POISON == -1515870811 and gd.POISON < -1
    assert (gd.POISON & 0xFF) == 165 and all(((gd.POISON >> s) & 0xFF) > 4 for s in (0, 8, 16, 24))
    assert gd.POISON != SENTINEL - (1 << 32) and gd.POISON != SENTINEL


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["front_first", "front_last", "back_first", "back_last"])
def test_a_planted_write_in_a_band_of_an_output_is_reported(dtype, where):
    g = gd.Guarded((3, 8), "cpu", dtype=dtype)
    assert g.outside_untouched()
    at = {"front_first": 0, "front_last": GUARD - 1, "back_first": GUARD + g.words, "back_last": GUARD + g.words + GUARD - 1}[where]
    keep = int(g.buf[at])
    g.buf[at] = keep ^ 1                                        # one bit of one word
    assert not g.outside_untouched()
    g.buf[at] = keep
    assert g.outside_untouched()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_planted_write_in_a_band_of_an_operand_is_reported(dtype):
    data = torch.full((2, 4), _value(dtype), dtype=dtype)
    g = gd.Guarded((2, 4), "cpu", data=data, dtype=dtype, band=7)
    assert g.outside_untouched() and torch.equal(g.t, data) and not g.has_unwritten()
    for at in (GUARD - 1, GUARD + g.words):
        keep = int(g.buf[at])
        g.buf[at] = 0x12345678
        assert not g.outside_untouched()
        g.buf[at] = keep
    assert g.outside_untouched()
    if dtype in (torch.int32, torch.uint8):                     # an integer operand's bands hold the caller's harmless value
        assert int(g.buf[0]) == 7 and int(g.buf[-1]) == 7
    else:                                                       # a floating-point operand's hold NaN
        assert bool(torch.isnan(g.buf[:GUARD].view(dtype)).all()) and bool(torch.isnan(g.buf[GUARD + g.words:].view(dtype)).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_unwritten_element_is_reported_and_a_fully_written_output_is_not(dtype):
    g = gd.Guarded((4, 4), "cpu", dtype=dtype)
    assert g.has_unwritten() and g.all_unwritten()
    g.t.fill_(_value(dtype))
    assert not g.has_unwritten() and not g.all_unwritten() and g.outside_untouched()
    for i, j in ((0, 0), (3, 3), (1, 2)):                       # one element left out, wherever it is
        h = gd.Guarded((4, 4), "cpu", dtype=dtype)
        keep = h.t[i, j].clone()
        h.t.fill_(_value(dtype))
        h.t[i, j] = keep
        assert h.has_unwritten() and not h.all_unwritten()
    if dtype in (torch.float32, torch.float16):
        assert not g.has_nan()
        g.t[2, 1] = float("nan")
        assert g.has_nan() and g.has_unwritten()
    else:                                                       # every value a contract names is a written one: -1, 0, large counts
        for v in ((-1, 0, 2 ** 31 - 1) if dtype == torch.int32 else (0, 4, 255)):
            g.t.fill_(v)
            assert not g.has_unwritten()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bits_of_two_identical_fills_are_equal(dtype):
    a, b = gd.Guarded((5, 4), "cpu", dtype=dtype), gd.Guarded((5, 4), "cpu", dtype=dtype)
    assert torch.equal(a.bits(), b.bits())                      # poisoned alike (NaN != NaN as floats: the bits compare)
    a.t.fill_(_value(dtype))
    assert not torch.equal(a.bits(), b.bits())
    b.t.fill_(_value(dtype))
    assert torch.equal(a.bits(), b.bits()) and a.bits().numel() == a.words


def test_workspace_is_exact_and_poisoned():
    assert gd.workspace(0, "cpu") is None
    w = gd.workspace(48, "cpu")
    assert w.words == 12 and w.has_nan() and w.all_unwritten() and w.outside_untouched() and w.ptr % 16 == 0
    w.buf[GUARD + 12] = 0                                       # the first word behind the reported size
    assert not w.outside_untouched()


def test_rows_with_a_stride_hold_the_fill_past_every_length():
    labels, lens = gd.pack_labels([[[1, 2, 3], None], [[], [4] * 9]], 6, 5)
    assert tuple(labels.shape) == (2, 2, 6) and labels.dtype == torch.int32 and lens.tolist() == [[3, -1], [0, 9]]
    assert labels[0, 0].tolist() == [1, 2, 3, 5, 5, 5] and labels[0, 1].tolist() == [5] * 6
    assert labels[1, 0].tolist() == [5] * 6 and labels[1, 1].tolist() == [4] * 6
    rows, n = gd.pack_rows([[2], [1, 1]], 3, 9)
    assert rows.tolist() == [[2, 9, 9], [1, 1, 9]] and n.tolist() == [1, 2]
