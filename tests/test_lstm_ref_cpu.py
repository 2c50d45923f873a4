"""CPU: the BiLSTM restatement of tests/lstm_ref.py against torch.nn.LSTM in double precision on packed sequences, and the bars of
tests/test_lstm_fp64_gpu.py against kernels that are wrong on purpose (mutants of the fp32 restatement at the bench shape's regime)."""
import pytest
import torch

from tests import lstm_ref as lr


@pytest.fixture(scope="module", autouse=True)
def _cpu_threads():
    """the CPU references at no more than 16 threads (what a GPU host gives one command); the caller's count is restored afterwards"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)


def _inputs(T, B, H, lens, seed, w_scale=0.08, x_scale=0.5):
    g = torch.Generator().manual_seed(seed)
    xproj = (torch.rand(2, T, B, 4 * H, generator=g, dtype=torch.float64) * 2 - 1) * x_scale
    whh = (torch.rand(2, 4 * H, H, generator=g, dtype=torch.float64) * 2 - 1) * w_scale
    dy = torch.rand(T, B, 2 * H, generator=g, dtype=torch.float64) * 2 - 1
    for b in range(B):                       # junk past the lengths must not leak
        xproj[:, lens[b]:, b] = 7.0
        dy[lens[b]:, b] = 3.0
    return xproj, whh, dy


def _nn_lstm(xproj, whh, lens, dy):
    """nn.LSTM (double) whose input IS the pre-activation: input [x_f | x_r] of width 8H, W_ih = [I 0] / [0 I], zero biases."""
    _, T, B, G = xproj.shape
    H = G // 4
    m = torch.nn.LSTM(2 * G, H, num_layers=1, bidirectional=True).double()
    eye = torch.eye(G, dtype=torch.float64)
    z = torch.zeros(G, G, dtype=torch.float64)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.cat((eye, z), 1))
        m.weight_ih_l0_reverse.copy_(torch.cat((z, eye), 1))
        m.weight_hh_l0.copy_(whh[0])
        m.weight_hh_l0_reverse.copy_(whh[1])
        for nm in ("bias_ih_l0", "bias_hh_l0", "bias_ih_l0_reverse", "bias_hh_l0_reverse"):
            getattr(m, nm).zero_()
    x = torch.cat((xproj[0], xproj[1]), 2).clone().requires_grad_(True)
    out, _ = m(torch.nn.utils.rnn.pack_padded_sequence(x, lens))
    y, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
    y.backward(dy)
    return y.detach(), torch.stack((x.grad[..., :G], x.grad[..., G:]))


@pytest.mark.parametrize("T,B,H,lens", [(9, 4, 8, [9, 7, 3, 1]), (6, 3, 16, [6, 6, 6]), (1, 2, 8, [1, 1]), (5, 1, 16, [5]),
                                        (12, 6, 32, [12, 11, 11, 5, 2, 1])])
def test_fp64_restatement_is_nn_lstm(T, B, H, lens):
    xproj, whh, dy = _inputs(T, B, H, lens, seed=T * 100 + B, w_scale=0.4, x_scale=2.0)
    y_nn, dg_nn = _nn_lstm(xproj, whh, lens, dy)
    y, gates, cell = lr.lstm_fwd(xproj, whh, lens)
    dg, db = lr.lstm_bwd(dy, whh, lens, gates, cell)
    assert float((y - y_nn).abs().max()) <= 1e-12
    assert float((dg - dg_nn).abs().max()) <= 1e-10
    assert torch.allclose(db, dg_nn.sum(dim=(1, 2)), rtol=0, atol=1e-10)
    inv = ~lr.valid_mask(T, B, lens)
    assert (y[inv] == 0).all() and (dg[:, inv] == 0).all() and (gates[:, inv] == 0).all() and (cell[:, inv] == 0).all()
    # the layouts: gates [2][T][B][H][4] post-activation interleaved per unit, cell [2][T][B][H], h = o tanh(c) in y's direction halves
    i, f, g, o = gates.unbind(-1)
    assert (i >= 0).all() and (i <= 1).all() and (g.abs() <= 1).all()
    for d in range(2):
        assert torch.allclose(y[:, :, d * H:(d + 1) * H], o[d] * torch.tanh(cell[d]), rtol=0, atol=1e-15)
    # the reverse direction starts at each row's own last frame with zero state: its first cell is i * g there
    for b in range(B):
        t = lens[b] - 1
        assert torch.allclose(cell[1, t, b], i[1, t, b] * g[1, t, b], rtol=0, atol=1e-15)
        assert torch.allclose(cell[0, 0, b], i[0, 0, b] * g[0, 0, b], rtol=0, atol=1e-15)


def test_dy_mask_is_a_product_with_dy():
    T, B, H, lens = 7, 5, 16, [7, 6, 4, 4, 1]
    xproj, whh, dy = _inputs(T, B, H, lens, seed=3)
    mask = (torch.rand(T, B, 2 * H, generator=torch.Generator().manual_seed(4)) > 0.3).double() / 0.7
    _, gates, cell = lr.lstm_fwd(xproj, whh, lens)
    a = lr.lstm_bwd(dy, whh, lens, gates, cell, dy_mask=mask)
    b = lr.lstm_bwd(dy * mask, whh, lens, gates, cell)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# the bench shape's regime (T = 294, B = 32, H = 512, reference init), ragged with the last length 1: what the GPU bars must catch
_T, _B, _H = 294, 32, 512
_LENS = sorted([max(1, _T - (_T * i) // (_B - 1)) for i in range(_B)], reverse=True)


@pytest.fixture(scope="module")
def bench_case():
    xproj, whh, dy = _inputs(_T, _B, _H, _LENS, seed=11)
    mask = (torch.rand(_T, _B, 2 * _H, generator=torch.Generator().manual_seed(12)) > 0.5).double() * 2.0
    return xproj, whh, dy, mask, lr.Refs(xproj, whh, _LENS, dy, mask)


def test_the_fp32_restatement_holds_the_bars(bench_case):
    xproj, whh, dy, mask, refs = bench_case
    assert _LENS[-1] == 1 and _LENS[0] == _T
    errs = refs.errors(refs.f32, refs.b32)
    assert not lr.failures(errs), errs
    for nm, ek, e32, b in errs:
        assert 0 < e32 < b


@pytest.mark.parametrize("mutant", lr.MUTANTS)
def test_the_bars_reject_a_wrong_recurrence(bench_case, mutant):
    xproj, whh, dy, mask, refs = bench_case
    fwd = lr.lstm_fwd(xproj, whh, _LENS, torch.float32, mutant=mutant)
    bwd = lr.lstm_bwd(dy, whh, _LENS, fwd[1], fwd[2], mask, torch.float32, mutant=mutant)
    bad = lr.failures(refs.errors(fwd, bwd))
    assert bad, "mutant %r passes every bar" % mutant
    if mutant == "no_mask":
        assert [nm for nm, *_ in bad] == ["dgates", "dbias"]
    else:
        assert "y" in [nm for nm, *_ in bad]
