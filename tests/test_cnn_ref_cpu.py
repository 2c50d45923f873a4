"""CPU: the CNN restatement of tests/cnn_ref.py against torch's float64 modules (conv2d and its gradients, batch_norm with running
statistics) and ATen's fp32 fractional_max_pool2d indices; the bars of tests/test_cnn_fp64_gpu.py against computations that are wrong
on purpose (every mutant misses its bar by at least 10x), and fp32 CPU results that must pass them.  The same two questions for the seam
tables of tests/cnn_cases.py (tests/test_cnn_seams_gpu.py): an honest fp32 convolution holds the bars on every small shape, each seam
mutant misses its bar by 10x on at least one."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cnn_cases as cc
from tests import cnn_ref as cr


@pytest.fixture(scope="module", autouse=True)
def _cpu_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)


def _rand(shape, seed, scale=1.0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).to(dtype)


@pytest.mark.parametrize("n,cin,h,w,cout", [(2, 3, 5, 7, 4), (1, 1, 1, 9, 8), (3, 8, 4, 1, 2), (2, 16, 6, 11, 12)])
def test_conv_restatement_is_torch_float64(n, cin, h, w, cout):
    x, wt, b, dy = _rand((n, cin, h, w), 1), _rand((cout, cin, 3, 3), 2), _rand((cout,), 3), _rand((n, cout, h, w), 4)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, wt, b))
    y = F.conv2d(xr, wr, br, padding=1)
    y.backward(dy)
    assert float((cr.conv3x3(x, wt, b) - y.detach()).abs().max()) <= 1e-13
    assert float((cr.conv3x3_dgrad(dy, wt) - xr.grad).abs().max()) <= 1e-13
    assert float((cr.conv3x3_wgrad(x, dy) - wr.grad).abs().max()) <= 1e-12
    assert float((dy.sum((0, 2, 3)) - br.grad).abs().max()) <= 1e-13
    # the scale is the same conv on absolute values, and bounds |y|
    s = cr.conv3x3(x, wt, b, absolute=True)
    assert torch.allclose(s, F.conv2d(x.abs(), wt.abs(), b.abs(), padding=1), rtol=0, atol=1e-13)
    assert bool((y.detach().abs() <= s + 1e-13).all())
    assert torch.allclose(cr.conv3x3_wgrad(x, dy, absolute=True), torch.nn.grad.conv2d_weight(x.abs(), wt.shape, dy.abs(), padding=1),
                          rtol=0, atol=1e-12)


def test_bn_restatement_is_torch_batch_norm():
    n, c, h, w = 3, 5, 4, 7
    y = _rand((n, c, h, w), 1, 2.0) + torch.arange(c, dtype=torch.float64).view(1, c, 1, 1)
    gamma, beta = _rand((c,), 2) + 1.5, _rand((c,), 3)
    rm0, rv0 = _rand((c,), 4), _rand((c,), 5) + 2.0
    rm, rv = rm0.clone(), rv0.clone()
    yr, gr, br = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
    pre = F.batch_norm(yr, rm, rv, gr, br, training=True, momentum=0.1, eps=1e-5)
    mean, invstd, var, rm1, rv1 = cr.bn_stats(y, rm0, rv0, 0.1, 1e-5)
    assert torch.allclose(rm1, rm, rtol=0, atol=1e-14) and torch.allclose(rv1, rv, rtol=0, atol=1e-14)
    assert torch.allclose(cr.bn_relu_pre(y, mean, invstd, gamma, beta), pre.detach(), rtol=0, atol=1e-13)
    da = _rand((n, c, h, w), 6)
    out = torch.relu(pre)
    out.backward(da)
    dy, dgamma, dbeta = cr.bn_relu_bwd(da, y, pre.detach() > 0, mean, invstd, gamma)
    assert torch.allclose(dy, yr.grad, rtol=0, atol=1e-12) and torch.allclose(dgamma, gr.grad, rtol=0, atol=1e-12)
    assert torch.allclose(dbeta, br.grad, rtol=0, atol=1e-12)
    assert float(dy.sum((0, 2, 3)).abs().max()) < 1e-12                  # the conv-bias gradient in front: 0
    # eval mode: the running statistics normalise
    rm2, rv2 = rm0.clone(), rv0.clone()
    ev = F.batch_norm(y, rm2, rv2, gamma, beta, training=False, eps=1e-5)
    assert torch.allclose(cr.bn_relu_pre(y, rm0, 1.0 / (rv0 + 1e-5).sqrt(), gamma, beta), ev, rtol=0, atol=1e-13)
    # a per-channel count of 1: var = 0, running_var takes the biased (zero) variance as the kernels do
    m1, is1, v1, _, rv_1 = cr.bn_stats(y[:1, :, :1, :1], rm0, rv0, 0.1, 1e-5)
    assert float(v1.abs().max()) == 0.0 and torch.allclose(rv_1, 0.9 * rv0, rtol=0, atol=1e-15)


@pytest.mark.parametrize("h,w,oh,ow", [(30, 600, 15, 420), (15, 420, 7, 294), (30, 1178, 15, 824), (7, 9, 3, 6), (5, 3, 2, 2)])
def test_pool_windows_are_atens_fp32_rule(h, w, oh, ow):
    n, c = 2, 3
    x = _rand((n, c, h, w), h * w, dtype=torch.float32)
    u = torch.rand(n, c, 2, generator=torch.Generator().manual_seed(ow))
    u[0, 0] = torch.tensor([0.0, 0.0])
    u[0, 1] = float(np.float32(1.0) - np.float32(2.0 ** -24))
    ref, idx = F.fractional_max_pool2d(x, 2, output_size=(oh, ow), _random_samples=u, return_indices=True)
    out, bidx = cr.fracpool2x2(x, u, oh, ow)
    assert torch.equal(out, ref) and torch.equal(bidx, idx)
    dout = _rand((n, c, oh, ow), 7, dtype=torch.float32)
    xr = x.clone().requires_grad_(True)
    F.fractional_max_pool2d(xr, 2, output_size=(oh, ow), _random_samples=u).backward(dout)
    # a pixel that wins several windows sums their gradients: fp32 in ATen's order against the exact sum, within one rounding per term
    assert cr.ratio(xr.grad, cr.pool_scatter(dout, idx, h, w), cr.pool_bwd_bar(dout, idx, h, w)) <= 1.0


def test_relu_maxpool_restatement():
    x = _rand((2, 3, 7, 9), 1, dtype=torch.float32)
    ref, idx = F.max_pool2d(torch.relu(x), 2, stride=2, return_indices=True)
    out, bidx = cr.relu_maxpool2(x)
    assert torch.equal(out, ref)
    # ties (ReLU zeros) may pick another winner than ATen: the index must point at a maximum of its window
    assert torch.equal(torch.gather(torch.relu(x).reshape(2, 3, -1), 2, bidx.reshape(2, 3, -1)).view_as(out), out)


# ---------------------------------------------------------------------------------------------------- bars: fp32 passes, mutants fail
_CONV = (4, 24, 6, 40, 32)                     # n, cin, h, w, cout: K = 216 per output


@pytest.fixture(scope="module")
def conv_case():
    n, cin, h, w, cout = _CONV
    x, wt, b, dy = _rand((n, cin, h, w), 11), _rand((cout, cin, 3, 3), 12, 0.2), _rand((cout,), 13), _rand((n, cout, h, w), 14)
    x32, w32, b32, dy32 = (t.float().double() for t in (x, wt, b, dy))
    return dict(x=x32, w=w32, b=b32, dy=dy32, y=cr.conv3x3(x32, w32, b32), s=cr.conv3x3(x32, w32, b32, absolute=True),
                dx=cr.conv3x3_dgrad(dy32, w32), sdx=cr.conv3x3_dgrad(dy32, w32, absolute=True),
                dw=cr.conv3x3_wgrad(x32, dy32), sdw=cr.conv3x3_wgrad(x32, dy32, absolute=True))


def test_fp32_conv_holds_the_bars(conv_case):
    k = conv_case
    y = F.conv2d(k["x"].float(), k["w"].float(), k["b"].float(), padding=1)
    dx = torch.nn.grad.conv2d_input(k["x"].shape, k["w"].float(), k["dy"].float(), padding=1)
    dw = torch.nn.grad.conv2d_weight(k["x"].float(), k["w"].shape, k["dy"].float(), padding=1)
    for got, ref, s in ((y, k["y"], k["s"]), (dx, k["dx"], k["sdx"]), (dw, k["dw"], k["sdw"])):
        r = cr.ratio(got, ref, cr.conv_bar("direct", s))
        assert r <= 1.0, r
    # the tightest bar of all (direct form, 8 U s) is not vacuous: it is within 1000x of the fp32 rounding of the result itself
    assert float(cr.conv_bar("direct", k["s"]).max()) < 1000 * cr.U * float(k["y"].abs().max())


@pytest.mark.parametrize("mutant", ["tap", "last4_cin", "tail_piece"])
def test_the_conv_bars_reject_a_wrong_kernel(conv_case, mutant):
    k = conv_case
    got = cr.conv_mutant(k["x"], k["w"], k["b"], mutant)
    loosest = max(cr.CONV_C.values())
    r = cr.ratio(got, k["y"], loosest * cr.U * k["s"])
    assert r >= 10.0, "mutant %r only %.1fx its loosest bar" % (mutant, r)


def test_the_wgrad_bar_rejects_a_dropped_slab(conv_case):
    k = conv_case
    got = cr.wgrad_mutant(k["x"], k["dy"])
    r = cr.ratio(got, k["dw"], cr.CONV_C["wgrad"] * cr.U * k["sdw"])
    assert r >= 10.0, r


def _bn_errors(y, rm0, rv0, mutant=None, momentum=0.1, eps=1e-5):
    """max error / bar of the fp32 statistics (a CPU fp32 pass, or a mutant's fp64 one rounded to fp32) against the fp64 restatement."""
    mean, invstd, var, rm, rv = cr.bn_stats(y, rm0, rv0, momentum, eps)
    cnt = y.numel() // y.shape[1]
    e_mean, e_is, e_var = cr.bn_stat_bars(mean, var, invstd)
    brm, brv = cr.running_bars(rm0, rv0, mean, var * cnt / max(cnt - 1, 1), e_mean, e_var, momentum, cnt)
    if mutant is None:                     # an honest fp32 implementation: double sums, one rounding, fp32 running update
        yd = y.double().transpose(0, 1).reshape(y.shape[1], -1)
        s, q = yd.sum(1), (yd * yd).sum(1)
        m = s / cnt
        v = (q / cnt - m * m).clamp_min(0)
        g = (m.float(), (1.0 / (v + eps).sqrt()).float())
        ub = (v * cnt / (cnt - 1)).float()
        grm = (1 - momentum) * rm0.float() + momentum * m.float()
        grv = (1 - momentum) * rv0.float() + momentum * ub
    else:
        km, kis, _, krm, krv = cr.bn_stats(y, rm0, rv0, momentum, eps, mutant=mutant)
        g, grm, grv = (km.float(), kis.float()), krm.float(), krv.float()
    return {"mean": cr.ratio(g[0], mean, e_mean), "invstd": cr.ratio(g[1], invstd, e_is * invstd),
            "running_mean": cr.ratio(grm, rm, brm), "running_var": cr.ratio(grv, rv, brv)}


def test_fp32_bn_statistics_hold_the_bars_and_mutants_fail():
    y = (_rand((4, 6, 9, 37), 21, 1.0, torch.float32) + 0.7)
    rm0, rv0 = _rand((6,), 22).float().double(), (_rand((6,), 23) + 2).float().double()
    honest = _bn_errors(y, rm0, rv0)
    assert max(honest.values()) <= 1.0, honest
    for mutant, what in (("biased_rv", "running_var"), ("eps_out", "invstd")):
        r = _bn_errors(y, rm0, rv0, mutant)[what]
        assert r >= 10.0, (mutant, what, r)
    # |mean| / sigma = 1e4: the fp32 design still holds its bars
    big = (_rand((2, 3, 5, 40), 24, 1.0) + 1e4).float()
    assert max(_bn_errors(big, rm0[:3], rv0[:3]).values()) <= 1.0


def test_the_stat_bar_rejects_a_skipped_last_vector():
    # 36 chunks of 16384 per channel (a batch-32 30x600 layer has 576 000 elements per channel): the last vector of the last one skipped
    y = (_rand((32, 2, 30, 600), 31, 1.0, torch.float32) + 0.5)
    rm0, rv0 = torch.zeros(2, dtype=torch.float64), torch.ones(2, dtype=torch.float64)
    r = _bn_errors(y, rm0, rv0, "last_vec")["mean"]
    assert r >= 10.0, r


def test_bn_apply_and_backward_bars():
    n, c, h, w = 3, 4, 6, 21
    y = _rand((n, c, h, w), 41, 1.0, torch.float32)
    y[:, 1] += 1e4                                                           # |mean| / sigma = 1e4 in one channel
    gamma, beta = (_rand((c,), 42) * 0.3 + 1).float(), (_rand((c,), 43) * 0.2).float()
    da = _rand((n, c, h, w), 44, 1.0, torch.float32)
    mean, invstd, var, _, _ = cr.bn_stats(y)
    e_mean, e_is, _ = cr.bn_stat_bars(mean, var, invstd)
    m32, is32 = mean.float(), invstd.float()
    pre32 = (y - m32.view(1, c, 1, 1)) * is32.view(1, c, 1, 1) * gamma.view(1, c, 1, 1) + beta.view(1, c, 1, 1)
    out32 = torch.relu(pre32)
    bar, e_xhat = cr.bn_apply_bar(y, mean, invstd, gamma, beta, e_mean, e_is)
    ref = torch.relu(cr.bn_relu_pre(y, mean, invstd, gamma, beta))
    assert cr.ratio(out32, ref, bar) <= 1.0
    # the rounding of the mean alone moves xhat by ~|mean| U invstd in the 1e4 channel: the bar must admit it, a looser design must not pass
    assert float(((out32[:, 1].double() - ref[:, 1]).abs()).max()) > 1e-5
    mask = out32 > 0
    dy, dgamma, dbeta = cr.bn_relu_bwd(da, y, mask, mean, invstd, gamma)
    b_dy, b_dg, b_db = cr.bn_bwd_bars(da, y, mask, mean, invstd, gamma, dgamma, dbeta, e_xhat)
    # an fp32 backward with the fp32 statistics (double sums, as the kernels do)
    xh = (y - m32.view(1, c, 1, 1)) * is32.view(1, c, 1, 1)
    dz = da * mask
    db32 = dz.double().sum((0, 2, 3)).float()
    dg32 = (dz.double() * xh.double()).sum((0, 2, 3)).float()
    cnt = n * h * w
    dy32 = (gamma * is32).view(1, c, 1, 1) * (dz - (db32 / cnt).view(1, c, 1, 1) - xh * (dg32 / cnt).view(1, c, 1, 1))
    for got, want, b in ((dy32, dy, b_dy), (dg32, dgamma, b_dg), (db32, dbeta, b_db)):
        assert cr.ratio(got, want, b) <= 1.0
    # the conv-bias gradient the kernels return: -gamma invstd dgamma / count * xhat_sum
    xs = ((y.double() - m32.double().view(1, c, 1, 1)) * is32.double().view(1, c, 1, 1)).sum((0, 2, 3))
    dcb = -gamma.double() * is32.double() * dg32.double() / cnt * xs
    assert bool((dcb.abs() <= cr.conv_bias_grad_bar(mean, invstd, gamma, dgamma, cnt)).all())
    # ... and a bias gradient of plain fp32 noise (sum of dy in fp32, what ATen returns) would not pass it in the 1e4 channel
    assert float(dy32[:, 1].sum()) != 0.0


def test_fp64_windows_differ_from_the_fp32_rule():
    """the "fp64 window arithmetic" mutant: some samples at the model's sizes give other window starts than ATen's fp32 rule, so the
    GPU test's exact index comparison rejects it."""
    rng = np.random.RandomState(5)
    diff = 0
    for in_size, out_size in ((600, 420), (420, 294), (30, 15), (1178, 824)):
        for u in rng.uniform(0, 1, size=300).astype(np.float32):
            diff += int((cr.fracpool_starts(u, in_size, out_size) != cr.fracpool_starts(u, in_size, out_size, np.float64)).any())
    assert diff > 0


# ------------------------------------------------------------------------------------------- the seam tables of tests/cnn_cases.py
_TABLES = [("WINO", cc.WINO_CASES, cc.WINO_AXES), ("DIRECT", cc.DIRECT_CASES, cc.DIRECT_AXES), ("H16", cc.H16_CASES, cc.H16_AXES),
           ("F16", cc.F16_CASES, cc.F16_AXES), ("WGRAD_F16", cc.WGRAD_F16_CASES, cc.WGRAD_F16_AXES)]


def test_the_seam_tables_are_short_and_cover_their_axes():
    for name, rows, axes in _TABLES:
        assert cc.covers2(rows, axes), name
        assert len(rows) <= 4 * max(len(v) for v in axes.values()), (name, len(rows))          # a cross product has hundreds
        assert len(set(rows)) == len(rows), name
    for rows, cap in ((cc.WINO_CASES, cc.SMALL_CAP), (cc.DIRECT_CASES, cc.SMALL_CAP), (cc.H16_CASES, cc.H16_CAP), (cc.F16_CASES, cc.H16_CAP)):
        assert max(n * cout * h * w for n, _, h, w, cout in rows) <= cap
    assert all(cout % 4 == 0 for *_, cout in cc.WINO_CASES) and all(cout % 4 for *_, cout in cc.DIRECT_CASES)
    assert cc.covers2([(n, h, w, (ci, co)) for n, ci, h, w, co in cc.WGRAD_CASES], cc.WGRAD_AXES)
    assert cc.covers2([((n, h), w, (ci, co)) for n, ci, h, w, co in cc.WGRAD_H16_CASES], cc.WGRAD_H16_AXES)
    assert cc.covers2(cc.LAYOUT_CASES, cc.LAYOUT_AXES)
    # the large-grid plans: one shape per W % 4, Cin = 8, outputs of 25 M elements
    assert set(cc.PLAN_CASES) | {1, 3, 4} == cc.REACHABLE_PLANS
    for plan, shapes in cc.PLAN_CASES.items():
        assert sorted(s[3] % 4 for s in shapes) == [0, 1, 2, 3] and all(s[1] == 8 for s in shapes), plan
        assert max(n * co * h * w for n, _, h, w, co in shapes) < 25.1e6
    # the weight-gradient table reaches all four kernels, an odd and an even H in each, and both reduce forms of the row-pair kernel
    kinds = {}
    for n, ci, h, w, co in cc.WGRAD_CASES:
        kinds.setdefault(cc.wgrad_kernel(ci, co)[0], set()).add(h % 2)
    assert kinds == {k: {0, 1} for k in ("rowpair", "wino3", "direct", "c1")}, kinds
    wide = [3 * ci * co // 4 < 4096 and cc.rowpair_splits(n, ci, h, w, co) >= 64 for n, ci, h, w, co in cc.WGRAD_CASES
            if cc.wgrad_kernel(ci, co)[0] == "rowpair"]
    assert any(wide) and not all(wide)


def _ops(shape, seed, f16=False):
    """fp32-representable operands of a launch (n, K, h, w, M) as float64: x [n][K], the forward filter [M][K] and its bias, the
    data-gradient layer's filter [K][M] (a layer M -> K whose gradient dy [n][K] gives dx [n][M]), dy for the weight gradient [n][M]"""
    n, k, h, w, m = shape
    r = lambda sh, i, sc=1.0: (cc.rand(sh, seed + i, sc).half() if f16 else cc.rand(sh, seed + i, sc)).double()
    return r((n, k, h, w), 1), r((m, k, 3, 3), 2, 0.2), cc.rand((m,), seed + 3).double(), r((k, m, 3, 3), 4, 0.2), r((n, m, h, w), 5)


def _honest(shape, seed, f16=False):
    """error / the direct bar (the tightest) of torch's fp32 CPU forward, data gradient and weight gradient at a launch shape"""
    x, wt, b, wd, dy = _ops(shape, seed, f16)
    n, k, h, w, m = shape
    y = F.conv2d(x.float(), wt.float(), b.float(), padding=1)
    dx = torch.nn.grad.conv2d_input((n, m, h, w), wd.float(), x.float(), padding=1)
    dw = torch.nn.grad.conv2d_weight(x.float(), wt.shape, dy.float(), padding=1)
    return (cr.ratio(y, cr.conv3x3(x, wt, b), cr.conv_bar("direct", cr.conv3x3(x, wt, b, absolute=True))),
            cr.ratio(dx, cr.conv3x3_dgrad(x, wd), cr.conv_bar("direct", cr.conv3x3_dgrad(x, wd, absolute=True))),
            cr.ratio(dw, cr.conv3x3_wgrad(x, dy), cr.conv_bar("direct", cr.conv3x3_wgrad(x, dy, absolute=True))))


@pytest.mark.parametrize("table", ["WINO", "DIRECT", "WGRAD", "H16", "F16", "WGRAD_F16", "WGRAD_H16"])
def test_an_honest_fp32_conv_holds_the_bars_on_every_small_seam_shape(table):
    """the condition that the tables are fair to a correct kernel: plain fp32 arithmetic, in torch's CPU order, stays within the
    tightest bar (8 U s) at every small shape - on the fp16-rounded operands for the fp16 tables, as the GPU test compares"""
    rows = cc.WGRAD_CASES if table == "WGRAD" else cc.WGRAD_H16_CASES if table == "WGRAD_H16" else dict((t[0], t[1]) for t in _TABLES)[table]
    worst = 0.0
    for i, shape in enumerate(rows):
        r = max(_honest(shape, 100 * i, f16="16" in table))
        assert r <= 1.0, (table, shape, r)
        worst = max(worst, r)
    print("%s: %d shapes, worst error / bar %.3f" % (table, len(rows), worst))


@pytest.mark.parametrize("mutant", cr.SEAM_CONV_MUTANTS)
def test_the_conv_bars_reject_the_seam_mutants(mutant):
    """against the LOOSEST conv bar (F(4,3): 64 U s), on the shapes of the forward table the mutant applies to"""
    hit, tried = [], 0
    for i, shape in enumerate(cc.WINO_CASES + cc.DIRECT_CASES):
        n, k, h, w, m = shape
        if (mutant == "odd_last_col" and w % 2 == 0) or (mutant == "cin_mod4" and k % 4 == 0) or (mutant == "gap_slot" and n * h == 1):
            continue
        x, wt, b, _, _ = _ops(shape, 100 * i)
        r = cr.ratio(cr.conv_mutant(x, wt, b, mutant), cr.conv3x3(x, wt, b), max(cr.CONV_C.values()) * cr.U * cr.conv3x3(x, wt, b, absolute=True))
        tried += 1
        hit.append(r >= 10.0)
    print("%s: rejected by 10x on %d of %d shapes" % (mutant, sum(hit), tried))
    assert tried >= 10 and all(hit), (mutant, sum(hit), tried)


@pytest.mark.parametrize("mutant", cr.SEAM_WGRAD_MUTANTS)
def test_the_wgrad_bars_reject_the_seam_mutants(mutant):
    """pair_lower_row / last_slab against the row-pair kernel's bar (16 U s) on the weight-gradient table (last_slab at the kernel's own
    split count); f16_pad against the fp16 bar (8 U s) on the fp16 weight-gradient table, fp16-rounded operands"""
    hit, tried = [], 0
    f16 = mutant == "f16_pad"
    for i, shape in enumerate(cc.WGRAD_H16_CASES if f16 else cc.WGRAD_CASES):
        n, k, h, w, m = shape
        if not f16 and cc.wgrad_kernel(k, m)[0] != "rowpair":
            continue
        if (mutant == "pair_lower_row" and h % 2 == 0) or (mutant == "last_slab" and cc.rowpair_splits(*shape) == 1):
            continue
        x, _, _, _, dy = _ops(shape, 100 * i, f16)
        got = cr.wgrad_mutant(x, dy, slabs=cc.rowpair_splits(*shape), mutant=mutant)
        r = cr.ratio(got, cr.conv3x3_wgrad(x, dy), cr.conv_bar("f16" if f16 else "wgrad", cr.conv3x3_wgrad(x, dy, absolute=True)))
        tried += 1
        hit.append(r >= 10.0)
    print("%s: rejected by 10x on %d of %d shapes" % (mutant, sum(hit), tried))
    assert tried >= 3 and all(hit), (mutant, sum(hit), tried)


def test_the_fp16_layout_restatement_pads_with_zeros():
    x = cc.rand((2, 16, 3, 9), 5)
    nhwc, nchwp = cc.f16_layouts_ref(x)
    assert nchwp.shape[-1] == cc.padded_row(9) == 24 and cc.padded_row(8) == 16 and cc.padded_row(1) == 16
    assert torch.equal(nchwp[..., :9], x.half()) and float(nchwp[..., 9:].abs().max()) == 0.0
    assert torch.equal(nhwc[1, 0, 2, 4], x.half()[1, :16, 2, 4])
    assert cc.f16_layouts_ref(x[:, :8])[0] is None


def test_minimal_filtering_at_a_tiny_k_is_held_to_the_scale_of_its_tile():
    """an honest fp32 F(m,3) convolution and row-pair weight gradient (cnn_ref.wino_conv_fp32 / wgrad_rowpair_fp32) over the tables: within
    the plain bar C U s wherever an output sums TINY_K products or more, within the bar of the tile (s_win) below - where they do miss
    the plain bar, so a correct kernel cannot be held to it there.  The seam mutants still miss the tile's bar by 10x at those shapes."""
    over, n_tiny = 0.0, 0
    for dgrad in (False, True):
        for i, shape in enumerate(cc.WINO_CASES):
            n, k, h, w, m = shape
            x, wt, b, wd, _ = _ops(shape, 7 * i)
            g, b = (wd.transpose(0, 1).flip(2, 3), None) if dgrad else (wt, b)
            mf, fam = (4, "f43") if m >= 64 else (2, "f23")
            got, ref, s, sw = cr.wino_conv_fp32(x, g, b, mf), cr.conv3x3(x, g, b), cr.conv3x3(x, g, b, absolute=True), cr.conv3x3_window(x, g, b, mf)
            assert bool((sw >= s * (1 - 1e-12)).all())
            r = cr.ratio(got, ref, cr.conv_bar(fam, s))
            if 9 * k >= cr.TINY_K:
                assert r <= 1.0, (shape, dgrad, r)
                continue
            over, n_tiny = max(over, r), n_tiny + 1
            assert cr.ratio(got, ref, cr.conv_bar(fam, sw)) <= 1.0, (shape, dgrad)
            for mutant in cr.SEAM_CONV_MUTANTS:
                if (mutant == "odd_last_col" and w % 2 == 0) or (mutant == "cin_mod4" and k % 4 == 0) or (mutant == "gap_slot" and n * h == 1):
                    continue
                assert cr.ratio(cr.conv_mutant(x, g, b, mutant), ref, cr.conv_bar(fam, sw)) >= 10.0, (shape, dgrad, mutant)
    assert n_tiny >= 10 and over > 1.0, (n_tiny, over)
    print("F(m,3) at K < %d: %d launches, honest fp32 up to %.2f of the plain bar" % (cr.TINY_K, n_tiny, over))
    over, n_tiny = 0.0, 0
    for i, shape in enumerate(cc.WGRAD_CASES):
        n, k, h, w, m = shape
        if cc.wgrad_kernel(k, m)[0] != "rowpair":
            continue
        x, _, _, _, dy = _ops(shape, 11 * i)
        got, ref, s, sw = cr.wgrad_rowpair_fp32(x, dy), cr.conv3x3_wgrad(x, dy), cr.conv3x3_wgrad(x, dy, absolute=True), cr.conv3x3_wgrad_window(x, dy)
        assert bool((sw >= s * (1 - 1e-12)).all())
        r = cr.ratio(got, ref, cr.conv_bar("wgrad", s))
        if n * h * w >= cr.TINY_K:
            assert r <= 1.0, (shape, r)
            continue
        over, n_tiny = max(over, r), n_tiny + 1
        assert cr.ratio(got, ref, cr.conv_bar("wgrad", sw)) <= 1.0, shape
        if h % 2:
            assert cr.ratio(cr.wgrad_mutant(x, dy, mutant="pair_lower_row"), ref, cr.conv_bar("wgrad", sw)) >= 10.0, shape
    assert n_tiny >= 3 and over > 1.0, (n_tiny, over)
    print("row-pair weight gradient below %d pixels: %d launches, honest fp32 up to %.2f of the plain bar" % (cr.TINY_K, n_tiny, over))
