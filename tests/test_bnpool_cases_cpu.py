"""CPU: the tables of tests/bnpool_cases.py and the references they are run against, judged without a GPU.
  - each table as a set reaches every branch its module names (one assertion per category, named in its message);
  - cnn_ref.fracpool2x2 and pool_scatter equal torch's CPU fractional_max_pool2d and its autograd bit for bit at every forward row, a NaN
    and a window of four -inf included;
  - a numpy restatement of the fused backward's algorithm equals pool_scatter on every accepted backward row, and six deliberate breaks of
    it each fail at least one row on integer data, where no tolerance can absorb the break;
  - an honest fp32 BatchNorm (double sums, fp32 everything else) stays under the unchanged bars of cnn_ref.py at every row: the table is
    fair to a correct kernel."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bnpool_cases as bc
from tests import cnn_ref as cr


@pytest.fixture(autouse=True)
def _cpu_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 8))
    yield
    torch.set_num_threads(n)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ the tables
def test_the_batchnorm_table_reaches_every_category():
    rows = bc.BN_CASES
    plain = [b for b in rows if not any(b.off.values())]
    assert {b.hw % 4 for b in plain} == {0, 1, 2, 3}, "hw % 4 in 0 .. 3 with aligned bases"
    assert {(b.hw % 4, b.v_bwd) for b in plain if b.hw < 32} >= {(0, 4), (1, 1), (2, 2), (3, 1)}, "the vector width hw alone allows"
    for t in ("y", "out", "da", "dy"):
        for o in (4, 8):
            alone = [b for b in rows if b.off[t] == o and sum(1 for v in b.off.values() if v) == 1 and b.hw % 4 == 0]
            assert alone, "%s alone %d bytes off" % (t, o)
            for b in alone:                      # vec_width takes the minimum over the bases of the pass, and only of that pass
                v = 1 if o == 4 else 2
                assert b.v_stats == (v if t == "y" else 4), (b, "statistics pass")
                assert b.v_apply == (v if t in ("y", "out") else 4), (b, "apply pass")
                assert b.v_bwd == (v if t in ("y", "da", "dy") else 4), (b, "backward")
    assert {b.hw for b in rows if b.n == 300} >= {1, 2, 3, 4, 5}, "planes shorter than one 256 V step (ChanWalk's while), n = 300"
    assert {b.v_bwd for b in rows if b.n == 300} == {1, 2, 4}, "... at every vector width"
    for v in (1, 2, 4):
        per_channel = {b.count // v for b in rows if b.v_stats == b.v_bwd == v}     # (4 x 1024 vectors of 4 are one chunk: one past it, two)
        for edge in (256, 768, 1024, 4096):      # the partial pass's four slots: 3, 1, 0 dead slots on the edge, 2 / 0 / 3 just past it
            assert {edge - 1, edge, edge + 1} <= per_channel, "n hw / V on and either side of %d at V = %d" % (edge, v)
        per_plane = {b.hw // v for b in rows if b.v_apply == b.v_bwd == v}
        for gx in (1, 2):
            for k in (1, 2, 3, 4):
                e = gx * 256 * k
                assert {e - 1, e, e + 1} <= per_plane, "hw / V on and either side of %d x 256 x %d at V = %d" % (gx, k, v)
        assert {bc.plane_gx(x) for x in per_plane} >= {1, 2, 3}
    counts = {b.count: b for b in rows}
    assert {bc.CHUNK - 4, bc.CHUNK, bc.CHUNK + 4, 2 * bc.CHUNK + 1} <= set(counts), "16384 - 4, 16384, 16384 + 4, 2 x 16384 + 1 per channel"
    assert [counts[k].nchunk for k in (bc.CHUNK - 4, bc.CHUNK, bc.CHUNK + 4, 2 * bc.CHUNK + 1)] == [1, 1, 2, 3]
    assert counts[bc.CHUNK + 4].seam_inside_a_plane() and counts[2 * bc.CHUNK + 1].seam_inside_a_plane(), "a chunk seam inside a plane"
    b = counts[2 * bc.CHUNK + 1]                 # chunks are balanced: the last one is 3 short of the others, never a single vector
    assert (b.per, b.count - 2 * b.per) == (10924, 10921) and b.v_stats == 1
    assert any(b.v_apply == 1 and b.hw > 65536 and b.hw > 4 * 64 * 256 and b.n == b.c == 1 for b in rows), "a fifth trip under the 64-workgroup cap"
    assert {1, 65} <= {b.c for b in rows} and any(b.n * b.c == 1 for b in rows), "c = 1, c = 65, n c = 1"
    for name in bc.OPTIONAL:
        assert any(name in b.null for b in rows) and sum(1 for b in rows if name not in b.null) > len(rows) // 2, "%s NULL in a case, present in the others" % name
    assert max(b.n * b.c * b.hw for b in rows) <= bc.MAX_PLANE
    assert set(bc.EVAL_CASES) >= {1, 64, 65}


def _frac_ok():
    return [f for f in bc.FRAC_CASES if f.backward and f.supported]


def test_the_fractional_pool_table_reaches_every_category():
    rows = bc.FRAC_CASES
    assert min(f.h for f in rows) == 2 and min(f.w for f in rows) == 2, "the forwards from h = 2 and w = 2"
    assert {1, 2} <= {f.oh for f in rows} and {1, 2} <= {f.ow for f in rows}, "out of 1 (alpha 0) and 2 on both axes"
    assert any(f.oh == f.h - 1 for f in rows) and any(f.ow == f.w - 1 for f in rows), "out = in - 1 (alpha exactly 1)"
    assert sum(1 for f in rows if (f.oh, f.ow) == bc.ratio_out(f.h, f.w)) >= 10, "the 0.5 / 0.7 ratios"
    ok, refused = _frac_ok(), [f for f in rows if f.backward and not f.supported]
    assert min(f.h for f in ok) == 4 and {4, 8, 12, 16, 20, 36, 260} <= {f.w for f in ok}, "the fused backward from h = 4, w in 4 .. 260"
    for w in (8, 12, 16, 36, 260, 204):          # the largest out accepted and the smallest refused, as the library's rule restated says
        top = max(o for o in range(2, w) if bc.fused_bwd_supported(6, w, 2, o))
        assert any(f.w == w and f.ow == top for f in ok), "the largest ow accepted at w = %d" % w
        assert any(f.w == w and f.ow == top + 1 for f in refused), "the smallest ow refused at w = %d" % w
    assert bc.fused_bwd_supported(6, 204, 3, 201) and not bc.fused_bwd_supported(6, 204, 3, 202), "alpha exactly 1.01f is accepted"
    assert any(f.oh == max(o for o in range(2, f.h) if bc.fused_bwd_supported(f.h, f.w, o, f.ow)) and f.h >= 6 for f in ok), "the largest oh accepted"
    assert any(f.backward and not bc.fused_bwd_supported(f.h, f.w, f.oh, 2) and f.w % 4 == 0 for f in refused), "the smallest oh refused"
    assert any((f.h, f.w) == (4, 8184) for f in ok) and (2 * 8184 + 8 + 2 * 4) * 4 == 65536, "the LDS bound met with equality is accepted"
    assert any((f.h, f.w) == (4, 8188) for f in refused), "the first width past the LDS bound is refused"
    assert any(f.w % 4 and f.backward for f in refused), "w % 4 != 0 is refused"
    for axis in (0, 1):
        assert {s[axis] for f in rows for s in f.sample_pairs()} == set(bc.SAMPLES), "every sample on axis %d" % axis
    assert len({s for f in rows for s in f.sample_pairs()}) >= 40, "u_w and u_h chosen independently"
    ops_ = {f.op for f in rows}
    assert {255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049} <= ops_, "pooled outputs per plane around 256 / 512 / 1024 / 2048"
    assert {255, 256, 1023, 1024, 1025, 2047, 2048, 2049} <= {f.op for f in ok}
    assert any(f.n * f.op < bc.nchunk(f.n * f.h * f.w) for f in ok), "n oh ow below the chunk count"
    planes = {f.h * f.w: f for f in rows if f.dx_offs == (0, 4)}
    assert set(bc.PLANE_SIZES) <= set(planes), "input planes on and past 8192 / 18432 / 36864 floats, dx aligned and 4 bytes off"
    for regime in ("lds8192", "lds18432", "lds36864", "scatter"):
        assert {p % 4 == 0 for p in bc.PLANE_SIZES if bc.pool_regime(p) == regime} == {True, False}, "in_plane % 4 zero and non-zero in " + regime
    assert all(1 <= f.planes <= 3 for f in rows)
    large = [f for f in rows if f.h * f.w > bc.LARGE] + [b for b in bc.BN_CASES if b.hw > bc.LARGE]
    assert len(large) <= 30 and max(f.h * f.w for f in rows) <= bc.MAX_PLANE, "few large planes, none above 300 000 floats"


def test_window_starts_increase_and_the_last_windows_never_coincide():
    seen = set()
    for f in _frac_ok():
        for p in range(f.planes):
            for s in f.starts(p):
                assert bool((np.diff(s) >= 1).all()), "%s: window starts must strictly increase where the fused backward is accepted" % f
        assert not any(kind == "coinciding" for _, kind in f.layouts()), f
        seen |= f.layouts()
    assert seen == {(a, k) for a in "wh" for k in ("overlapping", "abutting", "apart")}, "all three layouts of the pinned last window on both axes: %s" % sorted(seen)


def test_the_largest_sample_below_one_overlaps_at_the_models_shapes():
    """what tests/test_ops_gpu.py::test_conv_bn_relu_pool_fused_backward's docstring says of 1 - 2^-24: the last two windows overlap by one
    column (start in - 3 beside the pinned in - 2); they do not coincide"""
    u = np.float32(1.0) - np.float32(2.0 ** -24)
    for size, out in ((600, 420), (420, 294), (200, 140), (30, 15), (1178, 824)):
        s = cr.fracpool_starts(u, size, out)
        assert s[-1] - s[-2] == 1, (size, out, s[-3:])
    assert cr.fracpool_starts(u, 15, 7)[-1] - cr.fracpool_starts(u, 15, 7)[-2] == 2          # 15 -> 7 rows (alpha 13 / 6): they abut
    assert list(cr.fracpool_starts(u, 200, 140)[-3:]) == [195, 197, 198]


def test_the_maxpool_table_reaches_every_category():
    rows = bc.MAXPOOL_CASES
    assert bc.covers2(rows[:len(bc.cover2(bc.MAXPOOL_AXES))], bc.MAXPOOL_AXES), "h, w in {2, 3, 4, 5, 33}: each value with two of every other axis"
    assert {(h // 2) * (w // 2) for _, _, h, w in rows} >= {255, 256, 257, 1023, 1024, 1025}, "output counts around 256 and 1024"
    assert any(h % 2 and w % 2 for _, _, h, w in rows) and any(h % 2 and not w % 2 for _, _, h, w in rows), "odd sizes drop a row / column"


# ------------------------------------------------------------------------------------------ the pooling references against torch
def _torch_pool(x, f):
    xg = x.clone().requires_grad_(True)
    out, idx = F.fractional_max_pool2d(xg, 2, output_size=(f.oh, f.ow), _random_samples=f.samples(), return_indices=True)
    return xg, out, idx


@pytest.mark.parametrize("f", bc.FRAC_CASES + [bc.NONFINITE_CASE], ids=repr)
def test_the_pool_references_are_torchs_cpu_op_bit_for_bit(f):
    variants = ("rand", "const", "nonfinite") if f is bc.NONFINITE_CASE else f.variants
    for variant in variants:
        if variant == "nonfinite":
            x = bc.nonfinite_plane(f)
        else:
            x = bc.frac_plane_data(f, variant, 5)
        xg, out, idx = _torch_pool(x, f)
        ref, ridx = cr.fracpool2x2(x, f.samples(), f.oh, f.ow)
        assert _same_bits(out.detach(), ref), (f, variant)
        assert torch.equal(idx, ridx), (f, variant)
        if variant != "nonfinite":
            dout = bc.ints(out.shape, 7)
            out.backward(dout)
            assert torch.equal(xg.grad.double(), cr.pool_scatter(dout, ridx, f.h, f.w)), (f, variant)


def test_the_nonfinite_plane_holds_what_it_says():
    f = bc.NONFINITE_CASE
    out, idx = cr.fracpool2x2(bc.nonfinite_plane(f), f.samples(), f.oh, f.ow)
    assert bool(torch.isnan(out[0, 1]).any()) and float(out[0, 0, 0, 0]) == float("-inf")
    sw, sh = f.starts(0)
    assert int(idx[0, 0, 0, 0]) == sh[0] * f.w + sw[0]                       # four -inf: the first pixel
    sw, sh = f.starts(1)
    assert int(idx[0, 1, 1, 1]) == (sh[1] + 1) * f.w + sw[1] + 1             # two NaNs in a window: the last one


# --------------------------------------------------------------------------------------------- the fused backward's algorithm
@functools.lru_cache(maxsize=None)
def _int_case(i, variant):
    """integer planes of row i of the accepted backward rows: (y, idx, dout, da = pool_scatter) with mean 0, invstd 1, gamma 1, beta 0"""
    f = _frac_ok()[i]
    y = bc.frac_plane_data(f, variant, 11 + i, integer=True)
    _, idx = cr.fracpool2x2(torch.relu(y), f.samples(), f.oh, f.ow)
    dout = bc.ints((f.n, f.c, f.oh, f.ow), 13 + i)
    dout[dout == 0] = 1.0                                                    # no break hides behind a zero gradient
    return y, idx, dout, cr.pool_scatter(dout, idx, f.h, f.w)


def _variants(f):
    return f.variants if len(f.variants) > 1 else ("rand", "const")


def _restated(i, variant, mutant=None, stats=None):
    f = _frac_ok()[i]
    y, idx, dout, _ = _int_case(i, variant)
    da = np.zeros((f.n, f.c, f.h, f.w))
    for p in range(f.planes):
        sw, sh = f.starts(p)
        da[p // f.c, p % f.c] = bc.fused_bwd_gather(dout[p // f.c, p % f.c].numpy(), idx[p // f.c, p % f.c].numpy(), sw, sh, f.h, f.w, mutant, stats)
    return torch.from_numpy(da)


def test_the_restated_fused_backward_is_pool_scatter_on_every_backward_row():
    stats, four = {}, 0
    for i, f in enumerate(_frac_ok()):
        for variant in _variants(f):
            y, idx, dout, da = _int_case(i, variant)
            assert torch.equal(_restated(i, variant, stats=stats), da), (f, variant)
            s1, s2 = bc.pooled_partial_sums(dout, idx, torch.relu(y), y, f.h, f.w)
            dz = da * (y > 0)
            assert torch.equal(s1, dz.sum((0, 2, 3))) and torch.equal(s2, (dz * y).sum((0, 2, 3))), (f, variant)
            cnt = cr.pool_scatter(torch.ones_like(dout), idx, f.h, f.w)
            four += int((cnt == 4).sum())
            if variant == "ramp":                # every winner of the pinned windows lies in the last row / column
                assert bool((idx[:, :, -1, :] // f.w == f.h - 1).all()) and bool((idx[:, :, :, -1] % f.w == f.w - 1).all()), f
            if variant == "const":
                sw, sh = f.starts(0)
                assert int(idx[0, 0, 0, 0]) == sh[0] * f.w + sw[0]
    assert four > 0, "a pixel that takes four windows' gradients"
    assert stats["fifth"] > 0, "a pixel group whose fifth candidate (start == w0 + 3) is the winner's window"
    assert stats["skipped"] > 0, "a window row that the wave-uniform skip skips"
    apart = 0                                    # pixels no window covers: they receive the BatchNorm term alone
    for i, f in enumerate(_frac_ok()):
        if any(k == "apart" for _, k in f.layouts()):
            cover = torch.zeros(f.h, f.w)
            sw, sh = f.starts(0)
            for a in sh:
                for b in sw:
                    cover[a:a + 2, b:b + 2] = 1
            apart += int((cover == 0).sum())
    assert apart > 0, "pixels that no window covers"


@pytest.mark.parametrize("mutant", bc.FUSED_MUTANTS)
def test_every_break_of_the_fused_backward_fails_a_row_on_integers(mutant):
    failed = []
    for i, f in enumerate(_frac_ok()):
        for variant in _variants(f):
            y, idx, dout, da = _int_case(i, variant)
            if mutant == "no_last_chunk":
                s1, _ = bc.pooled_partial_sums(dout, idx, torch.relu(y), y, f.h, f.w, mutant)
                bad = not torch.equal(s1, (da * (y > 0)).sum((0, 2, 3)))
            else:
                bad = not torch.equal(_restated(i, variant, mutant), da)
            if bad:
                failed.append((f.name, variant))
    print("\n%s fails %d row x variant pairs, the first: %s" % (mutant, len(failed), failed[:3]))
    assert failed, mutant


# --------------------------------------------------------------------------------------------- an honest fp32 under the bars
def _assert_under(rows, case):
    over = ["%s %s: error / bar = %.3f" % (case, what, r) for what, r in rows if not r <= 1.0]
    assert not over, "\n".join(over)


def test_an_honest_fp32_batchnorm_holds_the_bars_on_every_dense_row():
    worst = 0.0
    for i, b in enumerate(bc.BN_CASES):
        y = bc.bn_y((b.n, b.c, b.hw), 100 + i)
        gamma, beta, rm0, rv0 = bc.bn_params(b.c, 200 + i)
        da = bc.ints((b.n, b.c, b.hw), 300 + i)
        m32, is32, out = bc.honest_bn_forward(y, gamma, beta)
        cnt = b.count
        yd = y.double().transpose(0, 1).reshape(b.c, -1)
        var = ((yd * yd).sum(1) / cnt - (yd.sum(1) / cnt) ** 2).clamp_min(0)
        got = dict(mean=m32, invstd=is32, out=out, running_mean=0.9 * rm0 + 0.1 * m32,
                   running_var=0.9 * rv0 + 0.1 * (var * cnt / max(cnt - 1, 1)).float(),
                   xhat_sum=((yd.sum(1) - cnt * m32.double()) * is32.double()).float())
        rows, ctx = bc.bn_forward_ratios(y, gamma, beta, got, rm0.double(), rv0.double())
        dy, dg, db = bc.honest_bn_backward(da, y, ctx["mask"], m32, is32, gamma)
        dcb = (-gamma.double() * is32.double() * (dg.double() / cnt) * got["xhat_sum"].double()).float()
        rows += bc.bn_backward_ratios(da, y, gamma, ctx, dict(dy=dy, dgamma=dg, dbeta=db, dconv_bias=dcb))
        _assert_under(rows, b)
        worst = max(worst, max(r for _, r in rows))
    print("\nhonest fp32 BatchNorm over %d rows: worst error / bar %.3f" % (len(bc.BN_CASES), worst))


def test_an_honest_fp32_fused_layer_holds_the_bars_on_every_backward_row():
    worst = 0.0
    for i, f in enumerate(_frac_ok()):
        for variant in f.variants:
            y = bc.frac_plane_data(f, variant, 400 + i)
            gamma, beta, _, _ = bc.bn_params(f.c, 500 + i)
            m32, is32, act = bc.honest_bn_forward(y, gamma, beta)
            rows, ctx = bc.bn_forward_ratios(y, gamma, beta, dict(mean=m32, invstd=is32, out=act))
            _, idx = cr.fracpool2x2(act, f.samples(), f.oh, f.ow)
            dout = bc.ints((f.n, f.c, f.oh, f.ow), 600 + i)
            da = cr.pool_scatter(dout, idx, f.h, f.w).float()
            dy, dg, db = bc.honest_bn_backward(da, y, ctx["mask"], m32, is32, gamma)
            rows += bc.bn_backward_ratios(da, y, gamma, ctx, dict(dy=dy, dgamma=dg, dbeta=db))
            _assert_under(rows, "%s %s" % (f, variant))
            worst = max(worst, max(r for _, r in rows))
    print("\nhonest fp32 fused layer over %d rows: worst error / bar %.3f" % (len(_frac_ok()), worst))
