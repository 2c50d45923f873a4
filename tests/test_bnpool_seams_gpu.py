"""GPU: every entry point of vistaocr_amd/csrc/bn_pool.hip at every seam of its host plan, through the C entry points, in guarded memory
(tests/bnpool_cases.py: the tables, why their rows, the data and the comparisons; tests/test_bnpool_cases_cpu.py judges them without a
GPU).  tests/test_cnn_fp64_gpu.py and tests/test_ops_gpu.py hold the same kernels at the model's shapes; here the shapes are tiny and each
call must
  - hold the unchanged bars of tests/cnn_ref.py (bn_stat_bars, running_bars, bn_apply_bar, bn_bwd_bars, conv_bias_grad_bar), ReLU decisions
    taken from the kernel's own forward and every decision that differs from fp64 a near-tie inside the forward bar;
  - keep the bit-for-bit identities include/vocr.h promises: the two-launch training forward is statistics + apply, the fused pooled
    forward is apply + pool in `out` and `idx`, the training one statistics + fused forward; the pooling forward and gradient are torch's
    CPU op and its autograd; with integer gradients all four regimes of vocr_fracpool2x2_bwd are cnn_ref.pool_scatter exactly;
  - write every element of every output (outputs start as NaN, idx as POISON), read nothing it did not write (operand bands and the
    exactly-sized workspace are NaN; idx is read between bands of 0), leave every band as it was, and give the same bits when run again.
Per-channel vectors (mean, invstd, gamma, beta, dgamma, dbeta, dconv_bias, xhat_sum, the running statistics, samples) are guarded too.
A refused call (vocr_bn_relu_fracpool2x2_bwd on a shape its _supported query refuses) must return an error and leave every output
poisoned.  Non-finite inputs: the pooling forward follows ATen (a NaN takes its window, four -inf keep the first pixel); the BatchNorm
apply, the fused forwards and ReLU + MaxPool turn a NaN into 0, which is pinned here and stated in include/vocr.h.
`-s` prints one row per case family: cases, comparisons, the worst error / bar, the wall time of the file."""
import time

import pytest
import torch
import torch.nn.functional as F

from tests import bnpool_cases as bc
from tests import cnn_ref as cr

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
_ROWS, _FAM, _T0, _EXACT, _HELD = [], [], [None], [0], [0]
_STAT_KEYS = ("mean", "invstd", "xhat_sum", "running_mean", "running_var", "num_batches_tracked")


def _row(case, what, r):
    _ROWS.append((case, what, float(r)))


def _exact(cond, msg):
    _EXACT[0] += 1
    assert cond, msg


def _family(name, cases, start, exact0):
    rows = _ROWS[start:]
    over = ["%s %s: error / bar = %.3f" % row for row in rows if not row[2] <= 1.0]
    worst = {}
    for _, what, r in rows:
        n_, w_ = worst.get(what, (0, 0.0))
        worst[what] = (n_ + 1, max(w_, r))
    _FAM.append((name, cases, len(rows), _EXACT[0] - exact0, worst))
    assert not over, "\n".join(over)
    _HELD[0] += 1


@pytest.fixture(scope="module", autouse=True)
def _table():
    _T0[0] = time.time()
    yield
    if _FAM:
        print("\n%-62s %6s %12s %12s %10s" % ("family / quantity", "cases", "bar checks", "exact checks", "worst/bar"))
        for name, cases, nbar, nexact, worst in _FAM:
            print("%-62s %6d %12d %12d %10.4f" % (name, cases, nbar, nexact, max([w for _, w in worst.values()] + [0.0])))
            for what in sorted(worst):
                print("    %-58s %6s %12d %12s %10.4f" % (what, "", worst[what][0], "", worst[what][1]))
        if _HELD[0] == len(_FAM):
            print("every case: no NaN in an output but the planted ones, no touched band, no run-to-run difference")
        else:
            print("%d of %d families held" % (_HELD[0], len(_FAM)))
        print("wall time of the file %.1f s" % (time.time() - _T0[0]))


@pytest.fixture(scope="module")
def dev():
    from vistaocr_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    from vistaocr_amd._lib import call
    call(name, *args)


def _lib():
    from vistaocr_amd import _lib as m
    return m.load()


def _vec(t, dev, name):
    return bc.Guarded(t.shape, dev, data=t, name=name)


def _out(shape, dev, name, dtype=torch.float32):
    return bc.Guarded(shape, dev, name=name, dtype=dtype)


def _ptr(g):
    return None if g is None else g.ptr


def _bits_equal(a, b):
    return torch.equal(a.bits(), b.bits())


def _twice(case, operands, run, nan_ok=()):
    """run() allocates fresh outputs / workspaces, calls the library and returns {name: buffer or None}; "ws" is the workspace (only its
    band is checked).  Runs it twice, holds both runs to their buffers and to the same bits; returns the first run's buffers."""
    a, b = run(), run()
    torch.cuda.synchronize()
    for g in operands:
        assert g.outside_untouched(), "%s: the guard band of operand %s changed" % (case, g.name)
    for bufs in (a, b):
        for name, g in bufs.items():
            if g is None:
                continue
            assert g.outside_untouched(), "%s: a store outside %s" % (case, name)
            if name != "ws" and name not in nan_ok:
                assert not g.has_unwritten(), "%s: %s holds NaN / POISON (an element not written, or a read outside an operand / of unwritten workspace)" % (case, name)
    for name, g in a.items():
        if g is not None and name != "ws":
            assert _bits_equal(g, b[name]), "%s: %s differs between two runs" % (case, name)
    _EXACT[0] += 1
    return a


# ------------------------------------------------------------------------------------------------------------ the statistics
def _stat_outputs(c, dev, rm0, rv0, null):
    o = dict(mean=_out((c,), dev, "mean"), invstd=_out((c,), dev, "invstd"))
    o["xhat_sum"] = None if "xhat_sum" in null else _out((c,), dev, "xhat_sum")
    o["running_mean"] = None if "running_mean" in null else _vec(rm0, dev, "running_mean")
    o["running_var"] = None if "running_var" in null else _vec(rv0, dev, "running_var")
    # a device int64 as two 32-bit words between bands of 0
    o["num_batches_tracked"] = None if "num_batches_tracked" in null else bc.Guarded((2,), dev, data=torch.zeros(2, dtype=torch.int32), dtype=torch.int32,
                                                                                     name="num_batches_tracked")
    return o


def _stat_ptrs(o):
    return (o["mean"].ptr, o["invstd"].ptr, _ptr(o["running_mean"]), _ptr(o["running_var"]), _ptr(o["num_batches_tracked"]), _ptr(o["xhat_sum"]))


def _same_stats(case, a, b, keys=_STAT_KEYS + ("out", "idx")):
    for k in keys:
        if k in a and k in b and a[k] is not None:
            _exact(_bits_equal(a[k], b[k]), "%s: %s differs between the fused call and the calls it stands for" % (case, k))


def _counted_once(case, o):
    if o["num_batches_tracked"] is not None:
        _exact(o["num_batches_tracked"].t.tolist() == [1, 0], "%s: num_batches_tracked %s after one call" % (case, o["num_batches_tracked"].t.tolist()))


def _ws_bytes(n, c, hw):
    nbytes = _lib().vocr_bn_workspace_bytes(n, c, hw)
    assert nbytes == bc.workspace_bytes(n, c, hw), (n, c, hw, nbytes)
    return nbytes


# ---------------------------------------------------------------------------------------------------------- dense BatchNorm
def _bn_row(dev, i, b):
    n, c, hw = b.n, b.c, b.hw
    case = repr(b)
    y, da = bc.bn_y((n, c, hw), 100 + i), bc.ints((n, c, hw), 300 + i)
    gamma, beta, rm0, rv0 = bc.bn_params(c, 200 + i)
    gy, gda = bc.buf(y.shape, dev, y, b.off["y"], "y"), bc.buf(da.shape, dev, da, b.off["da"], "da")
    gg, gb = _vec(gamma, dev, "gamma"), _vec(beta, dev, "beta")
    nbytes = _ws_bytes(n, c, hw)

    def forward(fused):
        def run():
            o = _stat_outputs(c, dev, rm0, rv0, b.null)
            o["out"], o["ws"] = bc.buf(y.shape, dev, None, b.off["out"], "out"), bc.workspace(nbytes, dev)
            if fused:
                _call("vocr_bn_train_relu_apply", gy.ptr, gg.ptr, gb.ptr, o["out"].ptr, n, c, hw, EPS, MOM, *_stat_ptrs(o), o["ws"].ptr, _st())
            else:
                _call("vocr_bn_train_stats", gy.ptr, n, c, hw, EPS, MOM, *_stat_ptrs(o), o["ws"].ptr, _st())
                _call("vocr_bn_relu_apply", gy.ptr, o["mean"].ptr, o["invstd"].ptr, gg.ptr, gb.ptr, o["out"].ptr, n, c, hw, _st())
            return o
        return run

    a = _twice(case + " statistics + apply", [gy, gg, gb], forward(False))
    f = _twice(case + " two-launch forward", [gy, gg, gb], forward(True))
    _same_stats(case, a, f)
    _counted_once(case, a)
    _counted_once(case, f)
    yd, g_d, b_d = gy.t, gg.t, gb.t
    got = {k: a[k].t for k in ("mean", "invstd", "out", "xhat_sum", "running_mean", "running_var") if a[k] is not None}
    rows, ctx = bc.bn_forward_ratios(yd, g_d, b_d, got, rm0.to(dev).double(), rv0.to(dev).double(), MOM, EPS)

    def backward():
        o = dict(dy=bc.buf(y.shape, dev, None, b.off["dy"], "dy"), dgamma=_out((c,), dev, "dgamma"), dbeta=_out((c,), dev, "dbeta"),
                 dconv_bias=None if "dconv_bias" in b.null else _out((c,), dev, "dconv_bias"), ws=bc.workspace(nbytes, dev))
        _call("vocr_bn_relu_bwd", gda.ptr, gy.ptr, a["mean"].ptr, a["invstd"].ptr, gg.ptr, gb.ptr, _ptr(a["xhat_sum"]), o["dy"].ptr, o["dgamma"].ptr,
              o["dbeta"].ptr, _ptr(o["dconv_bias"]), n, c, hw, o["ws"].ptr, _st())
        return o

    w = _twice(case + " backward", [gda, gy, gg, gb, a["mean"], a["invstd"]] + ([a["xhat_sum"]] if a["xhat_sum"] is not None else []), backward)
    rows += bc.bn_backward_ratios(gda.t, yd, g_d, ctx, {k: w[k].t for k in ("dy", "dgamma", "dbeta", "dconv_bias") if w[k] is not None})
    # integer gradients: dbeta is exact in any order
    _exact(torch.equal(w["dbeta"].t.double(), (gda.t.double() * ctx["mask"]).sum((0, 2))), "%s: dbeta of integer gradients is not exact" % case)
    if a["xhat_sum"] is None and w["dconv_bias"] is not None:
        _exact(bool((w["dconv_bias"].t == 0).all()), "%s: dconv_bias without xhat_sum must be 0" % case)
    for what, r in rows:
        _row(case, what, r)


def test_dense_batchnorm_seams(dev):
    """vocr_bn_train_stats + vocr_bn_relu_apply, vocr_bn_train_relu_apply (bit-identical) and vocr_bn_relu_bwd on every row of BN_CASES"""
    start, e0 = len(_ROWS), _EXACT[0]
    for i, b in enumerate(bc.BN_CASES):
        _bn_row(dev, i, b)
    _family("dense BatchNorm: statistics, apply, two-launch, backward", len(bc.BN_CASES), start, e0)


def test_eval_stats(dev):
    start, e0 = len(_ROWS), _EXACT[0]
    for c in bc.EVAL_CASES:
        _, _, rm0, rv0 = bc.bn_params(c, 700 + c)
        rv0[0] = 0.0
        grm, grv = _vec(rm0, dev, "running_mean"), _vec(rv0, dev, "running_var")

        def run():
            o = dict(mean=_out((c,), dev, "mean"), invstd=_out((c,), dev, "invstd"))
            _call("vocr_bn_eval_stats", grm.ptr, grv.ptr, c, EPS, o["mean"].ptr, o["invstd"].ptr, _st())
            return o

        o = _twice("eval c=%d" % c, [grm, grv], run)
        _exact(torch.equal(o["mean"].t, grm.t), "eval c=%d: mean is not running_mean" % c)
        ref = 1.0 / (grv.t.double() + EPS).sqrt()
        _row("eval c=%d" % c, "invstd", cr.ratio(o["invstd"].t, ref, 3 * cr.U * ref))
    _family("vocr_bn_eval_stats", len(bc.EVAL_CASES), start, e0)


# ---------------------------------------------------------------------------------------------------------- fractional pool
def _torch_pool(x, f, dout=None):
    xg = x.detach().cpu().clone().requires_grad_(True)
    out, idx = F.fractional_max_pool2d(xg, 2, output_size=(f.oh, f.ow), _random_samples=f.samples(), return_indices=True)
    if dout is not None:
        out.backward(dout)
    return out.detach(), idx, xg.grad


def _same_float_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


def _pool_fwd(case, f, gx, gs, dev, nan_ok=()):
    def run():
        o = dict(out=_out((f.n, f.c, f.oh, f.ow), dev, "out"), idx=_out((f.n, f.c, f.oh, f.ow), dev, "idx", torch.int32))
        _call("vocr_fracpool2x2_fwd", gx.ptr, gs.ptr, o["out"].ptr, o["idx"].ptr, f.n, f.c, f.h, f.w, f.oh, f.ow, _st())
        return o
    return _twice(case + " pool forward", [gx, gs], run, nan_ok)


def _pool_row(dev, i, f):
    from vistaocr_amd import ops
    case = repr(f)
    x, dout = bc.frac_plane_data(f, "rand", 5 + i), bc.ints((f.n, f.c, f.oh, f.ow), 7 + i)
    gx, gs = _vec(x, dev, "x"), _vec(f.samples(), dev, "samples")
    o = _pool_fwd(case, f, gx, gs, dev)
    out_t, idx_t, grad_t = _torch_pool(x, f, dout)
    _exact(_same_float_bits(o["out"].t, out_t), "%s: out differs from torch's CPU op" % case)
    _exact(torch.equal(o["idx"].t.cpu().long(), idx_t), "%s: idx differs from torch's CPU op" % case)
    gd = _vec(dout, dev, "dout")
    gi = bc.Guarded(o["idx"].t.shape, dev, data=o["idx"].t, dtype=torch.int32, name="idx", band=0)
    ref = cr.pool_scatter(dout, idx_t, f.h, f.w)
    dx0 = None
    for off in f.dx_offs:
        def run():
            d = dict(dx=bc.buf((f.n, f.c, f.h, f.w), dev, None, off, "dx"))
            _call("vocr_fracpool2x2_bwd", gd.ptr, gi.ptr, d["dx"].ptr, f.n, f.c, f.h, f.w, f.oh, f.ow, _st())
            return d
        dx = _twice("%s pool backward (%s, dx %d bytes off)" % (case, bc.pool_regime(f.h * f.w), off), [gd, gi], run)["dx"].t
        _exact(torch.equal(dx.cpu().double(), ref), "%s: dx (%d bytes off) is not pool_scatter" % (case, off))
        _exact(torch.equal(dx.cpu(), grad_t), "%s: dx differs from torch's autograd" % case)
        dx0 = dx if dx0 is None else dx0
    # the autograd function the model's un-fused path calls: its own torch.empty buffers, the same bits
    xg = x.to(dev).requires_grad_(True)
    y = ops.FracPoolFn.apply(xg, f.samples().to(dev), f.oh, f.ow)
    _exact(_same_float_bits(y.detach(), o["out"].t), "%s: ops.FracPoolFn differs from the entry point" % case)
    y.backward(dout.to(dev))
    _exact(torch.equal(xg.grad, dx0), "%s: ops.FracPoolFn's gradient differs from the entry point" % case)


def test_fracpool_forward_and_backward_are_torchs_cpu_op(dev):
    """vocr_fracpool2x2_fwd / _bwd on every row of FRAC_CASES: out and idx equal torch's CPU op, dx equals its autograd and pool_scatter
    exactly (integer gradients) in all four plane regimes with dx aligned and 4 bytes off; ops.FracPoolFn gives the same bits"""
    start, e0 = len(_ROWS), _EXACT[0]
    regimes = set()
    for i, f in enumerate(bc.FRAC_CASES):
        _pool_row(dev, i, f)
        regimes.add(bc.pool_regime(f.h * f.w))
    assert regimes == {"lds8192", "lds18432", "lds36864", "scatter"}, regimes
    _family("fractional pool forward / backward against torch (exact)", len(bc.FRAC_CASES), start, e0)


def _fused_forward(dev, case, f, y, gamma, beta, rm0, rv0, null, check):
    """the three forms of the pooled training forward on one tensor; check: each twice, the identities between them, the bars of the
    statistics and of the activation, and the pooled output against torch's op on the kernel's own activation.  Returns the buffers the
    backward needs."""
    n, c, h, w, oh, ow = f.n, f.c, f.h, f.w, f.oh, f.ow
    gy, gg, gb, gs = _vec(y, dev, "y"), _vec(gamma, dev, "gamma"), _vec(beta, dev, "beta"), _vec(f.samples(), dev, "samples")
    nbytes = _ws_bytes(n, c, h * w)
    pooled = lambda: dict(out=_out((n, c, oh, ow), dev, "out"), idx=_out((n, c, oh, ow), dev, "idx", torch.int32))

    def separate():                              # statistics, apply, pool
        o = _stat_outputs(c, dev, rm0, rv0, null)
        o.update(pooled(), act=_out((n, c, h, w), dev, "act"), ws=bc.workspace(nbytes, dev))
        _call("vocr_bn_train_stats", gy.ptr, n, c, h * w, EPS, MOM, *_stat_ptrs(o), o["ws"].ptr, _st())
        _call("vocr_bn_relu_apply", gy.ptr, o["mean"].ptr, o["invstd"].ptr, gg.ptr, gb.ptr, o["act"].ptr, n, c, h * w, _st())
        _call("vocr_fracpool2x2_fwd", o["act"].ptr, gs.ptr, o["out"].ptr, o["idx"].ptr, n, c, h, w, oh, ow, _st())
        return o

    def fused():                                 # statistics, apply + pool in one pass
        o = _stat_outputs(c, dev, rm0, rv0, null)
        o.update(pooled(), ws=bc.workspace(nbytes, dev))
        _call("vocr_bn_train_stats", gy.ptr, n, c, h * w, EPS, MOM, *_stat_ptrs(o), o["ws"].ptr, _st())
        _call("vocr_bn_relu_fracpool2x2_fwd", gy.ptr, o["mean"].ptr, o["invstd"].ptr, gg.ptr, gb.ptr, gs.ptr, o["out"].ptr, o["idx"].ptr, n, c, h, w, oh, ow, _st())
        return o

    def training():                              # partial statistics, then everything in one pass
        o = _stat_outputs(c, dev, rm0, rv0, null)
        o.update(pooled(), ws=bc.workspace(nbytes, dev))
        _call("vocr_bn_train_relu_fracpool2x2_fwd", gy.ptr, gg.ptr, gb.ptr, gs.ptr, o["out"].ptr, o["idx"].ptr, n, c, h, w, oh, ow, EPS, MOM, *_stat_ptrs(o),
              o["ws"].ptr, _st())
        return o

    ops_ = [gy, gg, gb, gs]
    if not check:
        a = separate()
        a.update(y=gy, gamma=gg, beta=gb, samples=gs)
        return a
    a = _twice(case + " statistics + apply + pool", ops_, separate)
    b = _twice(case + " statistics + fused forward", ops_, fused)
    t = _twice(case + " training fused forward", ops_, training)
    _same_stats(case, a, b)
    _same_stats(case, a, t)
    _counted_once(case, t)
    got = {k: a[k].t for k in ("mean", "invstd", "xhat_sum", "running_mean", "running_var") if a[k] is not None}
    got["out"] = a["act"].t
    rows, _ = bc.bn_forward_ratios(gy.t, gg.t, gb.t, got, rm0.to(dev).double(), rv0.to(dev).double(), MOM, EPS)
    for what, r in rows:
        _row(case, what, r)
    out_t, idx_t, _ = _torch_pool(a["act"].t, f)
    _exact(_same_float_bits(t["out"].t, out_t) and torch.equal(t["idx"].t.cpu().long(), idx_t), "%s: the pooled output is not torch's pool of the kernel's own activation" % case)
    return a


def _layer_inputs(f, i, variant):
    y = bc.frac_plane_data(f, variant, 400 + i)
    return (y,) + bc.bn_params(f.c, 500 + i)


def test_fused_forward_identities(dev):
    """vocr_bn_relu_fracpool2x2_fwd = vocr_bn_relu_apply + vocr_fracpool2x2_fwd and vocr_bn_train_relu_fracpool2x2_fwd = statistics +
    that, bit for bit in out, idx and every statistic, on every row and data variant of FRAC_CASES"""
    start, e0, cases = len(_ROWS), _EXACT[0], 0
    for i, f in enumerate(bc.FRAC_CASES):
        for variant in f.variants:
            _fused_forward(dev, "%s %s" % (f, variant), f, *_layer_inputs(f, i, variant), null=bc.NULL_SETS[i % len(bc.NULL_SETS)], check=True)
            cases += 1
    _family("fused pooled forwards: identities, statistics, activation", cases, start, e0)


def _fused_backward_row(dev, i, f, variant, errors):
    n, c, h, w, oh, ow = f.n, f.c, f.h, f.w, f.oh, f.ow
    case = "%s %s" % (f, variant)
    y, gamma, beta, rm0, rv0 = _layer_inputs(f, i, variant)
    null = bc.NULL_SETS[(i + 3) % len(bc.NULL_SETS)]
    a = _fused_forward(dev, case, f, y, gamma, beta, rm0, rv0, null, check=False)
    gy, gg, gb, gs = a["y"], a["gamma"], a["beta"], a["samples"]
    dout = bc.ints((n, c, oh, ow), 600 + i)
    gd = _vec(dout, dev, "dout")
    gi = bc.Guarded((n, c, oh, ow), dev, data=a["idx"].t, dtype=torch.int32, name="idx", band=0)
    nbytes = _ws_bytes(n, c, h * w)
    answer = _lib().vocr_bn_relu_fracpool2x2_bwd_supported(h, w, oh, ow)
    _exact(bool(answer) == f.supported, "%s: the library answers %d, the table's restatement %s" % (case, answer, f.supported))
    operands = [gd, gi, gs, gy, gg, gb, a["mean"], a["invstd"]] + ([a["xhat_sum"]] if a["xhat_sum"] is not None else [])

    def outputs():
        return dict(dy=_out((n, c, h, w), dev, "dy"), dgamma=_out((c,), dev, "dgamma"), dbeta=_out((c,), dev, "dbeta"),
                    dconv_bias=None if "dconv_bias" in null else _out((c,), dev, "dconv_bias"), ws=bc.workspace(nbytes, dev))

    def fused():
        o = outputs()
        _call("vocr_bn_relu_fracpool2x2_bwd", gd.ptr, gi.ptr, gs.ptr, gy.ptr, a["mean"].ptr, a["invstd"].ptr, gg.ptr, gb.ptr, _ptr(a["xhat_sum"]), o["dy"].ptr,
              o["dgamma"].ptr, o["dbeta"].ptr, _ptr(o["dconv_bias"]), n, c, h, w, oh, ow, o["ws"].ptr, _st())
        return o

    if not f.supported:                          # refused: an error, nothing launched, every output still poisoned
        o = outputs()
        with pytest.raises(RuntimeError):
            _call("vocr_bn_relu_fracpool2x2_bwd", gd.ptr, gi.ptr, gs.ptr, gy.ptr, a["mean"].ptr, a["invstd"].ptr, gg.ptr, gb.ptr, _ptr(a["xhat_sum"]), o["dy"].ptr,
                  o["dgamma"].ptr, o["dbeta"].ptr, _ptr(o["dconv_bias"]), n, c, h, w, oh, ow, o["ws"].ptr, _st())
        torch.cuda.synchronize()
        for name, g in o.items():
            if g is not None:
                _exact(g.all_unwritten() and g.outside_untouched(), "%s: a refused call touched %s" % (case, name))
        return
    try:
        k = _twice(case + " fused backward", operands, fused)
    except RuntimeError as e:                    # an accepted shape refused at launch: a finding, reported with the others
        errors.append("%s: %s" % (case, e))
        return

    def two_pass():
        o = outputs()
        o["da"] = _out((n, c, h, w), dev, "da")
        _call("vocr_fracpool2x2_bwd", gd.ptr, gi.ptr, o["da"].ptr, n, c, h, w, oh, ow, _st())
        _call("vocr_bn_relu_bwd", o["da"].ptr, gy.ptr, a["mean"].ptr, a["invstd"].ptr, gg.ptr, gb.ptr, _ptr(a["xhat_sum"]), o["dy"].ptr, o["dgamma"].ptr,
              o["dbeta"].ptr, _ptr(o["dconv_bias"]), n, c, h * w, o["ws"].ptr, _st())
        return o

    t = _twice(case + " two-pass backward", operands, two_pass)
    # the references: the gradient of the kernel's own winners, ReLU decisions of the kernel's own activation
    got = dict(mean=a["mean"].t, invstd=a["invstd"].t, out=a["act"].t)
    rows, ctx = bc.bn_forward_ratios(gy.t, gg.t, gb.t, got, eps=EPS)
    da = cr.pool_scatter(gd.t, a["idx"].t, h, w)
    _exact(torch.equal(t["da"].t.double(), da), "%s: vocr_fracpool2x2_bwd is not pool_scatter" % case)
    for form, o in (("fused", k), ("two-pass", t)):
        for what, r in bc.bn_backward_ratios(da, gy.t, gg.t, ctx, {q: o[q].t for q in ("dy", "dgamma", "dbeta", "dconv_bias") if o[q] is not None}):
            _row(case, "%s %s" % (form, what), r)
        _exact(torch.equal(o["dbeta"].t.double(), (da * ctx["mask"]).sum((0, 2, 3))), "%s: %s dbeta of integer gradients is not exact" % (case, form))
        if a["xhat_sum"] is None and o["dconv_bias"] is not None:
            _exact(bool((o["dconv_bias"].t == 0).all()), "%s: dconv_bias without xhat_sum must be 0" % case)
    if variant == "planted":
        return int((cr.pool_scatter(torch.ones_like(gd.t), a["idx"].t, h, w) == 4).sum())


def test_fused_backward_seams(dev):
    """vocr_bn_relu_fracpool2x2_bwd on every backward row and data variant: the support query against the table, accepted shapes against
    cnn_ref.bn_relu_bwd of pool_scatter and against the two-pass form under the same bars, refused shapes left untouched"""
    start, e0, cases, four, errors = len(_ROWS), _EXACT[0], 0, 0, []
    for i, f in enumerate(bc.FRAC_CASES):
        if not f.backward:
            continue
        for variant in (f.variants if f.supported else ("rand",)):
            four += _fused_backward_row(dev, i, f, variant, errors) or 0
            cases += 1
    assert not errors, "\n".join(errors)
    assert four > 0, "no pixel won four windows on the device"
    _family("fused pooled backward (accepted: bars; refused: untouched)", cases, start, e0)


# ------------------------------------------------------------------------------------------------------- non-finite inputs
def test_nonfinite_inputs_are_pinned(dev):
    start, e0 = len(_ROWS), _EXACT[0]
    f = bc.NONFINITE_CASE
    n, c, h, w, oh, ow = f.n, f.c, f.h, f.w, f.oh, f.ow
    x = bc.nonfinite_plane(f)
    gx, gs = _vec(x, dev, "x"), _vec(f.samples(), dev, "samples")
    # the pooling forward: ATen's rule - the NaN takes its windows (the last NaN of two), four -inf keep the first pixel
    o = _pool_fwd("non-finite", f, gx, gs, dev, nan_ok=("out",))
    out_t, idx_t, _ = _torch_pool(x, f)
    _exact(_same_float_bits(o["out"].t, out_t) and torch.equal(o["idx"].t.cpu().long(), idx_t), "non-finite: vocr_fracpool2x2_fwd differs from torch")
    _exact(bool(torch.isnan(o["out"].t).any()) and bool(torch.isinf(o["out"].t).any()), "non-finite: the planted values did not reach the output")
    # the BatchNorm apply with the identity statistics: a NaN and -inf become 0 (v > 0 ? v : 0); torch's relu would keep the NaN
    one, zero = torch.ones(c), torch.zeros(c)
    gm, gis, gg, gb = _vec(zero, dev, "mean"), _vec(one, dev, "invstd"), _vec(one, dev, "gamma"), _vec(zero, dev, "beta")

    def apply_pool():
        q = dict(act=_out((n, c, h, w), dev, "act"), out=_out((n, c, oh, ow), dev, "out"), idx=_out((n, c, oh, ow), dev, "idx", torch.int32))
        _call("vocr_bn_relu_apply", gx.ptr, gm.ptr, gis.ptr, gg.ptr, gb.ptr, q["act"].ptr, n, c, h * w, _st())
        _call("vocr_fracpool2x2_fwd", q["act"].ptr, gs.ptr, q["out"].ptr, q["idx"].ptr, n, c, h, w, oh, ow, _st())
        return q

    def fused():
        q = dict(out=_out((n, c, oh, ow), dev, "out"), idx=_out((n, c, oh, ow), dev, "idx", torch.int32))
        _call("vocr_bn_relu_fracpool2x2_fwd", gx.ptr, gm.ptr, gis.ptr, gg.ptr, gb.ptr, gs.ptr, q["out"].ptr, q["idx"].ptr, n, c, h, w, oh, ow, _st())
        return q

    a = _twice("non-finite apply + pool", [gx, gm, gis, gg, gb, gs], apply_pool)
    b = _twice("non-finite fused forward", [gx, gm, gis, gg, gb, gs], fused)
    pinned = torch.relu(torch.nan_to_num(x, nan=0.0, neginf=0.0))
    _exact(torch.equal(a["act"].t.cpu(), pinned), "non-finite: vocr_bn_relu_apply must turn NaN and -inf into 0 and leave the rest relu(y)")
    _same_stats("non-finite", a, b, keys=("out", "idx"))
    pin_out, pin_idx, _ = _torch_pool(pinned, f)
    _exact(torch.equal(b["out"].t.cpu(), pin_out) and torch.equal(b["idx"].t.cpu().long(), pin_idx), "non-finite: the fused forward is not the pool of the pinned activation")
    # the training forward: a NaN (or -inf) in y makes its channel's statistics NaN, every activation of the channel 0, the first pixel wins
    gamma, beta, rm0, rv0 = bc.bn_params(c, 3)
    gg2, gb2 = _vec(gamma, dev, "gamma"), _vec(beta, dev, "beta")
    nbytes = _ws_bytes(n, c, h * w)

    def training():
        q = _stat_outputs(c, dev, rm0, rv0, ())
        q.update(out=_out((n, c, oh, ow), dev, "out"), idx=_out((n, c, oh, ow), dev, "idx", torch.int32), ws=bc.workspace(nbytes, dev))
        _call("vocr_bn_train_relu_fracpool2x2_fwd", gx.ptr, gg2.ptr, gb2.ptr, gs.ptr, q["out"].ptr, q["idx"].ptr, n, c, h, w, oh, ow, EPS, MOM, *_stat_ptrs(q),
              q["ws"].ptr, _st())
        return q

    t = _twice("non-finite training forward", [gx, gg2, gb2, gs], training, nan_ok=("mean", "invstd", "xhat_sum", "running_mean", "running_var"))
    zero_out, zero_idx, _ = _torch_pool(torch.zeros(n, c, h, w), f)
    _exact(bool(torch.isnan(t["mean"].t[1])) and not bool(torch.isfinite(t["mean"].t[0])), "non-finite: the statistics of a channel with a NaN / -inf must not be finite")
    _exact(torch.equal(t["out"].t.cpu(), zero_out) and torch.equal(t["idx"].t.cpu().long(), zero_idx), "non-finite: the training forward must give 0 and first-pixel winners")
    # ReLU + MaxPool: fmaxf(NaN, 0) = 0
    xm = bc.bn_y((1, 2, 5, 6), 21)
    xm[0, 0, 1, 1], xm[0, 1, 2, 2:4] = float("nan"), float("-inf")
    gxm = _vec(xm, dev, "x")

    def maxpool():
        q = dict(out=_out((1, 2, 2, 3), dev, "out"), idx=_out((1, 2, 2, 3), dev, "idx", torch.int32))
        _call("vocr_relu_maxpool2_fwd", gxm.ptr, q["out"].ptr, q["idx"].ptr, 1, 2, 5, 6, _st())
        return q

    m = _twice("non-finite relu + maxpool", [gxm], maxpool)
    ref, ridx = cr.relu_maxpool2(torch.nan_to_num(xm, nan=0.0, neginf=0.0))
    _exact(torch.equal(m["out"].t.cpu(), ref) and torch.equal(m["idx"].t.cpu().long(), ridx.long()), "non-finite: vocr_relu_maxpool2_fwd must treat a NaN as 0")
    _family("non-finite inputs (pinned, see include/vocr.h)", 5, start, e0)


# ---------------------------------------------------------------------------------------------------------- ReLU + MaxPool
def test_relu_maxpool_seams(dev):
    """vocr_relu_maxpool2_fwd / _bwd on MAXPOOL_CASES: out and idx equal cnn_ref.relu_maxpool2, dx equals the scatter of dout (out > 0)
    into a plane that starts zero-filled between sentinel bands; the dropped odd row and column stay zero"""
    start, e0 = len(_ROWS), _EXACT[0]
    for i, (n, c, h, w) in enumerate(bc.MAXPOOL_CASES):
        case = "relu + maxpool %dx%dx%dx%d" % (n, c, h, w)
        oh, ow = h // 2, w // 2
        x, dout = bc.bn_y((n, c, h, w), 800 + i), bc.ints((n, c, oh, ow), 900 + i)
        gx, gd = _vec(x, dev, "x"), _vec(dout, dev, "dout")

        def forward():
            q = dict(out=_out((n, c, oh, ow), dev, "out"), idx=_out((n, c, oh, ow), dev, "idx", torch.int32))
            _call("vocr_relu_maxpool2_fwd", gx.ptr, q["out"].ptr, q["idx"].ptr, n, c, h, w, _st())
            return q

        o = _twice(case, [gx], forward)
        ref, ridx = cr.relu_maxpool2(x)
        _exact(_same_float_bits(o["out"].t, ref) and torch.equal(o["idx"].t.cpu().long(), ridx.long()), "%s: forward differs from cnn_ref.relu_maxpool2" % case)
        gi = bc.Guarded((n, c, oh, ow), dev, data=o["idx"].t, dtype=torch.int32, name="idx", band=0)

        def backward():
            q = dict(dx=_out((n, c, h, w), dev, "dx"))
            q["dx"].t.zero_()                    # the contract: dx arrives zero-filled (between sentinel bands here)
            _call("vocr_relu_maxpool2_bwd", gd.ptr, o["out"].ptr, gi.ptr, q["dx"].ptr, n, c, h, w, _st())
            return q

        dx = _twice(case + " backward", [gd, gi, o["out"]], backward)["dx"].t.cpu()
        _exact(torch.equal(dx.double(), cr.pool_scatter(dout * (ref > 0), ridx, h, w)), "%s: dx is not the scatter of dout (out > 0)" % case)
        _exact(float(dx[:, :, 2 * oh:, :].abs().sum()) == 0.0 and float(dx[:, :, :, 2 * ow:].abs().sum()) == 0.0, "%s: the dropped row / column must stay zero" % case)
    _family("ReLU + MaxPool(2,2) forward / backward (exact)", len(bc.MAXPOOL_CASES), start, e0)
