"""GPU: the kernels between the big ones of a training step - vocr_clamp_adam, vocr_clamp, vocr_bchw_to_wbch / vocr_wbch_to_bchw and the
dropout draw (vocr_dropout_fwd, vocr_dropout_mask) - on the C entry with raw pointers, in guarded memory (tests/guarded.py, tests/gemm_ref.py:
what a kernel reads sits between NaN bands, what it writes starts as NaN between sentinel bands that must survive bit for bit).

  vocr_clamp_adam   ONE step at a time against the float64 restatement of tests/step_glue_ref.py, from the kernel's own fp32 state, under
                    per-element bars made of the operands' magnitudes (2 .. 8 roundings): every count around a block and around the capped
                    grid up to a third trip of the grid-stride loop, every step / weight decay / gradient scale of the case lists, all
                    pointers one float off; run twice = same bits; idle elements keep p; the NaN policy with every OTHER element inside
                    the bars; +-inf; the health words; count 0; a refused clamp.  FlatClampAdam.step on the same bars, resumed at 99 990.
  vocr_clamp        bit-exact against torch.clamp on +-0, +-clamp and its neighbours, +-inf, denormals; 16-byte loop + tail and the scalar
                    path (1, 2, 3 floats off); clamp 5 and +inf; health[1] raised iff the data holds a NaN.
  the permutes      bit-exact against permute().contiguous() at every seam of the 32 x 64 tile, both directions, the output one float off
                    too, the round trip, ops.transpose2d, PermuteBchwToWbchFn.
  the dropout draw  both kernels equal the numpy restatement of the stream bit for bit, out == x * mask bit for bit.
Each test prints one row per case family (run with -s); profiles/step_glue_errors.txt keeps the rows measured on the MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from tests import step_glue_ref as sg
from tests.gemm_ref import Padded
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu

HYPER = (sg.LR, sg.BETA1, sg.BETA2, sg.EPS)


@pytest.fixture(scope="module")
def dev():
    from vistaocr_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _ptr(t):
    return ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf(object):
    """`count` floats `off` floats behind a 16-byte boundary: a Guarded (off = 0) or a one-row Padded.  data None / written=True: sentinel
    bands (a quiet NaN with a payload: a read of a band reaches the result as NaN, a store into one changes its bits); the body starts as
    NaN, or as `data` for a tensor updated in place.  written=False: an operand between plain NaN bands."""

    def __init__(self, data, count, off, dev, written):
        data = torch.from_numpy(data) if isinstance(data, np.ndarray) else data
        if off == 0:
            self.g = Guarded((count,), dev, data=None if written else data)
            self.body = self.g.t
        else:
            self.g = Padded(None if written else data.view(1, count), count, off, dev, sentinel=written, shape=(1, count))
            self.body = self.g.view[0]
        if written and data is not None:
            self.body.copy_(data.to(dev))
        self.ptr = self.body.data_ptr()
        assert self.ptr % 16 == 4 * off and self.body.is_contiguous() and self.body.numel() == count
        self.written = written

    def intact(self):
        if self.written or isinstance(self.g, Guarded):
            return self.g.outside_untouched()
        return bool(torch.isnan(self.g.buf[:self.g.start]).all()) and bool(torch.isnan(self.g.buf[self.g.start + self.body.numel():]).all())

    def np(self):
        return self.body.cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _health(dev, first=0):
    h = Guarded((2,), dev, dtype=torch.int32, name="health")
    h.t.copy_(torch.tensor([first, 0], dtype=torch.int32))
    return h


# ================================================================================================================ vocr_clamp_adam
def _adam_call(state, wd, gs, step, dev, off=0, health=None, clamp=sg.CLAMP):
    """one vocr_clamp_adam on fresh guarded copies of `state`; returns (p', m', v') as numpy and the four buffers"""
    from vistaocr_amd import _lib
    p, g, m, v = state
    n = p.shape[0]
    P, M, V = (Buf(x, n, off, dev, written=True) for x in (p, m, v))
    G = Buf(g, n, off, dev, written=False)
    _lib.call("vocr_clamp_adam", _ptr(P.ptr), _ptr(G.ptr), _ptr(M.ptr), _ptr(V.ptr), n, sg.LR, sg.BETA1, sg.BETA2, sg.EPS, wd, clamp, gs, step,
              _ptr(health.ptr) if health is not None else None, _stream())
    return (P.np(), M.np(), V.np()), (P, G, M, V)


def _adam_check(state, wd, gs, step, dev, off=0, twice=False, what=""):
    """a step inside the bars, bands intact, g unchanged, idle elements keep p, health stays [0, 0]; returns the three worst ratios"""
    args = HYPER + (wd, sg.CLAMP, gs, step)
    h = _health(dev)
    got, bufs = _adam_call(state, wd, gs, step, dev, off, h)
    ref, bars = sg.adam_step64(*state, *args), sg.adam_bars(*state, *args)
    r = sg.adam_ratios(got, ref, bars)
    where = "%s count %d step %d wd %g gs %.3g off %d" % (what, state[0].shape[0], step, wd, gs, off)
    for k, name in zip("pmv", ("p", "exp_avg", "exp_avg_sq")):
        i = r[k][1]
        assert r[k][0] <= 1.0, "%s: %s outside its bar: ratio %.3f at element %d (p %r g %r m %r v %r -> got %r, fp64 %r)" % (
            where, name, r[k][0], i, state[0][i], state[1][i], state[2][i], state[3][i], got["pmv".index(k)][i], ref["pmv".index(k)][i])
    for b, name in zip(bufs, "pgmv"):
        assert b.intact(), "%s: the bands of %s were touched" % (where, name)
    assert np.array_equal(bufs[1].np().view(np.int32), state[1].view(np.int32)), "%s: the gradient changed" % where
    assert h.t.tolist() == [0, 0] and h.outside_untouched(), "%s: health %r" % (where, h.t.tolist())
    if wd == 0.0:
        idle = sg.adam_idle(*state[1:])
        assert np.array_equal(got[0][idle].view(np.int32), state[0][idle].view(np.int32)), "%s: an element with g = m = v = 0 moved" % where
    if twice:
        again, _ = _adam_call(state, wd, gs, step, dev, off, None)
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, again)), "%s: two runs differ" % where
    return r["p"][0], r["m"][0], r["v"][0]


def _row(name, worst, extra=""):
    print("\n%-34s worst ratio to the bar: p %.3f  m %.3f  v %.3f%s" % (name, worst[0], worst[1], worst[2], extra))


def _fold(worst, r):
    return tuple(max(a, b) for a, b in zip(worst, r))


@pytest.mark.parametrize("count", sg.ADAM_SMALL_COUNTS)
def test_adam_every_step_decay_and_scale(dev, count):
    """the full product of the step, weight-decay and gradient-scale lists at a count below, on and above one block"""
    worst, idle = (0.0, 0.0, 0.0), 0
    for step in sg.ADAM_STEPS:
        state = sg.adam_inputs(count, step, seed=11)
        idle += int(sg.adam_idle(*state[1:]).sum())
        for wd in sg.ADAM_WDS:
            for gs in sg.ADAM_SCALES:
                worst = _fold(worst, _adam_check(state, wd, gs, step, dev, twice=(gs == 0.5), what="small"))
    assert idle > 0 or count == 1
    _row("adam count %d, 30 settings" % count, worst)


@pytest.mark.parametrize("count", sg.ADAM_LARGE_COUNTS)
def test_adam_around_the_grid_cap(dev, count):
    """4096 x 256 threads: one element short of the cap, on it, the first element of the second trip, the third trip"""
    worst = (0.0, 0.0, 0.0)
    for step, wd, gs in sg.ADAM_LARGE_SETTINGS:
        state = sg.adam_inputs(count, step, seed=11)
        assert sg.adam_idle(*state[1:])[sg.ADAM_GRID_CAP - 4096:].any() or step != 1
        worst = _fold(worst, _adam_check(state, wd, gs, step, dev, twice=True, what="large"))
    _row("adam count %d, 2 settings" % count, worst, "  (two runs bit-identical)")


@pytest.mark.parametrize("count", (1, 257, sg.ADAM_GRID_CAP + 1))
def test_adam_all_pointers_one_float_off(dev, count):
    worst = (0.0, 0.0, 0.0)
    for step, wd, gs in ((2, 0.01, 0.5), (1000, 0.0, 1.0)):
        worst = _fold(worst, _adam_check(sg.adam_inputs(count, step, seed=12), wd, gs, step, dev, off=1, twice=True, what="off1"))
    _row("adam count %d, pointers + 4 bytes" % count, worst)


@pytest.mark.parametrize("count", (257, sg.ADAM_LARGE_COUNTS[-1]))
def test_adam_nan_policy(dev, count):
    """one NaN gradient at the first, a middle and the last element (above the cap: the last element of the third trip): p, m, v of that
    element become NaN, every other element stays inside the bars, health[1] = 1 and health[0] keeps what it held; the same without a
    health word; +-inf * grad_scale clamps and raises nothing"""
    step, wd, gs = 10, 0.01, 0.5
    args = HYPER + (wd, sg.CLAMP, gs, step)
    worst = (0.0, 0.0, 0.0)
    base = sg.adam_inputs(count, step, seed=13)
    base_ref, bars = sg.adam_step64(*base, *args), sg.adam_bars(*base, *args)
    for at in (0, count // 2, count - 1):
        state = (base[0], base[1].copy(), base[2], base[3])
        state[1][at] = np.nan
        ref = tuple(r.copy() for r in base_ref)                   # the operation is elementwise: only element `at` has another reference
        for r in ref:
            r[at] = np.nan
        for with_health in (True, False):
            h = _health(dev, first=7) if with_health else None
            got, bufs = _adam_call(state, wd, gs, step, dev, 0, h)
            for x, name in zip(got, "pmv"):
                nan = np.isnan(x)
                assert nan[at] and nan.sum() == 1, "NaN gradient at %d of %d: %s has NaN at %r" % (at, count, name, np.flatnonzero(nan)[:8])
            r = sg.adam_ratios(got, ref, bars)                    # (leaves the NaN element out, counts any other NaN as infinite)
            assert max(x[0] for x in r.values()) <= 1.0, (at, count, r)
            worst = _fold(worst, (r["p"][0], r["m"][0], r["v"][0]))
            assert all(b.intact() for b in bufs)
            assert np.isnan(bufs[1].np()[at]) and np.array_equal(np.delete(bufs[1].np(), at).view(np.int32), np.delete(state[1], at).view(np.int32))
            if with_health:
                assert h.t.tolist() == [7, 1] and h.outside_untouched(), h.t.tolist()
    # +-inf: inf * 0.5 = inf clamps to +-clamp like any large gradient, no health report
    state = sg.adam_inputs(count, step, seed=14)
    state[1][0], state[1][count - 1] = np.inf, -np.inf
    h = _health(dev, first=7)
    got, bufs = _adam_call(state, wd, gs, step, dev, 0, h)
    r = sg.adam_ratios(got, sg.adam_step64(*state, *args), sg.adam_bars(*state, *args))
    assert max(x[0] for x in r.values()) <= 1.0 and all(np.isfinite(x).all() for x in got), r
    assert h.t.tolist() == [7, 0] and all(b.intact() for b in bufs)
    _row("adam count %d, NaN / inf gradients" % count, _fold(worst, (r["p"][0], r["m"][0], r["v"][0])), "  (health [7, 1] / [7, 0])")


def test_adam_count_zero_and_refused_clamp(dev):
    """count == 0: VOCR_OK and nothing touched; clamp < 0 or NaN: VOCR_EINVAL in front of any launch (vocr_clamp's contract)"""
    from vistaocr_amd import _lib
    lib = _lib.load()
    state = sg.adam_inputs(8, 2, seed=15)
    for count, clamp, want in ((0, 5.0, 0), (8, -1.0, -1), (8, float("nan"), -1), (0, -1.0, -1)):
        P, M, V = (Buf(x, 8, 0, dev, written=True) for x in (state[0], state[2], state[3]))
        G, h = Buf(state[1], 8, 0, dev, written=False), _health(dev, first=7)
        rc = lib.vocr_clamp_adam(_ptr(P.ptr), _ptr(G.ptr), _ptr(M.ptr), _ptr(V.ptr), count, sg.LR, sg.BETA1, sg.BETA2, sg.EPS, 0.01, clamp, 1.0, 3,
                                 _ptr(h.ptr), _stream())
        torch.cuda.synchronize()
        assert rc == want, (count, clamp, rc)
        if want:
            assert b"vocr_clamp_adam: clamp" in lib.vocr_last_error()
        for b, x in zip((P, G, M, V), (state[0], state[1], state[2], state[3])):
            assert np.array_equal(b.np().view(np.int32), x.view(np.int32)) and b.intact()
        assert h.t.tolist() == [7, 0]
    print("\nadam count 0: OK, untouched; clamp -1 / NaN: VOCR_EINVAL, untouched")


def _flat_steps(opt, first_step, nsteps, wd, gs, seed):
    """nsteps of opt.step(grad_scale=gs), each held to adam_step64 from the flat buffers' contents before it"""
    worst = (0.0, 0.0, 0.0)
    n = opt.flat_p.numel()
    for k in range(nsteps):
        step = first_step + k
        opt.zero_grad()
        opt.flat_g.copy_(torch.from_numpy(sg.adam_inputs(n, 2, seed=seed + k)[1]))
        state = tuple(t.cpu().numpy() for t in (opt.flat_p, opt.flat_g, opt.exp_avg, opt.exp_avg_sq))
        opt.step(grad_scale=gs)
        assert opt.step_count == step
        got = tuple(t.cpu().numpy() for t in (opt.flat_p, opt.exp_avg, opt.exp_avg_sq))
        args = HYPER + (wd, sg.CLAMP, gs, step)
        r = sg.adam_ratios(got, sg.adam_step64(*state, *args), sg.adam_bars(*state, *args))
        assert max(x[0] for x in r.values()) <= 1.0, "FlatClampAdam step %d: %r" % (step, r)
        worst = _fold(worst, (r["p"][0], r["m"][0], r["v"][0]))
    return worst


def test_flat_clamp_adam_steps_and_resumes_on_the_same_bars(dev):
    """twenty steps of FlatClampAdam(weight_decay=1e-5).step(grad_scale=0.5) over parameters of 1, 7, 256 and 3 x 5 elements, then twenty
    more in a fresh optimiser that loaded the state dict with its step set to 99 990: the step count that reaches the kernel is the
    resumed one (a restart at 1 would use bias corrections of 0.1 and 0.001)"""
    import copy
    from vistaocr_amd import FlatClampAdam, ops
    ops.reset_health(dev)
    g = torch.Generator().manual_seed(5)
    shapes = ((1,), (7,), (256,), (3, 5))
    params = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in shapes]
    opt = FlatClampAdam(params, lr=sg.LR, betas=(sg.BETA1, sg.BETA2), eps=sg.EPS, weight_decay=1e-5, clamp=sg.CLAMP)
    assert opt.flat_p.numel() == 279
    worst = _flat_steps(opt, 1, 20, 1e-5, 0.5, seed=100)
    assert all(p.data_ptr() == opt.flat_p.data_ptr() + 4 * off for p, off in zip(params, (0, 1, 8, 264)))
    _row("FlatClampAdam steps 1 .. 20", worst)
    sd = copy.deepcopy(opt.state_dict())
    for st in sd["state"].values():
        st["step"] = torch.tensor(99990.0)
    fresh = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt2 = FlatClampAdam(fresh, lr=0.5, betas=(0.5, 0.5), eps=1.0, weight_decay=0.5, clamp=1.0)       # every hyperparameter comes from the state
    opt2.load_state_dict(sd)
    assert opt2.step_count == 99990 and opt2.param_groups[0]["weight_decay"] == 1e-5 and opt2.param_groups[0]["clamp"] == sg.CLAMP
    assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq) and torch.equal(opt2.flat_p, opt.flat_p)
    worst = _flat_steps(opt2, 99991, 20, 1e-5, 0.5, seed=200)
    _row("FlatClampAdam steps 99991 .. 100010", worst)
    assert ops.health(dev).tolist() == [0, 0]


# ================================================================================================================ vocr_clamp
@pytest.mark.parametrize("count", sg.CLAMP_COUNTS)
def test_clamp_bit_exact(dev, count):
    """16-byte loop + scalar tail (aligned) and the all-scalar loop (1, 2, 3 floats off) against torch.clamp on the CPU, as bits; NaN
    stays NaN and raises health[1], nothing else does (+-inf included)"""
    from vistaocr_amd import _lib
    runs = 0
    for clamp in sg.CLAMP_VALUES:
        # (the special values; then every element beyond the clamp, so that an element the in-place kernel skips shows)
        for nan_at, outside in (((), False), ((), True), ((0,), True), ((count - 1,), False), ((count // 2, count - 1), True)):
            x = sg.clamp_data(count, clamp, seed=21, nan_at=nan_at, outside=outside)
            want = torch.clamp(torch.from_numpy(x), -clamp, clamp)
            nan = torch.isnan(want)
            assert int(nan.sum()) == len(set(nan_at))
            for off in sg.OFFSETS:
                X, h = Buf(x, count, off, dev, written=True), _health(dev, first=7)
                _lib.call("vocr_clamp", _ptr(X.ptr), count, clamp, _ptr(h.ptr), _stream())
                got = X.body.cpu()
                where = "count %d clamp %g nan_at %r %s off %d" % (count, clamp, nan_at, "outside" if outside else "specials", off)
                assert torch.equal(torch.isnan(got), nan), where
                assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), where
                assert X.intact(), where + ": bands touched"
                assert h.t.tolist() == [7, 1 if nan_at else 0] and h.outside_untouched(), (where, h.t.tolist())
                runs += 1
    X = Buf(sg.clamp_data(count, 5.0, seed=22, nan_at=(count - 1,)), count, 0, dev, written=True)
    _lib.call("vocr_clamp", _ptr(X.ptr), count, 5.0, None, _stream())                                    # health = NULL is accepted
    assert X.intact() and bool(torch.isnan(X.body[count - 1])) and float(X.body[:count - 1].abs().max() if count > 1 else 0) <= 5.0
    print("\nclamp count %d: %d runs bit-exact (clamp 5 / inf, 4 alignments, special values / all beyond the clamp, NaN nowhere / first / last / two), "
          "health[1] iff NaN" % (count, runs))


# ================================================================================================================ the permutes
def _wbch(x):
    b, c, h, w = x.shape
    return x.permute(3, 0, 1, 2).contiguous().view(w * b, c * h)


def _out2d(rows, cols, off, dev):
    if off == 0:
        return Guarded((rows, cols), dev)
    return Padded(None, cols, off, dev, sentinel=True, shape=(rows, cols))


def _out_tensor(o):
    return o.t if isinstance(o, Guarded) else o.view


@pytest.mark.parametrize("b", (1, 2, 3))
def test_permutes_bit_exact_at_every_tile_seam(dev, b):
    from vistaocr_amd import _lib
    shapes = [s for s in sg.permute_shapes() if s[0] == b]
    assert shapes
    for shape in shapes:
        _, c, h, w = shape
        x = torch.from_numpy(sg.permute_data(shape, seed=31))
        y = _wbch(x)                                              # [w b][c h]
        X = Guarded(shape, dev, data=x)                           # between NaN bands: a masked load that is not masked brings one in
        Y = Guarded((w * b, c * h), dev, data=y)
        for off in (0, 1):
            O = _out2d(w * b, c * h, off, dev)
            _lib.call("vocr_bchw_to_wbch", _ptr(X.ptr), _ptr(_out_tensor(O).data_ptr()), b, c, h, w, _stream())
            got = _out_tensor(O).cpu()
            assert not torch.isnan(got).any(), "bchw_to_wbch %r off %d: unwritten or read outside" % (shape, off)
            assert torch.equal(_bits(got), _bits(y)), "bchw_to_wbch %r off %d" % (shape, off)
            assert O.outside_untouched() and X.outside_untouched(), "bchw_to_wbch %r off %d: bands touched" % (shape, off)
            B = _out2d(b * c * h, w, off, dev)
            _lib.call("vocr_wbch_to_bchw", _ptr(Y.ptr), _ptr(_out_tensor(B).data_ptr()), b, c, h, w, _stream())
            back = _out_tensor(B).cpu()
            assert not torch.isnan(back).any(), "wbch_to_bchw %r off %d: unwritten or read outside" % (shape, off)
            assert torch.equal(_bits(back), _bits(x.view(b * c * h, w))), "wbch_to_bchw %r off %d" % (shape, off)
            assert B.outside_untouched() and Y.outside_untouched(), "wbch_to_bchw %r off %d: bands touched" % (shape, off)
        # the round trip through the library's own output
        O, R = Guarded((w * b, c * h), dev), Guarded(shape, dev)
        _lib.call("vocr_bchw_to_wbch", _ptr(X.ptr), _ptr(O.ptr), b, c, h, w, _stream())
        _lib.call("vocr_wbch_to_bchw", _ptr(O.ptr), _ptr(R.ptr), b, c, h, w, _stream())
        assert torch.equal(R.bits(), X.bits()) and R.outside_untouched() and O.outside_untouched(), "round trip %r" % (shape,)
    print("\npermutes b = %d: %d shapes x (both directions x output aligned / + 4 bytes, round trip) bit-exact, bands intact" % (b, len(shapes)))


def test_transpose2d_and_the_autograd_wrapper(dev):
    from vistaocr_amd import _lib, ops
    sizes = sorted(set(sg.PERMUTE_WS) | set(sg.PERMUTE_CHS))
    for r in sizes:
        for c in sizes:
            x = torch.from_numpy(sg.permute_data((r, c), seed=32))
            X = Guarded((r, c), dev, data=x)
            got = ops.transpose2d(X.t)
            assert got.shape == (c, r) and torch.equal(_bits(got.cpu()), _bits(x.t().contiguous())), "transpose2d %d x %d" % (r, c)
    checked = 0
    for shape in ((1, 63, 1, 33), (3, 13, 5, 65), (3, 26, 5, 32), (2, 256, 7, 45)):
        b, c, h, w = shape
        x = torch.from_numpy(sg.permute_data(shape, seed=33)).to(dev).requires_grad_(True)
        dy = torch.from_numpy(sg.permute_data((w * b, c * h), seed=34)).to(dev)
        y = ops.PermuteBchwToWbchFn.apply(x, None)
        y.backward(dy)
        O, B = Guarded((w * b, c * h), dev), Guarded(shape, dev)
        _lib.call("vocr_bchw_to_wbch", _ptr(x.detach()), _ptr(O.ptr), b, c, h, w, _stream())
        _lib.call("vocr_wbch_to_bchw", _ptr(dy), _ptr(B.ptr), b, c, h, w, _stream())
        assert torch.equal(_bits(y.detach()), O.bits().view(w * b, c * h)) and torch.equal(_bits(x.grad), B.bits().view(shape)), shape
        assert torch.equal(_bits(y.detach().cpu()), _bits(_wbch(x.detach().cpu())))
        checked += 1
    print("\ntranspose2d %d x %d sizes bit-exact; PermuteBchwToWbchFn forward + backward = the entry points on %d shapes" % (len(sizes), len(sizes), checked))


# ================================================================================================================ the dropout draw
_MASKS = {}


def _mask_ref(n, p, seed):
    key = (n, p, seed)
    if key not in _MASKS:
        _MASKS[key] = torch.from_numpy(sg.dropout_mask_ref(n, p, seed))
    return _MASKS[key]


def _dropout_cases(count):
    """(p, seed, (x, out, mask) offsets): the full product below the grid cap; above it every seed, every p and every alignment once"""
    aligned, offs = (0, 0, 0), ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))
    if count < sg.EW_GRID_CAP:
        return [(p, s, o) for p in sg.DROPOUT_PS for s in sg.DROPOUT_SEEDS for o in offs]
    return [(0.3, s, aligned) for s in sg.DROPOUT_SEEDS] + [(p, sg.DROPOUT_SEEDS[2], aligned) for p in (0.0, 0.5)] + \
           [(0.5, sg.DROPOUT_SEEDS[4], o) for o in offs[1:]]


@pytest.mark.parametrize("count", sg.DROPOUT_COUNTS)
def test_dropout_stream_is_its_definition(dev, count):
    from vistaocr_amd import _lib
    x = sg.dropout_data(count, seed=41)
    cases = _dropout_cases(count)
    for p, seed, (ox, oo, om) in cases:
        mk = _mask_ref(count, p, seed)
        want = torch.from_numpy(x * mk.numpy())                  # one fp32 product per element
        where = "count %d p %g seed %#x offsets %r" % (count, p, seed, (ox, oo, om))
        X = Buf(x, count, ox, dev, written=False)
        O, M = Buf(None, count, oo, dev, written=True), Buf(None, count, om, dev, written=True)
        _lib.call("vocr_dropout_fwd", _ptr(X.ptr), _ptr(O.ptr), _ptr(M.ptr), count, p, seed, _stream())
        assert torch.equal(_bits(M.body.cpu()), _bits(mk)), where + ": vocr_dropout_fwd's mask"
        assert torch.equal(_bits(O.body.cpu()), _bits(want)), where + ": out != x * mask"
        assert O.intact() and M.intact() and X.intact(), where + ": bands touched"
        if ox == 0 and oo == 0:                                   # the mask kernel has one pointer: aligned and one float off
            M2 = Buf(None, count, om, dev, written=True)
            _lib.call("vocr_dropout_mask", _ptr(M2.ptr), count, p, seed, _stream())
            assert torch.equal(_bits(M2.body.cpu()), _bits(mk)), where + ": vocr_dropout_mask"
            assert M2.intact(), where + ": vocr_dropout_mask touched its bands"
    kept = float((_mask_ref(count, 0.5, sg.DROPOUT_SEEDS[4]) != 0).float().mean())
    print("\ndropout count %d: %d cases, both kernels = the stream's definition bit for bit, out = x * mask (kept at p 0.5: %.4f)" % (count, len(cases), kept))
