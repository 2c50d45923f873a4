"""GPU: vocr_gemm, vocr_gemm_pair, vocr_colsum and the elementwise kernels of gemm.hip against float64 at every tile and split seam.

Each row of tests/gemm_ref.py's table is named for one launch path (tile shape x load form x cut form, panel kernel whole / split, the
pair's one launch or its two-call fallback).  A test first asserts with vocr_gemm_plan - the planner the entry points launch from - that
every call of the row takes that path on this device, then runs integers and power-of-two selectors (bit-exact, torch.equal, no
tolerance) and N(0,1) floats (2e-5 x the result's scale) through all its layouts and epilogues, twice (bitwise reproducible), on
NaN-poisoned padded operands with sentinel guard bands around C.  Because every route equals the float64 reference bit for bit on
integers, every route to one product - panel, tile, cut, uncut, half or no workspace, pair or two calls - gives identical bits.
Worst float errors per path: profiles/gemm_fp64_errors.txt."""
import ctypes

import pytest
import torch

from tests import gemm_ref as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from vistaocr_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _ptr(t):
    return ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else None


def _workspace(nbytes, dev):
    """NaN-filled, 16-byte aligned; NULL for 0 bytes"""
    if nbytes <= 0:
        return None
    return torch.full(((nbytes + 3) // 4 + 4,), float("nan"), device=dev)


def _bias_buffers(case, biases, dev):
    """the biases in ONE allocation, each `bias_off` floats behind a 16-byte boundary, NaN around them"""
    n4 = (case.n + 3) // 4 * 4 + 8
    buf = torch.full((gr.GUARD + len(biases) * n4 + gr.GUARD,), float("nan"), device=dev)
    views = []
    for i, b in enumerate(biases):
        s = gr.GUARD + i * n4 + case.bias_off
        buf[s:s + case.n] = b.to(dev)
        views.append(buf[s:s + case.n])
    return buf, views


def _launch(case, epi, layout, A, B, biases, c0s, dev):
    """One call of the case's entry point into fresh poisoned C buffers; returns them."""
    from vistaocr_amd import _lib
    lib = _lib.load()
    ta, tb = layout
    lda, ldb, ldc = case.lds(ta, tb)
    has_bias, relu, acc = gr.EPILOGUES[epi]
    nout = 2 if case.pair == 0 else 1
    C = [gr.Padded(c0s[i] if acc else None, ldc, 0, dev, sentinel=True, shape=(case.m, case.n)) for i in range(nout)]
    nbytes = gr.workspace_bytes(case, epi, lib, ta, tb)
    ws = _workspace(nbytes, dev)
    bp = [_ptr(b) if has_bias else None for b in biases]
    al = 0
    for t in A + B:
        al |= t.ptr
    assert (al % 16 == 0) == bool(case.aligned(epi) & 1), "operand alignment is not what the case declares"
    al = 0
    for t in C:
        al |= t.ptr
    for b in biases:
        al |= b.data_ptr() if has_bias else 0
    assert (al % 16 == 0) == bool(case.aligned(epi) & 2), "output / bias alignment is not what the case declares"
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if case.pair is None:
        _lib.call("vocr_gemm", ta, tb, case.m, case.n, case.k, _ptr(A[0].ptr), lda, _ptr(B[0].ptr), ldb, _ptr(C[0].ptr), ldc, bp[0], relu, acc,
                  _ptr(ws), nbytes, stream)
    else:
        mode = case.pair | (4 if case.tiles_only else 0)
        _lib.call("vocr_gemm_pair", mode, ta, tb, case.m, case.n, case.k, _ptr(A[0].ptr), _ptr(A[1].ptr), lda, _ptr(B[0].ptr), _ptr(B[1].ptr), ldb,
                  _ptr(C[0].ptr), _ptr(C[1].ptr) if nout == 2 else None, ldc, bp[0], bp[1] if nout == 2 else None, relu, _ptr(ws), nbytes, stream)
    return C


def _products(case, kind, seed):
    """[(A, B, bias, prior C, float64 A B)] per output, and the operand matrices per launch slot (A0, A1), (B0, B1) with `shared_a`."""
    m, n, k = case.m, case.n, case.k
    if case.pair is None:
        d = gr.make_data(kind, m, n, k, seed)
        return [d], [d[0]], [d[1]]
    if case.pair == 1:                                   # two K segments of ONE product
        d = gr.make_data(kind, m, n, 2 * k, seed)
        return [d], [d[0][:, :k].contiguous(), d[0][:, k:].contiguous()], [d[1][:k].contiguous(), d[1][k:].contiguous()]
    d0, d1 = gr.make_data(kind, m, n, k, seed), gr.make_data(kind, m, n, k, seed + 1)
    if kind in ("ints", "floats"):                       # a0 == a1, as the step's x-projections use the pair
        d1 = (d0[0], d1[1], d1[2], d1[3], d0[0].double() @ d1[1].double())
    return [d0, d1], [d0[0], d1[0]], [d0[1], d1[1]]


def _assert_paths(case, lib):
    for epi in case.epis:
        for layout in case.layouts:
            plans = gr.plans_of(case, epi, layout, lib)
            got, want = gr.path_name(plans), case.expected_path(epi, layout)
            assert got == want, "%s, %s, %s: the call takes %s, the case is about %s (%r)" % (case, epi, gr.LAYOUT_NAMES[layout], got, want, plans)
            for key, val in case.plan.get(epi, case.plan.get("*", {})).items():
                if plans[0][1]["kernel"] == "panel" or key in ("pieces_per_tile", "n_whole"):
                    assert plans[0][1][key] == val, "%s, %s, %s: %s = %d, the case is about %d" % (case, epi, gr.LAYOUT_NAMES[layout], key, plans[0][1][key], val)


@pytest.mark.parametrize("case", gr.CASES, ids=[c.name.replace(" ", "_") for c in gr.CASES])
def test_gemm_case(dev, case):
    from vistaocr_amd import _lib
    lib = _lib.load()
    _assert_paths(case, lib)                              # the path first, the values after
    worst = {}
    for ki, kind in enumerate(case.kinds):
        prods, a_mats, b_mats = _products(case, kind, 1000 + 17 * ki)
        ab = [p[4].to(dev) for p in prods]
        c0s = [p[3].to(dev) for p in prods]
        bias_buf, biases = _bias_buffers(case, [p[2] for p in prods], dev)
        for layout in case.layouts:
            ta, tb = layout
            lda, ldb, ldc = case.lds(ta, tb)
            A = [gr.Padded(gr.stored(a, ta), lda, case.a_offset(), dev) for a in a_mats]
            if case.pair == 0 and a_mats[0] is a_mats[1]:
                A[1] = A[0]
            B = [gr.Padded(gr.stored(b, tb), ldb, 0, dev) for b in b_mats]
            for epi in case.epis:
                what = "%s, %s, %s, %s" % (case, kind, gr.LAYOUT_NAMES[layout], epi)
                C = _launch(case, epi, layout, A, B, biases, c0s, dev)
                C2 = _launch(case, epi, layout, A, B, biases, c0s, dev)
                for i, (c, c2) in enumerate(zip(C, C2)):
                    assert torch.equal(c.buf.view(torch.int32), c2.buf.view(torch.int32)), what + ": two runs differ"
                    ref = gr.reference(ab[i], biases[i], c0s[i], epi)
                    if kind == "floats":
                        scale = float(ref.abs().max())
                        err = float((c.view.double() - ref).abs().max())
                        key = case.expected_path(epi, layout)
                        worst[key] = max(worst.get(key, 0.0), err / scale if err == err else float("inf"))
                        assert err <= gr.FLOAT_BAR * scale, "%s, output %d: max abs error %.3e at scale %.3e (bar %.1e x scale)" % (what, i, err, scale, gr.FLOAT_BAR)
                    else:
                        want = ref.float()
                        if not torch.equal(c.view, want):
                            bad = torch.nonzero(~(c.view == want))
                            r, q = int(bad[0][0]), int(bad[0][1])
                            raise AssertionError("%s, output %d: %d of %d elements differ from float64; first at [%d][%d]: got %r, want %r"
                                                 % (what, i, bad.shape[0], want.numel(), r, q, float(c.view[r, q]), float(want[r, q])))
                    assert c.outside_untouched(), what + ": a row gap or guard band of C was written"
    for key, rel in sorted(worst.items()):
        print("GEMM_ERR | %s | %s | %.3e" % (case.name, key, rel))


# ---------------------------------------------------------------------------------------------------------------- vocr_colsum
def _colsum(x, m, n, dev, with_ws):
    from vistaocr_amd import _lib
    lib = _lib.load()
    xb = torch.full((gr.GUARD + m * n + gr.GUARD,), float("nan"), device=dev)
    xb[gr.GUARD:gr.GUARD + m * n] = x.reshape(-1).to(dev)
    out = gr.Padded(None, n + 4, 0, dev, sentinel=True, shape=(1, n))
    nb = lib.vocr_colsum_workspace_bytes(m, n) if with_ws else 0
    ws = _workspace(nb, dev)
    _lib.call("vocr_colsum", _ptr(xb[gr.GUARD:]), _ptr(out.ptr), m, n, _ptr(ws), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert out.outside_untouched(), "colsum %dx%d: wrote outside out[n]" % (m, n)
    return out.view[0], nb


def test_colsum_integers_bit_exact_around_the_split_rules(dev):
    """m around the row-split rules (one split per 32 rows, at most 64 and at most cdiv(1024, column tiles): 2049 rows of 64 columns are 64
    splits of 33 rows - not a multiple of the 8 rows a workgroup walks per step), n around the 64-column tile and one n (1100: 18 column
    tiles, 57 splits) where the column tiles cap the splits; with the workspace and with NULL (one workgroup per column tile).  NaN sits
    behind the last row."""
    g = torch.Generator().manual_seed(5)
    seen_splits = set()
    for m in (1, 31, 32, 33, 64 * 32 - 1, 64 * 32 + 1):
        for n in (1, 63, 64, 65, 1100):
            x = torch.randint(-8, 9, (m, n), generator=g).float()
            want = x.double().sum(0).float()
            for with_ws in (True, False):
                got, nb = _colsum(x, m, n, dev, with_ws)
                seen_splits.add(nb // (4 * n))
                assert torch.equal(got, want.to(dev)), "colsum %dx%d %s" % (m, n, "with workspace" if with_ws else "workspace NULL")
    assert {0, 2, 57, 64} <= seen_splits, seen_splits


def test_colsum_floats_fp64(dev):
    m, n = 64 * 32 + 1, 65
    x = torch.randn((m, n), generator=torch.Generator().manual_seed(6))
    want = x.double().sum(0)
    for with_ws in (True, False):
        got, _ = _colsum(x, m, n, dev, with_ws)
        err = float((got.double().cpu() - want).abs().max())
        print("GEMM_ERR | colsum %dx%d %s | colsum | abs %.3e" % (m, n, "ws" if with_ws else "null", err))
        assert err <= 1e-5 * m, err


# ---------------------------------------------------------------------------------------------------------------- elementwise
_EW_COUNTS = (1, 3, 4, 1023, 1024, 1025, 2048 * 256 * 4 + 1029)     # the last one is above the grid cap: the grid-stride loop wraps


def _ew_operand(t, count, off, dev, sentinel=False):
    p = gr.Padded(t[None, :] if t is not None else None, count, off, dev, sentinel=sentinel, shape=(1, count))
    return p


@pytest.mark.parametrize("op", ["relu_bwd", "mul", "add", "scale_dev"])
def test_elementwise_bit_exact(dev, op):
    """One fp32 operation per element: bit-exact against torch, at counts around the 16-byte vector and the 256-thread block and above the
    grid cap, with every operand 16-byte aligned (vector loop + scalar tail) and with each operand in turn one float off (scalar loop);
    the sentinel in front of and behind the output survives."""
    from vistaocr_amd import _lib
    g = torch.Generator().manual_seed(7)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for count in _EW_COUNTS:
        x, y = torch.randn(count, generator=g), torch.randn(count, generator=g)
        sc = torch.randn(1, generator=g)
        if op == "relu_bwd":
            want = torch.where(y > 0, x, torch.zeros(()))
        elif op == "mul":
            want = x * y
        elif op == "add":
            want = x + y
        else:
            want = x * sc
        want = want.to(dev)
        offsets = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)] if count < (1 << 20) else [(0, 0, 0), (1, 0, 0)]
        for ox, oy, oo in offsets:
            X, Y = _ew_operand(x, count, ox, dev), _ew_operand(y, count, oy, dev)
            O = _ew_operand(None, count, oo, dev, sentinel=True)
            if op == "scale_dev":
                S = torch.full((8,), float("nan"), device=dev)
                S[4 + oy] = sc.to(dev)[0]
                _lib.call("vocr_scale_dev", _ptr(X.ptr), _ptr(S[4 + oy:]), _ptr(O.ptr), count, stream)
            else:
                _lib.call("vocr_" + op, _ptr(X.ptr), _ptr(Y.ptr), _ptr(O.ptr), count, stream)
            assert torch.equal(O.view[0], want), "%s, count %d, offsets %r" % (op, count, (ox, oy, oo))
            assert O.outside_untouched(), "%s, count %d, offsets %r: wrote outside the output" % (op, count, (ox, oy, oo))
