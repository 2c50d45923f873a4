"""GPU: the conv kernels against the fp64 restatement of tests/cnn_ref.py at every tile seam, in guarded buffers (tests/cnn_cases.py: the
tables, why their values, and the buffers).  tests/test_cnn_fp64_gpu.py holds the same kernels at the model's layer shapes; here the
shapes are tiny and sit on the seams, every call goes through the C entry points so that the test owns every byte the kernel may touch,
and each call must
  - hold the bar of its kernel family (cnn_ref.conv_bar, unchanged; fp16-operand kernels against the fp64 conv of the fp16-ROUNDED operands;
    a minimal-filtering launch whose outputs sum fewer than cnn_ref.TINY_K products is held to the same constant on the scale of the
    transform's tile, as cnn_ref.py derives and tests/test_cnn_ref_cpu.py shows an honest fp32 transform to need),
  - write every element of every output (outputs start as NaN) and read nothing it did not write (operand bands and workspaces are NaN),
  - leave every guard and sentinel band as it was, the one behind the exactly-sized workspace included,
  - give the same bits when run again into fresh NaN-filled buffers, and the same bits as the ops.* wrapper the model calls (which
    allocates its own buffers and recycled workspaces: values only).
One test per kernel family, each asserting the launch plans it ran; `-s` prints case / quantity / error over bar.

vocr_conv3x3_wgrad_f16 hands Cin <= 3 to the fp32 kernel (conv.hip: the first layer is memory-bound), so those cases answer to the fp64
gradient of the EXACT operands at the direct bar; Cin = 8 runs the fp16-operand kernel and answers to the rounded ones."""
import time

import pytest
import torch

from tests import cnn_cases as cc
from tests import cnn_ref as cr

pytestmark = pytest.mark.gpu

_ROWS = []
_PLANS = {"wino": set(), "h16": set()}
_T0 = [None]
_F43 = {3, 4, 5, 6, 7, 8}


def _row(case, what, r):
    """record error / bar; the test that ran the case asserts the whole family at its end (_settle), so one run shows every excess"""
    _ROWS.append((case, what, r))


def _settle(start):
    over = ["%s %s: error / bar = %.3f" % row for row in _ROWS[start:] if not row[2] <= 1.0]
    assert len(_ROWS) > start and not over, "\n".join(over)


@pytest.fixture(scope="module", autouse=True)
def _table():
    _T0[0] = time.time()
    yield
    if _ROWS:
        print("\n%-40s %-46s %10s" % ("case", "quantity", "err / bar"))
        for case, what, r in _ROWS:
            print("%-40s %-46s %10.4f" % (case, what, r))
        print("%d rows, worst %.4f; wall time of the file %.1f s" % (len(_ROWS), max(r for _, _, r in _ROWS), time.time() - _T0[0]))


@pytest.fixture(scope="module")
def dev():
    from vistaocr_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _in(t, dev, name, dtype=torch.float32):
    return cc.Guarded(t.shape, dev, data=t, dtype=dtype, name=name)


def _twice(case, operands, run):
    """run() allocates fresh outputs / workspaces, calls the library and returns {name: Guarded or None}; names starting with "ws" are
    workspaces (only their bands are checked).  Runs it twice; returns the first run's buffers."""
    a, b = run(), run()
    torch.cuda.synchronize()
    for g in operands:
        assert g.outside_untouched(), "%s: the guard band of operand %s changed" % (case, g.name)
    for bufs in (a, b):
        for name, g in bufs.items():
            if g is None:
                continue
            assert g.outside_untouched(), "%s: a store outside %s" % (case, name)
            if not name.startswith("ws"):
                assert not g.has_nan(), "%s: NaN in %s (an element not written, or a read outside an operand / of unwritten workspace)" % (case, name)
    for name, g in a.items():
        if g is not None and not name.startswith("ws"):
            assert torch.equal(g.bits(), b[name].bits()), "%s: %s differs between two runs" % (case, name)
    return a


def _tag(shape):
    return "x".join(map(str, shape))


# ------------------------------------------------------------------------------------------- fp32 forward / data gradient
def _conv_case(dev, shape, dgrad, seed, tag, expect_plan=None):
    """one launch (n, K, h, w, M) of vocr_conv3x3_wino_fwd (M % 4 == 0) or vocr_conv3x3_fwd, with the forward pack of a layer K -> M and
    its bias, or (dgrad) the data-gradient pack of a layer M -> K; the pack is written into a guarded buffer by the library's own pack call"""
    from vistaocr_amd import _lib
    from vistaocr_amd._lib import call
    lib = _lib.load()
    n, k, h, w, m = shape
    x = cc.rand((n, k, h, w), seed + 1, 1.0, dev)
    wt = cc.rand((k, m, 3, 3) if dgrad else (m, k, 3, 3), seed + (4 if dgrad else 2), 0.2, dev)
    bias = None if dgrad else cc.rand((m,), seed + 3, 1.0, dev)
    wino = m % 4 == 0
    plan = lib.vocr_conv3x3_wino_plan(n, k, h, w, m) if wino else 0
    if wino:
        assert plan != 0, (tag, shape)
        _PLANS["wino"].add(plan)
    if expect_plan is not None:
        assert plan == expect_plan, "%s: the library reports plan %d for %s, the table says %d" % (tag, plan, shape, expect_plan)
    fam = ("f43" if (plan & 15) in _F43 else "f23") if wino else "direct"
    floats = lib.vocr_conv3x3_wino_pack_floats(m, k) if wino else 9 * m * k
    pack_fn = "vocr_conv3x3_wino_pack_weights" if wino else "vocr_conv3x3_pack_weights"
    gx, gw = _in(x, dev, "x"), _in(wt, dev, "w")
    gb = None if bias is None else _in(bias, dev, "bias")
    case = "%s %s" % (tag, _tag(shape))

    def run():
        pack = cc.Guarded((floats,), dev, name="pack")
        if dgrad:
            call(pack_fn, gw.ptr, None, pack.ptr, k, m, _st())
        else:
            call(pack_fn, gw.ptr, pack.ptr, None, m, k, _st())
        y = cc.Guarded((n, m, h, w), dev, name="y")
        call("vocr_conv3x3_wino_fwd" if wino else "vocr_conv3x3_fwd", gx.ptr, pack.ptr, None if gb is None else gb.ptr, y.ptr, n, k, h, w, m, _st())
        return {"pack": pack, "y": y}

    out = _twice(case, [g for g in (gx, gw, gb) if g is not None], run)
    if dgrad:
        ref, s = cr.conv3x3_dgrad(x, wt), cr.conv3x3_dgrad(x, wt, absolute=True)
    else:
        ref, s = cr.conv3x3(x, wt, bias), cr.conv3x3(x, wt, bias, absolute=True)
    what = "%s %s" % ("dgrad" if dgrad else "fwd", ("plan %d" % plan) if wino else "direct")
    if wino and 9 * k < cr.TINY_K:               # fewer products than one K step: the scale of the transform's tile (cnn_ref.TINY_K)
        what += " tile scale (plain %.2f)" % cr.ratio(out["y"].t, ref, cr.conv_bar(fam, s))
        s = cr.conv3x3_window(x, wt.transpose(0, 1).flip(2, 3) if dgrad else wt, bias, 4 if fam == "f43" else 2)
    _row(case, what, cr.ratio(out["y"].t, ref, cr.conv_bar(fam, s)))
    # the wrapper the model calls (its own torch.empty buffers: values only) takes the same kernel: the same bits
    from vistaocr_amd import ops
    got = ops.conv3x3_forward(x, ops.conv3x3_pack(wt)[1 if dgrad else 0], bias, m)
    assert torch.equal(got, out["y"].t), "%s: ops.conv3x3_forward differs from the entry point" % case
    if k == 1 and not dgrad:                     # the one-input-channel kernel on the layer's own weight
        def run_c1():
            y = cc.Guarded((n, m, h, w), dev, name="y")
            call("vocr_conv3x3_c1_fwd", gx.ptr, gw.ptr, gb.ptr, y.ptr, n, h, w, m, 0, _st())
            return {"y": y}
        _row(case, "fwd Cin=1", cr.ratio(_twice(case + " c1", [gx, gw, gb], run_c1)["y"].t, ref, cr.conv_bar("c1", s)))


@pytest.mark.parametrize("family", ["wino fwd", "wino dgrad", "direct fwd", "direct dgrad"])
def test_conv_fp32_seams(dev, family):
    """cout % 4 == 0: the minimal-filtering kernels (plans 1, 3, 4 at these grids); cout in {6, 10}: the direct kernel"""
    rows, start = (cc.WINO_CASES if family.startswith("wino") else cc.DIRECT_CASES), len(_ROWS)
    _PLANS["wino"].clear()
    for i, shape in enumerate(rows):
        _conv_case(dev, shape, family.endswith("dgrad"), 7 * i, family)
    assert _PLANS["wino"] == ({1, 3, 4} if family.startswith("wino") else set()), _PLANS["wino"]
    _settle(start)


def test_conv_large_grid_plans(dev):
    """the 8-wave and two-workgroup F(4,3) kernels and every "+16" tail-piece form, one shape per W % 4; the id is the library's answer"""
    start = len(_ROWS)
    _PLANS["wino"].clear()
    for plan in sorted(cc.PLAN_CASES):
        for i, shape in enumerate(cc.PLAN_CASES[plan]):
            _conv_case(dev, shape, False, 100 * plan + i, "plan %d" % plan, expect_plan=plan)
            torch.cuda.empty_cache()
    assert _PLANS["wino"] == set(cc.PLAN_CASES) == cc.REACHABLE_PLANS - {1, 3, 4}, _PLANS["wino"]
    _settle(start)


# ------------------------------------------------------------------------------------------------------------ weight gradient
def _wgrad_case(dev, shape, seed):
    from vistaocr_amd import _lib
    from vistaocr_amd._lib import call
    lib = _lib.load()
    n, cin, h, w, cout = shape
    kind, fam = cc.wgrad_kernel(cin, cout)
    x, dy = cc.rand((n, cin, h, w), seed + 1, 1.0, dev), cc.rand((n, cout, h, w), seed + 5, 1.0, dev)
    gx, gdy = _in(x, dev, "x"), _in(dy, dev, "dy")
    case = "wgrad %s %s" % (kind, _tag(shape))
    ref, s = cr.conv3x3_wgrad(x, dy), cr.conv3x3_wgrad(x, dy, absolute=True)
    what = kind
    if kind in ("rowpair", "wino3"):
        nbytes = lib.vocr_conv3x3_wgrad_wino_workspace_bytes(n, cin, h, w, cout)
        if kind == "rowpair":                    # 12 planes per split
            splits = cc.rowpair_splits(n, cin, h, w, cout)
            assert nbytes == splits * 12 * cout * cin * 4, (case, nbytes, splits)
            what = "rowpair %d splits %s" % (splits, "reduce<16>" if (3 * cout * cin // 4 + 63) // 64 < 64 and splits >= 64 else "reduce<4>")
        fn = "vocr_conv3x3_wgrad_wino"
    else:
        nbytes, fn = lib.vocr_conv3x3_wgrad_workspace_bytes(n, cin, h, w, cout), "vocr_conv3x3_wgrad"

    def run():
        dw, ws = cc.Guarded((cout, cin, 3, 3), dev, name="dw"), cc.workspace(nbytes, dev)
        call(fn, gx.ptr, gdy.ptr, dw.ptr, ws.ptr, n, cin, h, w, cout, _st())
        return {"dw": dw, "ws": ws}

    dw = _twice(case, [gx, gdy], run)["dw"].t
    if kind == "rowpair" and n * h * w < cr.TINY_K:
        what += " tile scale (plain %.2f)" % cr.ratio(dw, ref, cr.conv_bar(fam, s))
        s = cr.conv3x3_wgrad_window(x, dy)
    _row(case, what, cr.ratio(dw, ref, cr.conv_bar(fam, s)))
    from vistaocr_amd import ops
    by_ops = ops.conv3x3_wgrad(x, dy)            # recycled torch.empty workspace instead of NaN: values only, the same bits

    # the bias gradient of the same dy
    sb = lib.vocr_channel_sum_workspace_bytes(n, cout, h * w)

    def run_sum():
        db, ws = cc.Guarded((cout,), dev, name="db"), cc.workspace(sb, dev)
        call("vocr_channel_sum", gdy.ptr, db.ptr, n, cout, h * w, None if ws is None else ws.ptr, _st())
        return {"db": db, "ws": ws}

    db = _twice(case + " channel_sum", [gdy], run_sum)["db"].t
    db_ref, db_bar = dy.double().sum((0, 2, 3)), cr.conv_bar("direct", dy.double().abs().sum((0, 2, 3)))
    _row(case, "channel_sum", cr.ratio(db, db_ref, db_bar))
    if kind == "c1":                             # the one-channel kernel: dw and dbias from one pass over dy
        cb = lib.vocr_conv3x3_c1_wgrad_workspace_bytes(n, h, cout)

        def run_c1():
            dw, dbias, ws = cc.Guarded((cout, 1, 3, 3), dev, name="dw"), cc.Guarded((cout,), dev, name="dbias"), cc.workspace(cb, dev)
            call("vocr_conv3x3_c1_wgrad", gx.ptr, gdy.ptr, dw.ptr, dbias.ptr, ws.ptr, n, h, w, cout, _st())
            return {"dw": dw, "dbias": dbias, "ws": ws}

        out = _twice(case + " c1", [gx, gdy], run_c1)
        _row(case, "c1 dw", cr.ratio(out["dw"].t, ref, cr.conv_bar("direct", s)))
        _row(case, "c1 dbias", cr.ratio(out["dbias"].t, db_ref, db_bar))
        # two fixed-order fp32 sums of the same terms, each within the bar of the exact sum
        _row(case, "c1 dbias vs channel_sum", cr.ratio(out["dbias"].t, db.double(), 2 * db_bar))
        if ops.conv3x3_c1_wgrad_takes(cin, cout):
            dw = out["dw"].t
    assert torch.equal(by_ops, dw), "%s: ops.conv3x3_wgrad differs from the entry point" % case
    assert torch.equal(ops.channel_sum(dy), db), "%s: ops.channel_sum differs from the entry point" % case


@pytest.mark.parametrize("kind", ["rowpair", "wino3", "direct", "c1"])
def test_conv_wgrad_seams(dev, kind):
    """the row-pair F(3,2) kernel with both reduce kernels, the 768-thread kernel (Cin Cout % 4 != 0), the direct kernel (Cin <= 3) and
    the one-channel kernel with its bias gradient; vocr_channel_sum on the same dy"""
    rows = [(i, s) for i, s in enumerate(cc.WGRAD_CASES) if cc.wgrad_kernel(s[1], s[4])[0] == kind]
    start = len(_ROWS)
    for i, shape in rows:
        _wgrad_case(dev, shape, 11 * i)
    if kind == "rowpair":
        seen = {w.split()[3] for c, w, _ in _ROWS[start:] if w.startswith("rowpair")}
        assert seen == {"reduce<16>", "reduce<4>"}, seen
    _settle(start)


# ----------------------------------------------------------------------------------------------------------------------- fp16
def _f16_conv_case(dev, shape, dgrad, seed, tag, h16, expect_plan=None):
    """vocr_conv3x3_h16_fwd on the channel-blocked fp16 copy (h16) or vocr_conv3x3_f16_fwd on the fp32 tensor, forward or data-gradient
    pack, against the fp64 conv of the fp16-rounded operands"""
    from vistaocr_amd import _lib
    from vistaocr_amd._lib import call
    lib = _lib.load()
    n, k, h, w, m = shape
    x = cc.rand((n, k, h, w), seed + 1, 1.0, dev)
    wt = cc.rand((k, m, 3, 3) if dgrad else (m, k, 3, 3), seed + (4 if dgrad else 2), 0.2, dev)
    bias = None if dgrad else cc.rand((m,), seed + 3, 1.0, dev)
    case = "%s %s" % (tag, _tag(shape))
    plan = 0
    if h16:
        plan = lib.vocr_conv3x3_h16_plan(n, k, h, w, m)
        assert plan != 0, case
        _PLANS["h16"].add(plan)
        if expect_plan is not None:
            assert plan == expect_plan, "%s: the library reports h16 plan %d, the table says %d" % (case, plan, expect_plan)
        gx = _in(cc.f16_layouts_ref(x)[0], dev, "x16", torch.float16)
    else:
        gx = _in(x, dev, "x")
    gw = _in(wt, dev, "w")
    gb = None if bias is None else _in(bias, dev, "bias")
    # the pack of a layer (cout, cin): forward (m, k); data gradient: the layer is m -> k, (cout, cin) = (k, m)
    halfs = (lib.vocr_conv3x3_f16_pack_bytes(k, m, 1) if dgrad else lib.vocr_conv3x3_f16_pack_bytes(m, k, 0)) // 2

    def run():
        pack = cc.Guarded((halfs,), dev, dtype=torch.float16, name="pack")
        if dgrad:
            call("vocr_conv3x3_f16_pack_weights", gw.ptr, None, pack.ptr, k, m, _st())
        else:
            call("vocr_conv3x3_f16_pack_weights", gw.ptr, pack.ptr, None, m, k, _st())
        y = cc.Guarded((n, m, h, w), dev, name="y")
        call("vocr_conv3x3_h16_fwd" if h16 else "vocr_conv3x3_f16_fwd", gx.ptr, pack.ptr, None if gb is None else gb.ptr, y.ptr, n, k, h, w, m, _st())
        return {"pack": pack, "y": y}

    out = _twice(case, [g for g in (gx, gw, gb) if g is not None], run)
    xh, wh = x.half().double(), wt.half().double()
    if dgrad:
        ref, s = cr.conv3x3_dgrad(xh, wh), cr.conv3x3_dgrad(xh, wh, absolute=True)
    else:
        ref, s = cr.conv3x3(xh, wh, bias), cr.conv3x3(xh, wh, bias, absolute=True)
    what = "%s %s" % ("dgrad" if dgrad else "fwd", ("h16 plan %d" % plan) if h16 else "f16")
    _row(case, what, cr.ratio(out["y"].t, ref, cr.conv_bar("f16", s)))
    from vistaocr_amd import ops
    assert ops.h16_takes(n, k, h, w, m) == h16
    got = ops.conv3x3_forward_f16(x, ops.conv3x3_pack_f16(wt)[1 if dgrad else 0], bias, m)
    assert torch.equal(got, out["y"].t), "%s: ops.conv3x3_forward_f16 differs from the entry point" % case
    if k == 1 and not dgrad and not h16:         # the one-channel kernel with fp16-rounded operands
        def run_c1():
            y = cc.Guarded((n, m, h, w), dev, name="y")
            call("vocr_conv3x3_c1_fwd", gx.ptr, gw.ptr, gb.ptr, y.ptr, n, h, w, m, 1, _st())
            return {"y": y}
        _row(case, "fwd Cin=1 round_f16", cr.ratio(_twice(case + " c1", [gx, gw, gb], run_c1)["y"].t, ref, cr.conv_bar("c1", s)))


@pytest.mark.parametrize("family", ["h16 fwd", "h16 dgrad", "f16 fwd", "f16 dgrad"])
def test_conv_f16_seams(dev, family):
    h16, dgrad, start = family.startswith("h16"), family.endswith("dgrad"), len(_ROWS)
    _PLANS["h16"].clear()
    for i, shape in enumerate(cc.H16_CASES if h16 else cc.F16_CASES):
        _f16_conv_case(dev, shape, dgrad, 13 * i, family, h16)
    if h16:                                      # the tiles of 12 and 16 rows and of 64 pixels need a full grid to be picked
        for plan, shape in sorted(cc.H16_PLAN_CASES.items()):
            _f16_conv_case(dev, shape, dgrad, 1000 + plan, family, True, expect_plan=plan)
        assert _PLANS["h16"] == {1, 2, 3, 4, 5}, _PLANS["h16"]
    _settle(start)


def test_wgrad_f16_seams(dev):
    from vistaocr_amd import _lib
    from vistaocr_amd._lib import call
    lib, start = _lib.load(), len(_ROWS)
    # ---- vocr_conv3x3_wgrad_h16 on the padded channel-major copies (made by torch: the zero tails are the halo)
    for i, shape in enumerate(cc.WGRAD_H16_CASES):
        n, cin, h, w, cout = shape
        assert lib.vocr_conv3x3_wgrad_h16_supported(cin, cout)
        x, dy = cc.rand((n, cin, h, w), 17 * i + 1, 1.0, dev), cc.rand((n, cout, h, w), 17 * i + 5, 1.0, dev)
        gx, gdy = _in(cc.f16_layouts_ref(x)[1], dev, "x16p", torch.float16), _in(cc.f16_layouts_ref(dy)[1], dev, "dy16p", torch.float16)
        case = "wgrad_h16 %s" % _tag(shape)
        nbytes = lib.vocr_conv3x3_wgrad_h16_workspace_bytes(n, cin, h, w, cout)
        # every unit (64 pixels of a row) a split of its own: tiles x splits x (8 waves / 32x32 blocks of a tile) k-subsets x 9 taps x tile
        units, ctco = n * h * ((w + 63) // 64), min(cout, 128)
        tiles = (cout // ctco) * (cin // 64)
        assert units <= 256 // tiles
        assert nbytes == tiles * units * (8 // ((ctco // 32) * 2)) * 9 * ctco * 64 * 4, (case, nbytes)

        def run():
            dw, ws = cc.Guarded((cout, cin, 3, 3), dev, name="dw"), cc.workspace(nbytes, dev)
            call("vocr_conv3x3_wgrad_h16", gx.ptr, gdy.ptr, dw.ptr, ws.ptr, n, cin, h, w, cout, _st())
            return {"dw": dw, "ws": ws}

        xh, dyh = x.half().double(), dy.half().double()
        _row(case, "splits = units = %d" % units,
             cr.ratio(_twice(case, [gx, gdy], run)["dw"].t, cr.conv3x3_wgrad(xh, dyh), cr.conv_bar("f16", cr.conv3x3_wgrad(xh, dyh, absolute=True))))
    # ---- vocr_conv3x3_wgrad_f16 on the fp32 tensors: Cin <= 3 is the fp32 kernel (exact operands), Cin = 8 the fp16-operand one
    for i, shape in enumerate(cc.WGRAD_F16_CASES):
        n, cin, h, w, cout = shape
        x, dy = cc.rand((n, cin, h, w), 19 * i + 1, 1.0, dev), cc.rand((n, cout, h, w), 19 * i + 5, 1.0, dev)
        gx, gdy = _in(x, dev, "x"), _in(dy, dev, "dy")
        case = "wgrad_f16 %s" % _tag(shape)
        nbytes = lib.vocr_conv3x3_wgrad_workspace_bytes(n, cin, h, w, cout)

        def run():
            dw, ws = cc.Guarded((cout, cin, 3, 3), dev, name="dw"), cc.workspace(nbytes, dev)
            call("vocr_conv3x3_wgrad_f16", gx.ptr, gdy.ptr, dw.ptr, ws.ptr, n, cin, h, w, cout, _st())
            return {"dw": dw, "ws": ws}

        xr, dyr, fam = (x, dy, "direct") if cin <= 3 else (x.half().double(), dy.half().double(), "f16")
        _row(case, "fp32 kernel (Cin <= 3)" if cin <= 3 else "fp16 operands",
             cr.ratio(_twice(case, [gx, gdy], run)["dw"].t, cr.conv3x3_wgrad(xr, dyr), cr.conv_bar(fam, cr.conv3x3_wgrad(xr, dyr, absolute=True))))
    _settle(start)


def test_f32_to_f16_layouts_bit_for_bit(dev):
    """both copies equal x.half() rearranged, bit for bit; every padded element (w >= W up to WP) of the channel-major copy is zero - they
    are the weight-gradient kernel's halo; c = 8 takes the padded copy alone"""
    from vistaocr_amd import _lib
    from vistaocr_amd._lib import call
    lib = _lib.load()
    for i, (n, c, h, w) in enumerate(cc.LAYOUT_CASES):
        wp = lib.vocr_f16_padded_row(w)
        assert wp == cc.padded_row(w)
        x = cc.rand((n, c, h, w), 23 * i + 1, 4.0, dev)
        gx = _in(x, dev, "x")
        nhwc_ref, nchwp_ref = cc.f16_layouts_ref(x)
        case = "layouts %s" % _tag((n, c, h, w))
        forms = [(True, True), (True, False), (False, True)] if c % 16 == 0 else [(False, True)]
        for want_nhwc, want_p in forms:
            def run():
                a = cc.Guarded((n, c // 16, h, w, 16), dev, dtype=torch.float16, name="nhwc") if want_nhwc else None
                b = cc.Guarded((n, c, h, wp), dev, dtype=torch.float16, name="nchwp") if want_p else None
                call("vocr_f32_to_f16_layouts", gx.ptr, None if a is None else a.ptr, None if b is None else b.ptr, n, c, h, w, _st())
                return {"nhwc": a, "nchwp": b}
            out = _twice(case, [gx], run)
            if want_nhwc:
                assert torch.equal(out["nhwc"].t.view(torch.int16), nhwc_ref.view(torch.int16)), case
            if want_p:
                assert torch.equal(out["nchwp"].t.view(torch.int16), nchwp_ref.view(torch.int16)), case
                assert int(out["nchwp"].t[..., w:].view(torch.int16).abs().max()) == 0, case
        _ROWS.append((case, "bit for bit, zero tails", 0.0))


# ----------------------------------------------------------------------------------------------------------------- coverage
def test_the_tables_reach_every_launch_plan(dev):
    """every id vocr_conv3x3_wino_plan can report in the shipped library is the library's answer for a row of the tables, and the fp16
    kernels' plans 1 to 5 (the tests above assert the ids of the launches they ran)"""
    from vistaocr_amd import _lib
    lib = _lib.load()
    small = {lib.vocr_conv3x3_wino_plan(*s) for s in cc.WINO_CASES}
    table = small | {lib.vocr_conv3x3_wino_plan(*s) for v in cc.PLAN_CASES.values() for s in v}
    h16 = {lib.vocr_conv3x3_h16_plan(*s) for s in cc.H16_CASES} | {lib.vocr_conv3x3_h16_plan(*s) for s in cc.H16_PLAN_CASES.values()}
    print("\nplans of vocr_conv3x3_wino_fwd over the small table: %s, with the large grids: %s; of vocr_conv3x3_h16_fwd: %s"
          % (sorted(small), sorted(table), sorted(h16)))
    assert 0 not in table and table == cc.REACHABLE_PLANS, table
    assert h16 == {1, 2, 3, 4, 5}, h16
