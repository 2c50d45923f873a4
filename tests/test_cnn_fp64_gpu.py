"""GPU: every conv, BatchNorm and pooling kernel variant against the fp64 restatement of tests/cnn_ref.py, computed on the GPU with
torch's own float64 ops.  Convs at every layer of the BASELINE workloads (configs[1] 32 x 30x600, configs[3] 32 x 30x1178, the reference's
speed_test 64 x 30x300, configs[4]'s fp16 layers at 32 x 60x1200) plus edge shapes for the minimal-filtering launch plans those miss; the
BatchNorm entry points fed a chosen y; the pooling gradient in all four plane regimes; the layer ops at the model's shapes.
`-s` prints a table of error / bar per case."""
import math

import pytest
import torch

from tests import cnn_ref as cr

pytestmark = pytest.mark.gpu

_ROWS = []


def _row(case, what, r):
    _ROWS.append((case, what, r))
    assert r <= 1.0, "%s %s: error / bar = %.3f" % (case, what, r)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    if _ROWS:
        print("\n%-44s %-22s %10s" % ("case", "quantity", "err / bar"))
        for case, what, r in _ROWS:
            print("%-44s %-22s %10.4f" % (case, what, r))


@pytest.fixture(scope="module")
def dev():
    from vistaocr_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _rand(shape, seed, scale=1.0, dev=None):
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(shape, generator=g) * 2 - 1) * scale
    return t.to(dev) if dev is not None else t


def _layers(B, W, himg=30):
    """(n, cin, h, w, cout) of every conv of the model at batch B and line width W (vistaocr_amd/model.py:_CONV_SLOTS)."""
    h, w, out = himg, W, []
    for st in [(1, 64), (64, 64), "pool", (64, 128), (128, 128), "pool", (128, 256), (256, 256), (256, 256)]:
        if st == "pool":
            h, w = math.floor(h * 0.5), math.floor(w * 0.7)
            continue
        out.append((B, st[0], h, w, st[1]))
    return out


_BASE = {"c1": (32, 600), "c4": (32, 1178), "speed_test": (64, 300)}
_BASE_LAYERS = sorted({l for B, W in _BASE.values() for l in _layers(B, W)})
# launch plans of vocr_conv3x3_wino_fwd (include/vocr.h) the BASELINE layers miss, each at the smallest shape found that takes it:
# F(2,3) with 64 channels with and without tail pieces (Cout < 64), the 4-wave 64-channel and the 8-wave 128-channel F(4,3) kernels.
# Not reachable in the shipped library, hence not here: 2 / 18 (F(2,3) above 64 channels: F(4,3) takes every Cout >= 64), 9 / 10
# (tensors of 2^29 elements or more, which ops.conv3x3_forward sends to the direct kernel), 19 / 21 / 22 (the 4-wave 64-channel and the
# 8-wave kernels run only while their tiles fit one round, so they never cut a tail).
_EDGE = {1: (1, 8, 3, 33, 16), 3: (1, 64, 3, 33, 64), 6: (32, 32, 30, 64, 256), 17: (4, 8, 30, 600, 16)}
_F43 = {3, 4, 5, 6, 7, 8}


def _family(plan):
    return "f43" if (plan & 15) in _F43 else "f23"


def test_fp64_reference_on_the_gpu_is_the_cpu_reference(dev):
    n, cin, h, w, cout = 2, 8, 5, 19, 12
    x, wt, b, dy = _rand((n, cin, h, w), 1), _rand((cout, cin, 3, 3), 2), _rand((cout,), 3), _rand((n, cout, h, w), 4)
    for f in (lambda *a: cr.conv3x3(a[0], a[1], a[2]), lambda *a: cr.conv3x3_dgrad(a[3], a[1]), lambda *a: cr.conv3x3_wgrad(a[0], a[3])):
        cpu = f(x, wt, b, dy)
        gpu = f(x.to(dev), wt.to(dev), b.to(dev), dy.to(dev)).cpu()
        assert float((cpu - gpu).abs().max()) <= 1e-12 * float(cpu.abs().max())


def test_the_plans_cover_every_baseline_launch(dev):
    from vistaocr_amd import _lib
    lib = _lib.load()
    seen = set()
    for n, cin, h, w, cout in _BASE_LAYERS:
        seen.add(lib.vocr_conv3x3_wino_plan(n, cin, h, w, cout))
        if cin > 1:
            seen.add(lib.vocr_conv3x3_wino_plan(n, cout, h, w, cin))
    tested = set(seen) | {lib.vocr_conv3x3_wino_plan(*s) for s in _EDGE.values()}
    for p, s in _EDGE.items():
        assert lib.vocr_conv3x3_wino_plan(*s) == p, (p, s)
    print("\nplans of the BASELINE layers: %s; with the edge shapes: %s" % (sorted(seen), sorted(tested)))
    # the F(4,3) kernels the issue found unreached: x2_64 with and without tail pieces, w8_64, w4_128 with tail pieces
    assert {7, 23, 5, 20} <= seen and 0 not in seen
    assert tested >= seen | set(_EDGE)


def _check_conv(dev, n, cin, h, w, cout, tag, seed=0):
    from vistaocr_amd import ops, _lib
    lib = _lib.load()
    x, wt, b, dy = _rand((n, cin, h, w), seed + 1, 1.0, dev), _rand((cout, cin, 3, 3), seed + 2, 0.2, dev), _rand((cout,), seed + 3, 1.0, dev), \
        _rand((n, cout, h, w), seed + 4, 1.0, dev)
    case = "%s %s" % (tag, (n, cin, h, w, cout))
    pf, pd = ops.conv3x3_pack(wt)
    plan_f = lib.vocr_conv3x3_wino_plan(n, cin, h, w, cout)
    y = ops.conv3x3_forward(x, pf, b, cout)
    ref, s = cr.conv3x3(x, wt, b), cr.conv3x3(x, wt, b, absolute=True)
    _row(case, "fwd plan %d" % plan_f, cr.ratio(y, ref, cr.conv_bar(_family(plan_f), s)))
    del y, ref, s
    if cin == 1:
        y = ops.conv3x3_c1_forward(x, wt, b)
        _row(case, "fwd Cin=1", cr.ratio(y, cr.conv3x3(x, wt, b), cr.conv_bar("c1", cr.conv3x3(x, wt, b, absolute=True))))
        del y
    else:
        plan_d = lib.vocr_conv3x3_wino_plan(n, cout, h, w, cin)
        dx = ops.conv3x3_forward(dy, pd, None, cin)
        _row(case, "dgrad plan %d" % plan_d, cr.ratio(dx, cr.conv3x3_dgrad(dy, wt), cr.conv_bar(_family(plan_d), cr.conv3x3_dgrad(dy, wt, True))))
        del dx
    dw = ops.conv3x3_wgrad(x, dy)
    fam = "wgrad" if cin >= 4 else "direct"
    _row(case, "wgrad (%s)" % fam, cr.ratio(dw, cr.conv3x3_wgrad(x, dy), cr.conv_bar(fam, cr.conv3x3_wgrad(x, dy, True))))
    db = ops.channel_sum(dy)
    _row(case, "bias grad", cr.ratio(db, dy.double().sum((0, 2, 3)), cr.conv_bar("direct", dy.double().abs().sum((0, 2, 3)))))
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", _BASE_LAYERS, ids=lambda s: "x".join(map(str, s)))
def test_conv_baseline_layers_fp64(dev, shape):
    _check_conv(dev, *shape, tag="baseline")


@pytest.mark.parametrize("plan", sorted(_EDGE))
def test_conv_edge_plans_fp64(dev, plan):
    _check_conv(dev, *_EDGE[plan], tag="edge plan %d" % plan, seed=10 * plan)


_C5 = [(32, 16, 30, 600, 64), (32, 64, 30, 600, 64), (32, 64, 15, 420, 128), (32, 128, 15, 420, 128), (32, 128, 7, 294, 256), (32, 256, 7, 294, 256)]


def test_conv_f16_config5_layers_fp64(dev):
    """configs[4]'s fp16-operand layers at batch 32: the fp64 conv of the fp16-ROUNDED operands; every h16 plan id and wgrad_h16."""
    from vistaocr_amd import ops, _lib
    lib = _lib.load()
    plans = set()
    for i, (n, cin, h, w, cout) in enumerate(_C5):
        x, wt, b, dy = _rand((n, cin, h, w), 5 * i + 1, 1.0, dev), _rand((cout, cin, 3, 3), 5 * i + 2, 0.2, dev), _rand((cout,), 5 * i + 3, 1.0, dev), \
            _rand((n, cout, h, w), 5 * i + 4, 1.0, dev)
        xh, wh, dyh = x.half().double(), wt.half().double(), dy.half().double()
        case = "f16 %s" % ((n, cin, h, w, cout),)
        pf, pd = ops.conv3x3_pack_f16(wt)
        pfw, pdw = lib.vocr_conv3x3_h16_plan(n, cin, h, w, cout), lib.vocr_conv3x3_h16_plan(n, cout, h, w, cin)
        plans |= {pfw, pdw}
        y = ops.conv3x3_forward_f16(x, pf, b, cout)
        _row(case, "fwd h16 plan %d" % pfw, cr.ratio(y, cr.conv3x3(xh, wh, b), cr.conv_bar("f16", cr.conv3x3(xh, wh, b, absolute=True))))
        del y
        dx = ops.conv3x3_forward_f16(dy, pd, None, cin)
        _row(case, "dgrad h16 plan %d" % pdw, cr.ratio(dx, cr.conv3x3_dgrad(dyh, wh), cr.conv_bar("f16", cr.conv3x3_dgrad(dyh, wh, True))))
        del dx
        if ops.wgrad_f16_layouts_ok(cin, cout):
            x16p, dy16p = ops.f16_layouts(x, False, True)[1], ops.f16_layouts(dy, False, True)[1]
            dw = ops.conv3x3_wgrad(x, dy, f16=True, x16p=x16p, dy16p=dy16p)
            _row(case, "wgrad_h16", cr.ratio(dw, cr.conv3x3_wgrad(xh, dyh), cr.conv_bar("f16", cr.conv3x3_wgrad(xh, dyh, True))))
            del x16p, dy16p
        dw = ops.conv3x3_wgrad(x, dy, f16=True)                 # without the copies: the fp32 row-pair kernel on the exact operands
        _row(case, "wgrad (fp32 row pairs)", cr.ratio(dw, cr.conv3x3_wgrad(x, dy), cr.conv_bar("wgrad", cr.conv3x3_wgrad(x, dy, True))))
        torch.cuda.empty_cache()
    assert plans >= {1, 2, 4, 5}, plans


# ------------------------------------------------------------------------------------------------------------------------ BatchNorm
def _bn_call(dev, y, gamma, beta, rm, rv, nbt, eps=1e-5, mom=0.1, fused=True):
    from vistaocr_amd import _lib
    from vistaocr_amd._lib import call
    lib = _lib.load()
    n, c = y.shape[:2]
    hw = y[0, 0].numel()
    st = torch.cuda.current_stream().cuda_stream
    mean, invstd, xs = (torch.empty(c, device=dev) for _ in range(3))
    out = torch.empty(n, c, hw, device=dev)
    ws = torch.empty(lib.vocr_bn_workspace_bytes(n, c, hw) // 8 + 2, dtype=torch.float64, device=dev)
    if fused:
        call("vocr_bn_train_relu_apply", y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), n, c, hw, eps, mom, mean.data_ptr(),
             invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), xs.data_ptr(), ws.data_ptr(), st)
    else:
        call("vocr_bn_train_stats", y.data_ptr(), n, c, hw, eps, mom, mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(),
             nbt.data_ptr(), xs.data_ptr(), ws.data_ptr(), st)
        call("vocr_bn_relu_apply", y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
             n, c, hw, st)
    return mean, invstd, xs, out


def _bn_bwd_call(dev, da, y, mean, invstd, gamma, beta, xs):
    from vistaocr_amd import _lib
    from vistaocr_amd._lib import call
    lib = _lib.load()
    n, c = y.shape[:2]
    hw = y[0, 0].numel()
    dy = torch.empty(n, c, hw, device=dev)
    dg, db, dcb = (torch.empty(c, device=dev) for _ in range(3))
    ws = torch.empty(lib.vocr_bn_workspace_bytes(n, c, hw) // 8 + 2, dtype=torch.float64, device=dev)
    call("vocr_bn_relu_bwd", da.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), xs.data_ptr(),
         dy.data_ptr(), dg.data_ptr(), db.data_ptr(), dcb.data_ptr(), n, c, hw, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return dy, dg, db, dcb


def _check_bn(dev, case, y, gamma, beta, calls=1, fused=True):
    """y [n][c][hw] (a view, possibly misaligned): statistics, running statistics over `calls` successive calls, num_batches_tracked,
    the apply pass, the backward and the conv-bias gradient against fp64; ReLU decisions from the kernel's own forward."""
    n, c, hw = y.shape
    rm = _rand((c,), 90, 0.5, dev)
    rv = _rand((c,), 91, 0.5, dev) + 1.5
    nbt = torch.zeros(1, dtype=torch.int64, device=dev)
    rm64, rv64 = rm.double(), rv.double()
    for k in range(calls):
        rm0, rv0 = rm.double(), rv.double()
        mean_k, is_k, xs_k, out_k = _bn_call(dev, y, gamma, beta, rm, rv, nbt, fused=fused)
        mean, invstd, var, rm64, rv64 = cr.bn_stats(y, rm64, rv64)
        cnt = n * hw
        e_mean, e_is, e_var = cr.bn_stat_bars(mean, var, invstd)
        _row(case, "mean", cr.ratio(mean_k, mean, e_mean))
        _row(case, "invstd", cr.ratio(is_k, invstd, e_is * invstd))
        # the running statistics: each call's fp32 update from the kernel's own previous values, and the fp64 chain itself
        var_unb = var * cnt / (cnt - 1) if cnt > 1 else var
        brm, brv = cr.running_bars(rm0, rv0, mean, var_unb, e_mean, e_var, 0.1, cnt)
        _row(case, "running_mean (call %d)" % (k + 1), cr.ratio(rm, 0.9 * rm0 + 0.1 * mean, brm))
        _row(case, "running_var (call %d)" % (k + 1), cr.ratio(rv, 0.9 * rv0 + 0.1 * var_unb, brv))
    assert int(nbt.item()) == calls
    _row(case, "running_var chain", cr.ratio(rv, rv64, (6 * calls) * cr.U * rv64.abs() + 0.1 * calls * e_var + 1e-30))
    pre = cr.bn_relu_pre(y, mean, invstd, gamma, beta)
    bar, e_xhat = cr.bn_apply_bar(y, mean, invstd, gamma, beta, e_mean, e_is)
    mask = out_k > 0
    flips = mask != (pre > 0)
    if bool(flips.any()):                       # a decision that differs from fp64 must be a near-tie within the forward bar
        _row(case, "ReLU flips near-tie", float((pre[flips].abs() / bar[flips]).max()))
    _row(case, "apply", cr.ratio(out_k, torch.where(mask, pre, torch.zeros_like(pre)), bar))
    da = _rand((n, c, hw), 77, 1.0, dev)
    dy_k, dg_k, db_k, dcb_k = _bn_bwd_call(dev, da, y, mean_k, is_k, gamma, beta, xs_k)
    dy, dgamma, dbeta = cr.bn_relu_bwd(da, y, mask, mean, invstd, gamma)
    b_dy, b_dg, b_db = cr.bn_bwd_bars(da, y, mask, mean, invstd, gamma, dgamma, dbeta, e_xhat)
    _row(case, "bwd dy", cr.ratio(dy_k, dy, b_dy))
    _row(case, "bwd dgamma", cr.ratio(dg_k, dgamma, b_dg))
    _row(case, "bwd dbeta", cr.ratio(db_k, dbeta, b_db))
    _row(case, "conv-bias grad", cr.ratio(dcb_k, torch.zeros_like(dgamma), cr.conv_bias_grad_bar(mean, invstd, gamma, dgamma, n * hw)))
    return mean_k, is_k


def _bn_inputs(dev, n, c, hw, seed, offset=0.0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    y = ((torch.rand(n, c, hw, generator=g) * 2 - 1) * scale + offset).to(dev)
    gamma = (torch.rand(c, generator=g) * 0.6 + 0.7).to(dev)
    beta = ((torch.rand(c, generator=g) * 2 - 1) * 0.3).to(dev)
    return y, gamma, beta


# hw % 4 in {0, 1, 2, 3} (vector widths 4, 2, 1); 1, 2 and 36 chunks (16384 elements per chunk); the 512-chunk cap
@pytest.mark.parametrize("n,c,hw,what", [(2, 5, 72, "hw%4=0"), (3, 4, 37, "hw%4=1"), (2, 3, 38, "hw%4=2"), (2, 3, 39, "hw%4=3"),
                                         (2, 3, 12000, "2 chunks"), (32, 2, 18000, "36 chunks"), (64, 2, 140000, "512-chunk cap"),
                                         (1, 3, 1, "count 1")])
def test_bn_entry_points_fp64(dev, n, c, hw, what):
    y, gamma, beta = _bn_inputs(dev, n, c, hw, seed=hw + c, offset=0.3)
    for fused in (True, False):
        _check_bn(dev, "bn %s %s%s" % (what, (n, c, hw), "" if fused else " 3-launch"), y, gamma, beta, fused=fused)


def test_bn_misaligned_base_constant_channel_large_mean_and_running_stats(dev):
    n, c, hw = 4, 4, 300
    y, gamma, beta = _bn_inputs(dev, n, c, hw, seed=5)
    buf = torch.empty(n * c * hw + 1, device=dev)
    buf[1:] = y.reshape(-1)
    _check_bn(dev, "bn misaligned base", buf[1:].view(n, c, hw), gamma, beta)            # a 4-byte offset: scalar loads
    yc = y.clone()
    yc[:, 1] = 0.625                                                                     # a constant channel: var = 0
    yc[:, 2] = yc[:, 2] + 1e4                                                            # |mean| / sigma ~ 2e4
    _check_bn(dev, "bn constant / |mean|/sigma=1e4", yc, gamma, beta, calls=3)           # three successive calls


def test_bn_eval_mode(dev):
    from vistaocr_amd._lib import call
    c = 6
    rm = _rand((c,), 1, 2.0, dev)
    rv = _rand((c,), 2, 0.5, dev) + 1.0
    rv[0] = 0.0
    mean, invstd = torch.empty(c, device=dev), torch.empty(c, device=dev)
    call("vocr_bn_eval_stats", rm.data_ptr(), rv.data_ptr(), c, 1e-5, mean.data_ptr(), invstd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert torch.equal(mean, rm)
    ref = 1.0 / (rv.double() + 1e-5).sqrt()
    _row("bn eval", "invstd", cr.ratio(invstd, ref, 3 * cr.U * ref))


# --------------------------------------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize("h,w,what", [(15, 420, "LDS 8192"), (30, 600, "LDS 18432"), (30, 1178, "LDS 36864"), (30, 1300, "scatter")])
def test_fracpool_bwd_plane_regimes(dev, h, w, what):
    from vistaocr_amd import ops
    n, c = 3, 5
    oh, ow = math.floor(h * 0.5), math.floor(w * 0.7)
    x = _rand((n, c, h, w), h + w, 1.0, dev)
    u = torch.rand(n, c, 2, generator=torch.Generator().manual_seed(w)).to(dev)
    xg = x.clone().requires_grad_(True)
    out = ops.FracPoolFn.apply(xg, u, oh, ow)
    ref, idx = cr.fracpool2x2(x, u, oh, ow)
    assert torch.equal(out, ref)
    assert torch.equal(out.grad_fn.saved_tensors[0].long(), idx)
    dout = _rand((n, c, oh, ow), 3, 1.0, dev)
    out.backward(dout)
    _row("fracpool bwd %s %s" % (what, (h, w)), "dx (exact at single winners)",
         cr.ratio(xg.grad, cr.pool_scatter(dout, idx, h, w), cr.pool_bwd_bar(dout, idx, h, w)))


# ------------------------------------------------------------------------------------------------------------------------- layer ops
@pytest.mark.parametrize("n,cin,h,w,cout,f16,pooled", [(8, 64, 30, 600, 64, False, True), (8, 64, 30, 600, 64, False, False),
                                                       (8, 128, 15, 420, 128, False, True), (8, 256, 7, 294, 256, False, False),
                                                       (8, 64, 30, 600, 64, True, True), (8, 128, 7, 294, 256, True, False)])
def test_conv_bn_relu_layer_fp64(dev, n, cin, h, w, cout, f16, pooled):
    """ConvBnReluFn at the model's shapes: the conv output, the statistics, the (pooled) activation and every gradient against fp64;
    ReLU and pool-winner decisions taken from the kernel's own forward, each decision that differs from fp64 a near-tie."""
    from vistaocr_amd import ops
    case = "layer %s%s%s" % ((n, cin, h, w, cout), " fp16" if f16 else "", " pooled" if pooled else "")
    seed = cin + h
    x = _rand((n, cin, h, w), seed, 1.0, dev).relu()
    wt = _rand((cout, cin, 3, 3), seed + 1, 0.1, dev)
    b = _rand((cout,), seed + 2, 0.5, dev)
    gamma = _rand((cout,), seed + 3, 0.3, dev) + 1.0
    beta = _rand((cout,), seed + 4, 0.2, dev)
    leaf = [t.clone().requires_grad_(True) for t in (x, wt, b, gamma, beta)]
    rm, rv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
    oh, ow = (math.floor(h * 0.5), math.floor(w * 0.7)) if pooled else (0, 0)
    u = torch.rand(n, cout, 2, generator=torch.Generator().manual_seed(seed)).to(dev) if pooled else None
    out = ops.ConvBnReluFn.apply(leaf[0], leaf[1], leaf[2], leaf[3], leaf[4], rm, rv, True, 1e-5, 0.1, f16, u, oh, ow)
    _, y_k, mean_k, is_k, _, _, _, idx_k, _, xs_k, _ = out.grad_fn.saved_tensors
    xr, wr = (x.half().double(), wt.half().double()) if f16 else (x, wt)
    y64 = cr.conv3x3(xr, wr, b)
    _row(case, "conv out", cr.ratio(y_k, y64, cr.conv_bar("f16" if f16 else "f43", cr.conv3x3(xr, wr, b, absolute=True))))
    del y64
    # BatchNorm + ReLU (+ pool) on the kernel's own conv output
    mean, invstd, var, _, _ = cr.bn_stats(y_k)
    e_mean, e_is, _ = cr.bn_stat_bars(mean, var, invstd)
    _row(case, "mean", cr.ratio(mean_k, mean, e_mean))
    _row(case, "invstd", cr.ratio(is_k, invstd, e_is * invstd))
    pre = cr.bn_relu_pre(y_k, mean, invstd, gamma, beta)
    bar, e_xhat = cr.bn_apply_bar(y_k, mean, invstd, gamma, beta, e_mean, e_is)
    act = pre.relu()
    dout = _rand(tuple(out.shape), seed + 5, 1.0, dev)
    if pooled:
        flat = act.reshape(n, cout, -1)
        got = torch.gather(flat, 2, idx_k.reshape(n, cout, -1).long()).view_as(out)
        _row(case, "pooled out", cr.ratio(out, got, torch.gather(bar.reshape(n, cout, -1), 2, idx_k.reshape(n, cout, -1).long()).view_as(out)))
        best, _ = cr.fracpool2x2(act, u, oh, ow)
        gap = best - got                             # the kernel's winner is a near-tie of the fp64 maximum
        wb = 2 * bar.max()
        _row(case, "pool winner near-tie", float(gap.max() / wb))
        da = cr.pool_scatter(dout, idx_k, h, w)
        mask = cr.pool_scatter((out > 0).double(), idx_k, h, w) > 0
    else:
        _row(case, "activation", cr.ratio(out, torch.where(out > 0, pre, torch.zeros_like(pre)), bar))
        flips = (out > 0) != (pre > 0)
        if bool(flips.any()):
            _row(case, "ReLU flips near-tie", float((pre[flips].abs() / bar[flips]).max()))
        da, mask = dout, out > 0
    out.backward(dout)
    dy, dgamma, dbeta = cr.bn_relu_bwd(da, y_k, mask, mean, invstd, gamma)
    b_dy, b_dg, b_db = cr.bn_bwd_bars(da, y_k, mask, mean, invstd, gamma, dgamma, dbeta, e_xhat)
    _row(case, "dgamma", cr.ratio(leaf[3].grad, dgamma, b_dg))
    _row(case, "dbeta", cr.ratio(leaf[4].grad, dbeta, b_db))
    _row(case, "conv-bias grad", cr.ratio(leaf[2].grad, torch.zeros_like(dgamma), cr.conv_bias_grad_bar(mean, invstd, gamma, dgamma, n * h * w)))
    # dx, dw: the conv gradients of the fp64 dy, with dy's own bar carried through |W| / |x|
    fam = "f16" if f16 else "f43"
    dyr = dy.half().double() if f16 else dy
    dx64 = cr.conv3x3_dgrad(dyr, wr)
    bx = cr.conv_bar(fam, cr.conv3x3_dgrad(dyr, wr, True)) + cr.conv3x3_dgrad(b_dy, wr, True) * (2 if f16 else 1)
    if f16:                                          # the kernel rounds ITS dy to fp16: one fp16 rounding of each dy element
        bx = bx + cr.conv3x3_dgrad(dy.abs() * 2.0 ** -11, wr, True)
    _row(case, "dx", cr.ratio(leaf[0].grad, dx64, bx))
    del dx64, bx
    dw64 = cr.conv3x3_wgrad(x, dy)
    bw = cr.conv_bar("wgrad", cr.conv3x3_wgrad(x, dy, True)) + cr.conv3x3_wgrad(x, b_dy, True)
    if f16:                                          # the all-DMA fp16 weight gradient rounds x and dy to fp16
        bw = bw + cr.conv3x3_wgrad(x, dy, True) * 2.0 ** -10
    _row(case, "dw", cr.ratio(leaf[1].grad, dw64, bw))
    torch.cuda.empty_cache()


@pytest.mark.parametrize("f16", [False, True])
def test_conv_relu_pool_layer_fp64(dev, f16):
    """ConvReluPoolFn at configs[4]'s rapid_ds shape (32 x 1 x 60 x 1200 -> 16 channels): values against fp64 (max is 1-Lipschitz), the
    winners from the kernel's own forward, parameter gradients against fp64 through them."""
    from vistaocr_amd import ops
    n, h, w, cout = 32, 60, 1200, 16
    case = "rapid_ds %s%s" % ((n, 1, h, w, cout), " fp16" if f16 else "")
    x = _rand((n, 1, h, w), 1, 1.0, dev).abs()
    wt, b = _rand((cout, 1, 3, 3), 2, 0.3, dev), _rand((cout,), 3, 0.2, dev)
    leaf = [wt.clone().requires_grad_(True), b.clone().requires_grad_(True)]
    out = ops.ConvReluPoolFn.apply(x, leaf[0], leaf[1], f16)
    idx_k = out.grad_fn.saved_tensors[2]
    xr, wr = (x.half().double(), wt.half().double()) if f16 else (x, wt)
    y64 = cr.conv3x3(xr, wr, b)
    bar = cr.conv_bar("c1", cr.conv3x3(xr, wr, b, absolute=True))
    ref, _ = cr.relu_maxpool2(y64)
    bmax, _ = cr.relu_maxpool2(bar)
    _row(case, "out", cr.ratio(out, ref, bmax + 1e-30))
    got = torch.gather(y64.relu().reshape(n, cout, -1), 2, idx_k.reshape(n, cout, -1).long()).view_as(out)
    _row(case, "winner near-tie", float(((ref - got) / (2 * bmax + 1e-30)).max()))
    dout = _rand(tuple(out.shape), 4, 1.0, dev)
    out.backward(dout)
    dy = cr.pool_scatter(dout * (out > 0), idx_k, h, w)
    _row(case, "dw", cr.ratio(leaf[0].grad, cr.conv3x3_wgrad(x, dy), cr.conv_bar("direct", cr.conv3x3_wgrad(x, dy, True))))
    _row(case, "dbias", cr.ratio(leaf[1].grad, dy.sum((0, 2, 3)), cr.conv_bar("direct", dy.abs().sum((0, 2, 3)))))
