"""An fp64 restatement of the CNN ops of include/vocr.h (3x3 / pad-1 conv forward, data, weight and bias gradient; BatchNorm2d training
and eval statistics, BatchNorm + ReLU apply and backward; FractionalMaxPool2d 2x2; ReLU + MaxPool2d(2,2)), the yardstick of
tests/test_cnn_fp64_gpu.py and tests/test_cnn_seams_gpu.py.  Plain torch, on the device of its inputs: a conv is an F.unfold plus a float64 matmul, image by image, so
the same code serves the CPU test and the GPU test (where torch has no float64 convolution of its own to lean on).

The bars are fixed constants with their reasoning below; none is derived from a kernel's output.  tests/test_cnn_ref_cpu.py holds them
to having teeth: every mutant (a wrong variant of an fp32 computation, `MUTANTS`) misses its bar by at least 10x."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                       # unit roundoff of fp32

# ---- conv bars: |k - ref| <= C * U * s, s = (|W| * |X|) + |bias| the same conv on absolute values (the scale an fp32 sum of products
# cannot resolve below).  A plain fp32 fmaf chain over K terms lands at ~1-6 U s for K up to 4096 (round-off grows like sqrt(K) in
# practice); 8 leaves room for a kernel's split and tree order.  Minimal filtering adds the rounding of the transformed operands: F(2,3)
# transforms are sums of <= 3 terms with weights <= 1 (x2 16); F(4,3) along the row uses points 0, +-1, +-2 whose input / output
# transforms carry weights up to 5 / 8 and the filter transform 1/4 .. 1/24: each product then carries ~4x the relative error of a
# direct product (x8 64).  The weight gradient of the row-pair F(3,2) kernel sums per-split slabs in a fixed tree (x 16).  fp16-operand
# kernels are held against the fp64 conv of the fp16-ROUNDED operands: products of fp16 numbers are exact in fp32, so only the fp32
# accumulation remains (8).  The one-input-channel kernels run one chain of 9 products and the bias: its worst case, 10.
CONV_C = {"direct": 8.0, "f23": 16.0, "f43": 64.0, "wgrad": 16.0, "f16": 8.0, "c1": 10.0}

# ---- BatchNorm bars.  Statistics: the kernels sum in double and round once to fp32, so mean and invstd sit within half an fp32 ulp of
# the fp64 value, plus the double-precision cancellation of var = E[y^2] - mean^2, ~SUM_DEPTH eps64 (1 + mean^2 / var) relative, which
# reaches an fp32 ulp only where |mean| / sigma approaches 1e4.  STAT_ULPS = 1 ulp (2 U) of headroom over the rounding itself.
STAT_ULPS = 1.0
SUM_DEPTH = 64.0
EPS64 = 2.0 ** -53


def _f(t):
    return t.double()


# ------------------------------------------------------------------------------------------------------------------------------ conv
def conv3x3(x, w, bias=None, absolute=False):
    """y[n][co][h][w] = sum_{ci,kh,kw} w[co][ci][kh][kw] x[n][ci][h+kh-1][w+kw-1] (+ bias[co]), fp64; `absolute`: |w| * |x| + |bias|."""
    x, w = _f(x), _f(w)
    if absolute:
        x, w = x.abs(), w.abs()
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    wm = w.reshape(cout, cin * 9)
    y = torch.empty(n, cout, h, wd, dtype=torch.float64, device=x.device)
    for i in range(n):
        y[i] = (wm @ F.unfold(x[i:i + 1], 3, padding=1)[0]).view(cout, h, wd)
    if bias is not None:
        b = _f(bias).abs() if absolute else _f(bias)
        y += b.view(1, -1, 1, 1)
    return y


def conv3x3_dgrad(dy, w, absolute=False):
    """dx = the conv of dy with the flipped, transposed filter (the data gradient of conv3x3)."""
    return conv3x3(dy, _f(w).transpose(0, 1).flip(2, 3), absolute=absolute)


def conv3x3_wgrad(x, dy, absolute=False):
    """dw[co][ci][kh][kw] = sum over n, pixels of dy[n][co][p] x[n][ci][p + (kh - 1, kw - 1)], fp64."""
    x, dy = _f(x), _f(dy)
    if absolute:
        x, dy = x.abs(), dy.abs()
    n, cin, h, wd = x.shape
    cout = dy.shape[1]
    dw = torch.zeros(cout, cin * 9, dtype=torch.float64, device=x.device)
    for i in range(n):
        dw += dy[i].reshape(cout, h * wd) @ F.unfold(x[i:i + 1], 3, padding=1)[0].t()
    return dw.view(cout, cin, 3, 3)


def conv_bar(family, s):
    return CONV_C[family] * U * s


# ---- minimal filtering at a tiny K.  The constants above measure a kernel's error against s, the products IN an output's support.  A
# minimal-filtering kernel forms each output from transformed points of a whole tile - F(m,3): the m + 2 input columns of the output's
# column group; the row-pair weight gradient: the 2 x 2 gradient pixels and 4 x 4 inputs of a block - and the tile's other values cancel
# only in exact arithmetic: its rounding error scales with the tile, |e| <~ c U (largest tap of the filter row) (sum of |x| over the tile).
# Summed over many products the two scales agree within a small factor (what x2 / x8 above stand for); an output that sums fewer
# products than ONE K step of the kernels (a half-chunk of 4 input channels x 9 taps = 36) can have a support of small values beside
# large neighbours, and an honest fp32 transform then misses C U s (tests/test_cnn_ref_cpu.py: 7.6x at 1 x 1 x 1 x 32 -> 132, F(4,3)).
# Below TINY_K the same constants therefore apply to the scale of the tile, s_win >= s elementwise.
TINY_K = 36


def _windows(t, size, step, dims=(3,)):
    """sum of |t| over windows of `size` every `step` along dims (t already padded)"""
    t = t.abs().double()
    for d in dims:
        t = t.unfold(d, size, step)
    return t.sum(tuple(range(-len(dims), 0)))


def conv3x3_window(x, w, bias, m):
    """s_win of an F(m,3) row transform (m = 2, 4): sum over (ci, kh) of the largest |tap| of the filter row x the sum of |x| over the
    m + 2 columns m t - 1 .. m t + m of the output's column group t, + |bias|"""
    x, w = _f(x), _f(w)
    n, cin, h, wd = x.shape
    t = (wd + m - 1) // m
    win = _windows(F.pad(x, (1, m * t + 1 - wd, 1, 1)), m + 2, m)                       # [n][ci][h + 2][t]
    gmax = w.abs().amax(-1)                                                            # [co][ci][kh]
    s = torch.zeros(n, w.shape[0], h, t, dtype=torch.float64, device=x.device)
    for kh in range(3):
        s += torch.einsum("mk,nkht->nmht", gmax[:, :, kh], win[:, :, kh:kh + h])
    s = s.repeat_interleave(m, 3)[..., :wd]
    return s if bias is None else s + _f(bias).abs().view(1, -1, 1, 1)


def conv3x3_wgrad_window(x, dy):
    """s_win of the row-pair weight gradient: per (co, ci), the sum over blocks of (sum of |dy| over the block's 2 x 2 pixels) x (sum of
    |x| over its 4 x 4 inputs, rows 2r - 1 .. 2r + 2 and columns 2p - 1 .. 2p + 2); the same for all nine taps"""
    n, cin, h, wd = x.shape
    h2, w2 = (h + 1) // 2, (wd + 1) // 2
    xs = _windows(F.pad(_f(x), (1, 2 * w2 + 1 - wd, 1, 2 * h2 + 1 - h)), 4, 2, (2, 3))
    ds = _windows(F.pad(_f(dy), (0, 2 * w2 - wd, 0, 2 * h2 - h)), 2, 2, (2, 3))
    return torch.einsum("nohw,nihw->oi", ds, xs)[:, :, None, None].expand(-1, -1, 3, 3)


def ratio(got, ref, bar):
    """max over elements of |got - ref| / bar (bar > 0 elementwise)."""
    return float(((got.double().to(ref.device) - ref).abs() / bar.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------------------------------ BatchNorm
def bn_stats(y, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, mutant=None):
    """Training statistics of y [n][c][h][w] in fp64: (mean, invstd, biased var, running_mean', running_var').  running_var takes the
    UNBIASED variance (the biased one at a count of 1), running stats move by `momentum`.
    mutants: "last_vec" (the last 4 elements of the channel - the last vector of the last chunk - skipped), "biased_rv" (running_var
    from the biased variance), "eps_out" (eps outside the square root)."""
    yd = _f(y).transpose(0, 1).reshape(y.shape[1], -1)
    if mutant == "last_vec":
        yd = yd[:, :-4]
    cnt = yd.shape[1]
    mean = yd.mean(1)
    var = ((yd - mean[:, None]) ** 2).mean(1)
    invstd = 1.0 / (var.sqrt() + eps) if mutant == "eps_out" else 1.0 / (var + eps).sqrt()
    unb = var * cnt / (cnt - 1) if (cnt > 1 and mutant != "biased_rv") else var
    rm = rv = None
    if running_mean is not None:
        rm = (1 - momentum) * _f(running_mean) + momentum * mean
    if running_var is not None:
        rv = (1 - momentum) * _f(running_var) + momentum * unb
    return mean, invstd, var, rm, rv


def bn_stat_bars(mean, var, invstd, eps=1e-5):
    """(bar of mean, RELATIVE bar of invstd, ABSOLUTE bar of the biased var) per channel: STAT_ULPS fp32 ulps over the final rounding of
    mean and invstd, and the double-precision cancellation of E[y^2] - mean^2 (SUM_DEPTH eps64 (var + mean^2) absolute)."""
    e_var = SUM_DEPTH * EPS64 * (var + mean * mean)
    e_mean = (1.0 + 2 * STAT_ULPS) * U * mean.abs() + SUM_DEPTH * EPS64 * var.sqrt()
    e_is_rel = (1.0 + 2 * STAT_ULPS) * U + 0.5 * e_var / (var + eps)
    return e_mean, e_is_rel, e_var


def running_bars(rm0, rv0, mean, var_unb, e_mean, e_var, momentum, count):
    """bars of the fp32 running-stat update (1 - m) r + m v: three fp32 roundings of each term + the statistic's own error."""
    brm = 3 * U * ((1 - momentum) * _f(rm0).abs() + momentum * mean.abs()) + momentum * e_mean + 1e-30
    brv = 3 * U * ((1 - momentum) * _f(rv0).abs() + momentum * var_unb.abs()) + momentum * (e_var * count / max(count - 1, 1) + 2 * U * var_unb) + 1e-30
    return brm, brv


def _bc(v, like):
    return v.view(1, -1, *([1] * (like.dim() - 2)))


def bn_relu_pre(y, mean, invstd, gamma, beta):
    """the pre-activation (y - mean) invstd gamma + beta, fp64."""
    return (_f(y) - _bc(mean, y)) * _bc(invstd, y) * _bc(_f(gamma), y) + _bc(_f(beta), y)


def bn_apply_bar(y, mean, invstd, gamma, beta, e_mean, e_is_rel):
    """bar of out = relu((y - m32) is32 gamma + beta) in fp32: the fp32 rounding of mean (e_mean) and invstd (e_is_rel) - at |mean| /
    sigma = 1e4 that alone moves xhat by ~3e-4, the fp32 design - and four fp32 roundings (subtract, two products, add)."""
    yd, g, b = _f(y), _bc(_f(gamma).abs(), y), _bc(_f(beta).abs(), y)
    d = (yd - _bc(mean, y)).abs()
    inv = _bc(invstd, y)
    e_xhat = inv * (_bc(e_mean, y) + d * (_bc(e_is_rel, y) + 3 * U))
    return g * e_xhat + 2 * U * (g * d * inv + b) + 1e-30, e_xhat


def bn_relu_bwd(da, y, mask, mean, invstd, gamma):
    """training-mode BatchNorm + ReLU backward in fp64 with the ReLU decisions `mask` (the kernel's own forward: out > 0):
    (dy, dgamma, dbeta); the conv-bias gradient sum(dy) is 0 in exact arithmetic."""
    dz = _f(da) * mask.to(torch.float64)
    cnt = dz.numel() // dz.shape[1]
    xhat = (_f(y) - _bc(mean, y)) * _bc(invstd, y)
    red = [0] + list(range(2, dz.dim()))
    dbeta = dz.sum(red)
    dgamma = (dz * xhat).sum(red)
    dy = _bc(_f(gamma) * invstd, y) * (dz - _bc(dbeta / cnt, y) - xhat * _bc(dgamma / cnt, y))
    return dy, dgamma, dbeta


def bn_bwd_bars(da, y, mask, mean, invstd, gamma, dgamma, dbeta, e_xhat):
    """bars of (dy, dgamma, dbeta) for the fp32 backward whose xhat carries e_xhat (bn_apply_bar) and whose sums add the (up to 4)
    elements of one vector load in fp32 and carry the rest in double (bn_pool.hip): dbeta: 3 U per summed term + one rounding;
    dgamma: sum |dz| e_xhat + 5 U per product term + one rounding; dy: the propagated errors + five fp32 roundings of its terms."""
    dz = (_f(da) * mask.to(torch.float64)).abs()
    cnt = dz.numel() // dz.shape[1]
    red = [0] + list(range(2, dz.dim()))
    xhat = ((_f(y) - _bc(mean, y)) * _bc(invstd, y)).abs()
    b_dbeta = 2 * U * dbeta.abs() + 3 * U * dz.sum(red) + 1e-30
    b_dgamma = (dz * (e_xhat + 5 * U * xhat)).sum(red) + 2 * U * dgamma.abs() + 1e-30
    gs = _bc(_f(gamma).abs() * invstd, y)
    terms = dz + _bc(dbeta.abs() / cnt, y) + xhat * _bc(dgamma.abs() / cnt, y)
    b_dy = gs * (5 * U * terms + _bc(b_dbeta / cnt, y) + e_xhat * _bc(dgamma.abs() / cnt, y) + xhat * _bc(b_dgamma / cnt, y)) + 1e-30
    return b_dy, b_dgamma, b_dbeta


def xhat_sum_bound(mean, invstd, count):
    """the bound on |xhat_sum| that conv_bias_grad_bar is built from"""
    return count * (U * mean.abs() + SUM_DEPTH * EPS64 * mean.abs()) * invstd + SUM_DEPTH * EPS64 * count ** 0.5


def conv_bias_grad_bar(mean, invstd, gamma, dgamma, count):
    """The conv-bias gradient of a batch-statistics BatchNorm is 0 in exact arithmetic; the kernels return -gamma invstd (dgamma / count)
    xhat_sum, where xhat_sum = count (mean - m32) invstd is the rounding residue of the fp32 mean (|mean - m32| <= U |mean|, + the
    double sum's own error).  The bar is that bound, twice over."""
    xs = xhat_sum_bound(mean, invstd, count)
    return 2 * (_f(gamma).abs() * invstd * dgamma.abs() / count * xs) + 4 * U * dgamma.abs() / count + 1e-30


# --------------------------------------------------------------------------------------------------------------------------- pooling
def fracpool_starts(u, in_size, out_size, arith=np.float32):
    """ATen's fractional_max_pool2d window starts: alpha = (in - 2) / (out - 1), start(i) = int((i + u) alpha) - int(u alpha), the last
    window at in - 2; in float32 arithmetic (oracle/vista_oracle.py:fracpool_intervals).  arith=np.float64: the "fp64 window" mutant."""
    if arith is np.float32:
        from oracle.vista_oracle import fracpool_intervals
        return fracpool_intervals(u, in_size, out_size)
    seq = np.zeros(out_size, dtype=np.int64)
    uu = np.float64(np.float32(u))
    if out_size > 1:
        alpha = np.float64(in_size - 2) / np.float64(out_size - 1)
        for i in range(out_size - 1):
            seq[i] = int((np.float64(i) + uu) * alpha) - int(uu * alpha)
    seq[out_size - 1] = in_size - 2
    return seq


def fracpool2x2(x, samples, oh, ow, arith=np.float32):
    """FractionalMaxPool2d(2) with explicit samples [n][c][2] = (u_w, u_h): (out, idx = flat h * W + w of the first maximum in
    row-major window order), computed on x's device.  ATen's rule, `val > max || isnan(val)`: a NaN takes the window (the last one of
    several), index included; a window of four -inf keeps its first pixel."""
    n, c, h, w = x.shape
    s = samples.detach().cpu().numpy()
    sw = torch.tensor(np.stack([[fracpool_starts(s[i, j, 0], w, ow, arith) for j in range(c)] for i in range(n)]), device=x.device)
    sh = torch.tensor(np.stack([[fracpool_starts(s[i, j, 1], h, oh, arith) for j in range(c)] for i in range(n)]), device=x.device)
    flat = x.reshape(n, c, h * w)
    best = bidx = None
    for dh in (0, 1):
        for dw in (0, 1):
            ii = (sh[:, :, :, None] + dh) * w + (sw[:, :, None, :] + dw)
            v = torch.gather(flat, 2, ii.reshape(n, c, -1)).view(n, c, oh, ow)
            if best is None:
                best, bidx = v, ii
            else:
                take = (v > best) | torch.isnan(v)   # the first maximum wins; a NaN always does
                best, bidx = torch.where(take, v, best), torch.where(take, ii, bidx)
    return best, bidx


def pool_scatter(dout, idx, h, w):
    """dx of a pooling layer: dout added at its winners' flat indices, fp64 (exact for the <= 4 contributions a pixel receives)."""
    n, c = dout.shape[:2]
    dx = torch.zeros(n, c, h * w, dtype=torch.float64, device=dout.device)
    dx.scatter_add_(2, idx.reshape(n, c, -1).long(), _f(dout).reshape(n, c, -1))
    return dx.view(n, c, h, w)


def pool_bwd_bar(dout, idx, h, w):
    """bar of an fp32 pooling gradient against pool_scatter: exact where a pixel takes one window's gradient, one fp32 rounding per
    added term where it takes up to four."""
    n, c = dout.shape[:2]
    cnt = torch.zeros(n, c, h * w, dtype=torch.float64, device=dout.device)
    cnt.scatter_add_(2, idx.reshape(n, c, -1).long(), torch.ones_like(dout, dtype=torch.float64).reshape(n, c, -1))
    a = pool_scatter(dout.abs(), idx, h, w)
    return torch.where(cnt.view(n, c, h, w) > 1, 3 * U * a, torch.zeros_like(a))


def relu_maxpool2(x):
    """ReLU + MaxPool2d(2, 2): (out, idx = flat h * W + w of the first maximum), the odd last row / column dropped."""
    n, c, h, w = x.shape
    oh, ow = h // 2, w // 2
    r = torch.relu(x[:, :, :2 * oh, :2 * ow])
    best = bidx = None
    for dh in (0, 1):
        for dw in (0, 1):
            v = r[:, :, dh::2, dw::2]
            ii = (torch.arange(oh, device=x.device)[:, None] * 2 + dh) * w + torch.arange(ow, device=x.device)[None, :] * 2 + dw
            ii = ii.expand_as(v)
            if best is None:
                best, bidx = v, ii
            else:
                take = v > best
                best, bidx = torch.where(take, v, best), torch.where(take, ii, bidx)
    return best, bidx


# --------------------------------------------------------------------------------------------------------------------------- mutants
MUTANTS = ("tap", "last4_cin", "tail_piece", "wgrad_slab", "last_vec", "biased_rv", "eps_out", "fp64_windows",
           # the seam errors of tests/cnn_cases.py's tables (tests/test_cnn_seams_gpu.py)
           "odd_last_col", "gap_slot", "cin_mod4", "pair_lower_row", "last_slab", "f16_pad")
SEAM_CONV_MUTANTS = ("odd_last_col", "gap_slot", "cin_mod4")
SEAM_WGRAD_MUTANTS = ("pair_lower_row", "last_slab", "f16_pad")


def _next_row_first_col(x):
    """[n][c][h]: for every row of the (n, h) stream of a channel, column 0 of the row that follows it in memory (the last row of an image
    is followed by the first of the next image, the last image by zeros)"""
    n, c, h, _ = x.shape
    col = x[:, :, :, 0].transpose(0, 1).reshape(c, n * h)
    nxt = torch.cat([col[:, 1:], torch.zeros(c, 1, dtype=x.dtype)], 1)
    return nxt.view(c, n, h).transpose(0, 1)


def conv_mutant(x, w, bias, mutant):
    """an fp32 conv (CPU) that is wrong on purpose: "tap" drops tap (1, 2) of the pair (co, ci) = (1, 2); "last4_cin" drops the last 4
    input channels; "tail_piece" zeroes one tail piece (32 output channels x 8 pixels at the end of the last image's last row).
    The seams: "odd_last_col" leaves out the last column of a row of odd width (the half-filled last column group); "gap_slot" lets the
    column right of a row's last one - the zero padding the gap slot of the slot stream stands for - read the first column of the next
    row of the stream; "cin_mod4" drops the last Cin % 4 input channels (the partial half-chunk)."""
    w = w.clone()
    if mutant == "tap":
        w[1, 2, 1, 2] = 0
    elif mutant == "last4_cin":
        w[:, -4:] = 0
    elif mutant == "cin_mod4" and w.shape[1] % 4:
        w[:, -(w.shape[1] % 4):] = 0
    b = None if bias is None else bias.float()
    if mutant == "gap_slot":
        xp = F.pad(x.float(), (1, 1, 1, 1))
        xp[:, :, 1:-1, -1] = _next_row_first_col(x.float())
        return F.conv2d(xp, w.float(), b)
    y = F.conv2d(x.float(), w.float(), b, padding=1)
    if mutant == "tail_piece":
        y[-1, :32, -1, -8:] = 0
    elif mutant == "odd_last_col" and x.shape[3] % 2:
        y[..., -1] = 0 if b is None else b.view(1, -1, 1)
    return y


def wgrad_mutant(x, dy, slabs=16, mutant="wgrad_slab"):
    """an fp32 weight gradient that is wrong on purpose.  "wgrad_slab": one of `slabs` split slabs (a run of rows of the (n, h) stream)
    dropped, the last one; "last_slab": the same at a kernel's own split count - `slabs` may exceed the rows, at least one row goes;
    "pair_lower_row": with an odd H the lower row of every image's last row pair, which lies outside the image, is counted - it reads
    the first row of what follows in memory (the next image; the first image after the last); "f16_pad": the first padded element of
    the first row of the channel-major fp16 copy of x (vocr_f32_to_f16_layouts: the right halo of that row) holds 1 instead of 0."""
    n, cin, h, wd = x.shape
    x, dy = x.float(), dy.float()
    shape = (dy.shape[1], cin, 3, 3)
    if mutant == "pair_lower_row":
        if h % 2 == 0:
            return torch.nn.grad.conv2d_weight(x, shape, dy, padding=1)
        below = lambda t: torch.cat([t, torch.roll(t, -1, 0)[:, :, :1]], 2)
        return torch.nn.grad.conv2d_weight(below(x), shape, below(dy), padding=1)
    if mutant == "f16_pad":
        xe, dye = F.pad(x, (0, 1)), F.pad(dy, (0, 1))
        xe[0, 0, 0, wd] = 1.0
        return torch.nn.grad.conv2d_weight(xe, shape, dye, padding=1)
    rows = n * h
    cut = rows - (max(1, rows // slabs) if mutant == "last_slab" else rows // slabs)
    keep = torch.zeros(n, 1, h, 1)
    keep.view(-1)[:cut] = 1
    return torch.nn.grad.conv2d_weight(x, shape, dy * keep, padding=1)


# ------------------------------------------------------------------------------------- honest fp32 minimal filtering (CPU, for the bars)
_BT4 = ((4, 0, -5, 0, 1, 0), (0, -4, -4, 1, 1, 0), (0, 4, -4, -1, 1, 0), (0, -2, -1, 2, 1, 0), (0, 2, -1, -2, 1, 0), (0, 4, 0, -5, 0, 1))
_G4 = ((1 / 4, 0, 0), (-1 / 6, -1 / 6, -1 / 6), (-1 / 6, 1 / 6, -1 / 6), (1 / 24, 1 / 12, 1 / 6), (1 / 24, -1 / 12, 1 / 6), (0, 0, 1))
_AT4 = ((1, 1, 1, 1, 1, 0), (0, 1, -1, 2, -2, 0), (0, 1, 1, 4, 4, 0), (0, 1, -1, 8, -8, 1))
_BT2 = ((1, 0, -1, 0), (0, 1, 1, 0), (0, -1, 1, 0), (0, 1, 0, -1))
_G2 = ((1, 0, 0), (.5, .5, .5), (.5, -.5, .5), (0, 0, 1))
_AT2 = ((1, 1, 1, 0), (0, 1, -1, -1))
_WA = ((1, 0), (.5, .5), (.5, -.5), (0, 1))                 # weight gradient F(3,2): the gradient pair's four points
_WBT = ((1, 0, -1, 0), (0, 1, 1, 0), (0, -1, 1, 0), (0, -1, 0, 1))
_WGT = ((1, 1, 1, 0), (0, 1, -1, 0), (0, 1, 1, 1))


def _mv(mat, v):
    """rows of `mat` applied along the last dim of v, term by term in v's precision"""
    out = []
    for row in mat:
        acc = None
        for c, val in zip(row, v.unbind(-1)):
            if c:
                acc = val * c if acc is None else acc + val * c
        out.append(acc)
    return torch.stack(out, -1)


def _mv2(mat, v):
    """`mat` along the last two dims of v"""
    return _mv(mat, _mv(mat, v).transpose(-1, -2)).transpose(-1, -2)


def wino_conv_fp32(x, w, bias, m):
    """the 3x3 convolution by F(m,3) along the row (m = 2, 4; points 0, +-1, (+-2,) infinity) in plain fp32 on the CPU: what an honest
    minimal-filtering kernel computes, in one of its possible orders"""
    bt, g, at = (_BT4, _G4, _AT4) if m == 4 else (_BT2, _G2, _AT2)
    x, w = x.float(), w.float()
    n, cin, h, wd = x.shape
    t = (wd + m - 1) // m
    v = _mv(bt, F.pad(x, (1, m * t + 1 - wd, 1, 1)).unfold(3, m + 2, m))                # [n][ci][h + 2][t][points]
    u = _mv(g, w)                                                                      # [co][ci][kh][points]
    acc = torch.zeros(n, w.shape[0], h, t, len(bt))
    for ci in range(cin):
        for kh in range(3):
            acc = acc + u[None, :, ci, kh, None, None, :] * v[:, None, ci, kh:kh + h]
    y = _mv(at, acc).reshape(n, w.shape[0], h, t * m)[..., :wd]
    return y if bias is None else y + bias.float().view(1, -1, 1, 1)


def wgrad_rowpair_fp32(x, dy):
    """the weight gradient by F(3,2) along the row and across row pairs, in plain fp32 on the CPU"""
    x, dy = x.float(), dy.float()
    n, cin, h, wd = x.shape
    h2, w2 = (h + 1) // 2, (wd + 1) // 2
    xt = F.pad(x, (1, 2 * w2 + 1 - wd, 1, 2 * h2 + 1 - h)).unfold(2, 4, 2).unfold(3, 4, 2)
    dt = F.pad(dy, (0, 2 * w2 - wd, 0, 2 * h2 - h)).unfold(2, 2, 2).unfold(3, 2, 2)
    return _mv2(_WGT, torch.einsum("nohwrc,nihwrc->oirc", _mv2(_WA, dt), _mv2(_WBT, xt)))
