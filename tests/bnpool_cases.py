"""The case tables, the data and the host restatements of the BatchNorm / pooling seam suite (vistaocr_amd/csrc/bn_pool.hip: 14 entry
points and one support query).  tests/test_bnpool_seams_gpu.py runs every row through the C entry points in guarded memory;
tests/test_bnpool_cases_cpu.py holds the tables to reaching every branch named below, the references to torch's CPU ops bit for bit and
an honest fp32 restatement to the unchanged bars of tests/cnn_ref.py.  Importing this module needs no GPU and no library.

Every row is named for the branch it sits on.  The host plan of bn_pool.hip is restated here (vec_width, nchunk, chunk_len, plane_gx,
fused_bwd_supported), so that a row can say which path it takes and the CPU test can hold the table to its categories:

  dense BatchNorm   V = the widest load hw and the bases allow (4 / 2 / 1 floats; the backward takes the minimum over da, y and dy);
                    a channel's n hw elements are cut into nchunk = ceil(n hw / 16384) (<= 512) chunks of equal length rounded up to 4
                    (so 2 x 16384 + 1 elements are three chunks of 10924 / 10924 / 10921, never a chunk of one vector); a workgroup
                    walks its chunk in steps of 256 V, the backward's partial pass four steps at a time with dead slots in its last
                    iteration; the apply passes run gx = ceil(hw / V / 1024) (<= 64) workgroups per plane, the backward apply three
                    (V = 4) or four steps at a time with clamped indices.
  fractional pool   windows by ATen's float32 rule (cnn_ref.fracpool_starts), the last one pinned at in - 2.  The fused backward keeps
                    the pinned window out of its inverse maps; how it lies to its neighbour (start gap 1: overlapping, 2: abutting,
                    >= 3: apart, with pixels no window covers between them) is recorded per case, plane and axis (Frac.layouts).
                    vocr_fracpool2x2_bwd assembles planes of <= 8192 / 18432 / 36864 floats in LDS and scatters larger ones.
  ReLU + MaxPool    odd h / w drop a row / column, which the backward must leave at the zero its caller filled in.

Data, as in the GEMM suite: integers in [-8, 8] for every gradient (pooled gradients and their sums are exact in any order), N(0,1)
with a per-channel offset for y.  Fractional-pool planes come in variants (Frac.variants): "rand"; "const" (every window elects its
first pixel: the first-column / first-row maps alone); "ramp" (every window elects its last pixel: the second-column / second-row maps
alone, and every winner of the pinned windows lies in the last row / column); "planted" (maxima planted where a row of two windows
crosses a column of two windows, so that one pixel wins all four)."""
import numpy as np
import torch

from tests import cnn_ref as cr
from tests.cnn_cases import cover2, covers2                          # noqa: F401
from tests.gemm_ref import GUARD, SENTINEL, Padded                   # noqa: F401
from tests.guarded import POISON, Guarded, workspace                 # noqa: F401

CHUNK = 16384
SAMPLES = (0.0, 2.0 ** -24, 0.5, float(np.float32(1) / np.float32(3)), 0.999, 1.0 - 2.0 ** -23, 1.0 - 2.0 ** -24)
OPTIONAL = ("running_mean", "running_var", "num_batches_tracked", "xhat_sum", "dconv_bias")
MAX_PLANE = 300000                                                   # floats of the largest plane a row may have
LARGE = 20000                                                        # a "larger plane": at most about 30 rows above it


# ---------------------------------------------------------------------------------------------------- the host plan, restated
def vec_width(hw, *byte_offsets):
    m = 0
    for o in byte_offsets:
        m |= o
    if hw % 4 == 0 and m % 16 == 0:
        return 4
    if hw % 2 == 0 and m % 8 == 0:
        return 2
    return 1


def nchunk(per_channel):
    return max(1, min(512, -(-per_channel // CHUNK)))


def chunk_len(per_channel, nch):
    return (-(-per_channel // nch) + 3) // 4 * 4


def plane_gx(per_plane):
    return max(1, min(64, -(-per_plane // 1024)))


def workspace_bytes(n, c, hw):
    return c * nchunk(n * hw) * 2 * 8


def fused_bwd_supported(h, w, oh, ow):
    """vocr_bn_relu_fracpool2x2_bwd_supported: both alphas >= 1.01 in float32, rows of whole 4-pixel groups, the four inverse maps
    (2 w + 8 + 2 h ints) within 64 KB of LDS"""
    if h < 2 or w < 2 or oh < 2 or ow < 2 or oh > h - 1 or ow > w - 1:
        return False
    f = np.float32
    return bool(f(h - 2) / f(oh - 1) >= f(1.01) and f(w - 2) / f(ow - 1) >= f(1.01) and w % 4 == 0 and (2 * w + 8 + 2 * h) * 4 <= 64 * 1024)


def pool_regime(in_plane):
    return "lds8192" if in_plane <= 8192 else "lds18432" if in_plane <= 18432 else "lds36864" if in_plane <= 36864 else "scatter"


def ratio_out(h, w):
    """the model's output_ratio = (0.5, 0.7)"""
    return max(1, int(np.floor(h * 0.5))), max(1, int(np.floor(w * 0.7)))


# ------------------------------------------------------------------------------------------------------------ dense BatchNorm
class Bn(object):
    """(n, c, hw) with `off` = bytes by which y / out / da / dy sit behind a 16-byte boundary and `null` = the optional pointers passed
    as NULL (a NULL xhat_sum in the statistics call is NULL in the backward too: dconv_bias is then 0)."""

    def __init__(self, name, n, c, hw, off=None, null=()):
        self.name, self.n, self.c, self.hw, self.null = name, n, c, hw, tuple(null)
        self.off = dict(y=0, out=0, da=0, dy=0)
        self.off.update(off or {})
        assert all(o in (0, 4, 8) for o in self.off.values()) and n * c * hw <= MAX_PLANE * 3

    def __repr__(self):
        return "%s %dx%dx%d" % (self.name, self.n, self.c, self.hw)

    count = property(lambda s: s.n * s.hw)
    v_stats = property(lambda s: vec_width(s.hw, s.off["y"]))
    v_apply = property(lambda s: vec_width(s.hw, s.off["y"], s.off["out"]))
    v_bwd = property(lambda s: min(vec_width(s.hw, s.off["da"], s.off["y"]), vec_width(s.hw, s.off["dy"])))
    nchunk = property(lambda s: nchunk(s.count))
    per = property(lambda s: chunk_len(s.count, s.nchunk))

    def seam_inside_a_plane(self):
        return any((j * self.per) % self.hw for j in range(1, self.nchunk))


_V_OFF = {4: 0, 2: 8, 1: 4}                                          # the offset of y that forces V on a plane with hw % 4 == 0
# vectors per plane (n = 1: per channel too) on and either side of 256 k and 512 k (the apply grids of 1 and 2 workgroups), of 768 (one
# dead slot of the partial pass's four), 1024 and 4096 (its whole iterations)
_NV = (255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 4095, 4096, 4097)
NULL_SETS = ((), ("running_mean",), (), ("running_var",), (), ("num_batches_tracked",), (), ("xhat_sum",), (), ("dconv_bias",), OPTIONAL)


def _bn_cases():
    rows = []
    add = lambda *a, **k: rows.append(Bn(*a, **k))
    for hw in (8, 9, 10, 11):
        add("hw%%4=%d aligned" % (hw % 4), 2, 3, hw)
    add("hw%4=0 aligned n3", 3, 2, 24)
    for t in ("y", "out", "da", "dy"):
        for o in (4, 8):
            add("%s %d bytes off" % (t, o), 2, 2, 24, off={t: o})
            add("%s %d bytes off hw%%4=2" % (t, o), 3, 1, 26, off={t: o})
    for hw, c in ((1, 1), (2, 2), (3, 1), (4, 2), (5, 2)):            # one 256 V step crosses many planes: ChanWalk's while
        add("plane shorter than a step", 300, c, hw)
    add("plane shorter than a step, V=1 by offset", 300, 1, 4, off={"y": 4})
    for i, nv in enumerate(_NV):
        for v in (4, 2, 1):                                             # every edge at every width: the edges are in vectors
            n, hw = 1, nv * v
            off = {"y": _V_OFF[v]} if v != 4 else {}
            b = Bn("%d vectors of %d per channel" % (nv, v), n, 1 + i % 2, hw, off=off)
            assert b.v_stats == b.v_apply == b.v_bwd == v and b.count == nv * v, (b, v)
            rows.append(b)
    # the chunks: one, exactly one, two (the seam inside the one plane), three (the seam inside the second plane; hw odd: V = 1)
    add("one chunk less a vector", 1, 2, CHUNK - 4)
    add("one chunk", 2, 1, CHUNK // 2)
    add("two chunks, seam inside the plane", 1, 2, CHUNK + 4)
    add("three chunks of 2*16384+1", 3, 1, (2 * CHUNK + 1) // 3)
    add("fifth trip of the 64-workgroup cap", 1, 1, 65537 + 4)
    add("c=1 n=1", 1, 1, 8)
    add("c=65", 2, 65, 12)
    add("c=65 hw odd", 1, 65, 7)
    for i, b in enumerate(rows):
        b.null = NULL_SETS[i % len(NULL_SETS)]
    return rows


BN_CASES = _bn_cases()
EVAL_CASES = (1, 2, 64, 65, 130)                                      # channels of vocr_bn_eval_stats (64 threads per workgroup)


def ints(shape, seed, dev=None):
    t = torch.randint(-8, 9, tuple(shape), generator=torch.Generator().manual_seed(seed)).float()
    return t if dev is None else t.to(dev)


def bn_params(c, seed):
    g = torch.Generator().manual_seed(seed)
    gamma = torch.rand(c, generator=g) * 0.6 + 0.7
    beta = (torch.rand(c, generator=g) * 2 - 1) * 0.3
    rm0 = (torch.rand(c, generator=g) * 2 - 1) * 0.5
    rv0 = torch.rand(c, generator=g) + 1.0
    return gamma, beta, rm0, rv0


def bn_y(shape, seed):
    """N(0,1) scaled and offset per channel (shape [n][c]...)"""
    g = torch.Generator().manual_seed(seed)
    c = shape[1]
    v = [1, -1] + [1] * (len(shape) - 2)
    return torch.randn(shape, generator=g) * (0.5 + torch.rand(c, generator=g)).view(v) + ((torch.rand(c, generator=g) * 2 - 1) * 0.6).view(v)


# ---------------------------------------------------------------------------------------------------------- fractional pool
class Frac(object):
    """(n, c, h, w) -> (oh, ow); plane p = i c + j takes the samples u_w = SAMPLES[(su + p) % 7], u_h = SAMPLES[(sv + 3 p) % 7].
    dx_offs: the byte offsets of dx vocr_fracpool2x2_bwd runs at.  variants: the planes the fused forward / backward run on."""

    def __init__(self, name, n, c, h, w, oh, ow, su=0, sv=0, dx_offs=(0,), variants=("rand",)):
        self.name, self.n, self.c, self.h, self.w, self.oh, self.ow = name, n, c, h, w, oh, ow
        self.su, self.sv, self.dx_offs, self.variants = su, sv, tuple(dx_offs), tuple(variants)
        assert h >= 2 and w >= 2 and 1 <= oh <= h - 1 and 1 <= ow <= w - 1 and 1 <= n * c <= 3 and h * w <= MAX_PLANE, self

    def __repr__(self):
        return "%s %dx%dx%dx%d->%dx%d" % (self.name, self.n, self.c, self.h, self.w, self.oh, self.ow)

    supported = property(lambda s: fused_bwd_supported(s.h, s.w, s.oh, s.ow))
    backward = property(lambda s: s.oh >= 2 and s.ow >= 2)           # a row the fused backward is asked about (accepted or refused)
    op = property(lambda s: s.oh * s.ow)
    planes = property(lambda s: s.n * s.c)

    def sample_pairs(self):
        return [(SAMPLES[(self.su + p) % 7], SAMPLES[(self.sv + 3 * p) % 7]) for p in range(self.planes)]

    def samples(self):
        return torch.tensor(self.sample_pairs(), dtype=torch.float32).view(self.n, self.c, 2)

    def starts(self, p):
        """(window starts along w, along h) of plane p, the pinned last one included"""
        uw, uh = self.sample_pairs()[p]
        return cr.fracpool_starts(uw, self.w, self.ow), cr.fracpool_starts(uh, self.h, self.oh)

    def layouts(self):
        """{(axis, "overlapping" / "abutting" / "apart")} over the planes: the pinned last window against its neighbour"""
        out = set()
        for p in range(self.planes):
            for axis, s in zip("wh", self.starts(p)):
                if len(s) >= 2:
                    gap = int(s[-1] - s[-2])
                    out.add((axis, "coinciding" if gap <= 0 else "overlapping" if gap == 1 else "abutting" if gap == 2 else "apart"))
        return out


_ALL = ("rand", "const", "ramp", "planted")


def _frac_cases():
    rows = []
    k = [0]

    def add(name, n, c, h, w, oh, ow, **kw):
        k[0] += 1
        kw.setdefault("su", k[0])
        kw.setdefault("sv", 3 * k[0] + k[0] // 7)
        if h * w <= 4096 and oh >= 2 and ow >= 2:
            kw.setdefault("variants", _ALL)
        rows.append(Frac(name, n, c, h, w, oh, ow, **kw))

    # ---- the forwards: out of 1 (alpha 0), 2, in - 1 (alpha exactly 1), the ratios
    add("out 1x1", 1, 1, 2, 2, 1, 1)
    add("oh=1 ow=in-1", 1, 2, 2, 3, 1, 2)
    add("oh=in-1 ow=1", 2, 1, 3, 2, 2, 1)
    add("alpha 1 both", 1, 3, 3, 3, 2, 2)
    add("oh=1", 1, 2, 4, 4, 1, 3)
    add("ow=1", 2, 1, 4, 4, 3, 1)
    add("ratios odd", 1, 3, 5, 7, 2, 4)
    add("alpha 1 both", 3, 1, 5, 7, 4, 6)
    add("alpha 1 both", 1, 2, 9, 13, 8, 12)
    add("ratios odd", 1, 2, 9, 13, 4, 9)
    add("ratios w%4=2", 1, 2, 7, 30, 3, 21)
    add("out 2x2 w odd", 1, 2, 6, 9, 2, 2)
    # ---- the fused backward: h from 4, w in 4 ... 260; out = 2, the ratios, the largest accepted and the smallest refused
    add("smallest", 1, 1, 4, 4, 2, 2, dx_offs=(0, 4))
    add("out 2x2: pinned window apart", 1, 2, 5, 8, 2, 2)
    add("ratios", 1, 3, 6, 8, 3, 5)
    add("largest ow", 1, 2, 4, 8, 2, 6)
    add("smallest refused ow", 1, 1, 4, 8, 2, 7)
    add("ratios", 3, 1, 7, 12, 3, 8)
    add("largest oh and ow", 1, 2, 6, 12, 4, 10)
    add("smallest refused oh", 1, 1, 6, 12, 5, 8)
    add("smallest refused ow", 1, 1, 7, 12, 3, 11)
    add("out 2 x ratio", 1, 3, 9, 16, 2, 11)
    add("largest ow", 1, 2, 9, 16, 4, 14)
    add("smallest refused ow", 1, 1, 9, 16, 4, 15)
    add("ratios", 1, 3, 30, 20, 15, 14, dx_offs=(0, 4))
    add("largest ow", 2, 1, 5, 20, 2, 18)
    add("ratios", 1, 3, 15, 36, 7, 25)
    add("largest ow", 1, 2, 4, 36, 2, 34)
    add("smallest refused ow", 1, 1, 4, 36, 2, 35)
    add("ow=2: pinned column apart", 1, 2, 30, 36, 15, 2)
    add("ratios", 1, 3, 7, 260, 3, 182)
    add("largest ow", 1, 1, 4, 260, 2, 256)
    add("smallest refused ow", 1, 1, 4, 260, 2, 257)
    add("alpha exactly 1.01f", 1, 2, 6, 204, 3, 201)
    add("alpha below 1.01f", 1, 1, 6, 204, 3, 202)
    add("w%4=2 refused", 1, 2, 6, 30, 3, 21)
    # ---- pooled outputs per plane on and around 256 / 1024 (the pooled partial pass's four slots, the forward's grid) and 512 / 2048
    # (pool_bwd_lds_kernel's trips of 4 x 512)
    for op, (h, w, oh, ow) in ((255, (30, 24, 15, 17)), (256, (32, 24, 16, 16)), (511, (14, 104, 7, 73)), (512, (32, 48, 16, 32)),
                               (513, (38, 40, 19, 27)), (1023, (62, 48, 31, 33)), (1024, (64, 48, 32, 32)), (1025, (50, 60, 25, 41)),
                               (2047, (46, 128, 23, 89)), (2048, (64, 92, 32, 64)), (2049, (6, 976, 3, 683))):
        assert oh * ow == op
        add("%d outputs per plane" % op, 1, 1 + op % 2, h, w, oh, ow)
    add("257 outputs per plane (oh=1)", 1, 1, 2, 300, 1, 257)
    # ---- n oh ow below the chunk count (5 chunks sized from n h w, 4 outputs)
    add("fewer outputs than chunks", 1, 1, 16, 4100, 2, 2)
    # ---- the LDS bound of the fused backward with equality, and the first width past it
    add("LDS bound met", 1, 1, 4, 8184, 2, 5728)
    add("LDS bound exceeded", 1, 1, 4, 8188, 2, 5731)
    # ---- input planes on and past 8192 / 18432 / 36864 floats, in_plane % 4 zero and non-zero, dx aligned and 4 bytes off
    # (18433 is prime: 18434 stands for it)
    for h, w in ((2, 4095), (8, 1024), (3, 2731), (3, 2732), (10, 1843), (16, 1152), (13, 1418), (4, 4609), (14, 2633), (32, 1152),
                 (5, 7373), (4, 9217)):
        oh, ow = ratio_out(h, w)
        add("plane of %d floats (%s)" % (h * w, pool_regime(h * w)), 1, 1 + (h * w) % 2, h, w, oh, ow, dx_offs=(0, 4))
    return rows


FRAC_CASES = _frac_cases()
PLANE_SIZES = (8190, 8192, 8193, 8196, 18430, 18432, 18434, 18436, 36862, 36864, 36865, 36868)
# non-finite inputs: (h, w, oh, ow) of one plane; a NaN at a pixel two windows share, and a window of four -inf
NONFINITE_CASE = Frac("NaN and an all -inf window", 1, 2, 6, 8, 3, 5, su=2, sv=3)


def nonfinite_plane(f):
    """NONFINITE_CASE's planes: a NaN in a pixel two windows share and a later NaN in one of them (plane 1), a window of four -inf (plane
    0, its first window)"""
    x = frac_plane_data(f, "rand", 9)
    sw, sh = f.starts(1)
    x[0, 1, sh[1], sw[1]] = float("nan")
    x[0, 1, sh[1] + 1, sw[1] + 1] = float("nan")
    sw, sh = f.starts(0)
    x[0, 0, sh[0]:sh[0] + 2, sw[0]:sw[0] + 2] = float("-inf")
    return x


def frac_plane_data(case, variant, seed, integer=False):
    """y [n][c][h][w] of a variant (module docstring); integer: small integers instead of N(0,1), for the exact host checks (used with
    mean 0, invstd 1, gamma 1, beta 0: the activation is relu(y))"""
    n, c, h, w = case.n, case.c, case.h, case.w
    if variant == "const":
        return torch.full((n, c, h, w), 3.0 if integer else 0.625)
    pos = (torch.arange(h).view(h, 1) * w + torch.arange(w).view(1, w)).float()
    if variant == "ramp":
        return (pos + 1.0 if integer else pos / (h * w)).expand(n, c, h, w).clone()
    y = ints((n, c, h, w), seed) if integer else bn_y((n, c, h, w), seed)
    if variant == "planted":
        for p in range(case.planes):
            sw, sh = case.starts(p)
            rows = [int(a) + 1 for a, b in zip(sh[:-1], sh[1:]) if b - a == 1]
            cols = [int(a) + 1 for a, b in zip(sw[:-1], sw[1:]) if b - a == 1]
            for r in rows:
                for q in cols:                   # later pixels a little larger: the last of a run of shared pixels wins its four windows
                    y[p // c, p % c, r, q] = (20.0 + r * w + q) if integer else (8.0 + float(pos[r, q]) / (h * w))
    else:
        assert variant == "rand", variant
    return y


# ---------------------------------------------------------------------------------------------------------- ReLU + MaxPool
MAXPOOL_AXES = dict(n=(1, 2), c=(1, 3), h=(2, 3, 4, 5, 33), w=(2, 3, 4, 5, 33))
# output counts on and around 256 and 1024 (the grid of one and two workgroups per plane)
MAXPOOL_CASES = cover2(MAXPOOL_AXES) + [(1, 2, 31, 34), (2, 1, 32, 33), (1, 1, 2, 515), (1, 2, 63, 66), (1, 1, 64, 65), (1, 1, 51, 82)]


# ------------------------------------------------------------------------------------- the fused backward's algorithm, restated
FUSED_MUTANTS = ("no_last_col", "no_last_row", "no_wb", "no_fifth", "skip_by_first_lane", "no_last_chunk")


def fused_bwd_gather(dout, idx, sw, sh, H, W, mutant=None, stats=None):
    """The un-pooled gradient of ONE plane as bn_pool.hip's comment describes the fused backward: the starts of windows 0 .. out - 2
    strictly increase, so a column is the first column of at most one window (map wa) and the second of at most one (wb), rows likewise
    (ha, hb); the last window, pinned at in - 2, stays out of the maps.  A thread owns 4 consecutive pixels of a row (W % 4 == 0); the
    windows that can have elected one of them start in [w0 - 1, w0 + 3] - five candidates - in at most two window rows; a candidate row
    none of the 64 pixel groups of a wave has is skipped by the whole wave; groups in the last two rows or at the end of a row also look
    at the pinned window row / column.  dout [OH][OW] and idx [OH][OW] numpy; returns da [H][W] (float64).
    mutants (FUSED_MUTANTS): the pinned last column / row left out; the second-column map dropped; the fifth candidate (start == w0 + 3)
    dropped; the wave-uniform skip decided by the wave's first group alone.  stats: a dict that receives what the plane exercised."""
    OH, OW = dout.shape
    d, ix = dout.reshape(-1).astype(np.float64), idx.reshape(-1).astype(np.int64)
    wa, wb = np.full(W + 4, -1, dtype=np.int64), np.full(W + 4, -1, dtype=np.int64)
    ha, hb = np.full(H, -1, dtype=np.int64), np.full(H, -1, dtype=np.int64)
    for o in range(OW - 1):
        wa[sw[o]], wb[sw[o] + 1] = o, o
    for o in range(OH - 1):
        ha[sh[o]], hb[sh[o] + 1] = o, o
    if mutant == "no_wb":
        wb[:] = -1
    gw = W // 4
    gi = np.arange(H * gw)
    h, w0 = gi // gw, (gi % gw) * 4
    p0 = h * W + w0
    orow = [ha[h], hb[h]]
    ocol = [wb[w0], wa[w0], wa[w0 + 1], wa[w0 + 2], wa[w0 + 3]]
    if mutant == "no_fifth":
        ocol[4] = np.full_like(ocol[4], -1)
    da = np.zeros((H * gw, 4))
    wave = gi // 64
    skipped = fifth = 0

    def take(ok, o):
        j = ix[o] - p0
        for q in range(4):
            da[:, q] += np.where(ok & (j == q), d[o], 0.0)
        return j

    for r in range(2):
        live = orow[r] >= 0
        if mutant == "skip_by_first_lane":
            runs = live[::64][wave]
        else:
            any_ = np.zeros(int(wave.max()) + 1, dtype=bool)
            np.logical_or.at(any_, wave, live)
            runs = any_[wave]
        skipped += int((~runs).sum())
        for k in range(5):
            ok = runs & live & (ocol[k] >= 0)
            j = take(ok, np.maximum(orow[r], 0) * OW + np.maximum(ocol[k], 0))
            if k == 4:
                fifth += int((ok & (j == 3)).sum())
    lr = np.where(h >= H - 2, OH - 1, -1)
    lc = np.where(w0 + 3 >= W - 2, OW - 1, -1)
    if mutant == "no_last_row":
        lr[:] = -1
    if mutant == "no_last_col":
        lc[:] = -1
    rows3, cols6 = orow + [lr], ocol + [lc]
    for r in range(3):
        for k in range(6):
            if r < 2 and k < 5:
                continue
            ok = (rows3[r] >= 0) & (cols6[k] >= 0)
            take(ok, np.where(ok, rows3[r] * OW + cols6[k], 0))
    if stats is not None:
        stats["skipped"] = stats.get("skipped", 0) + skipped
        stats["fifth"] = stats.get("fifth", 0) + fifth
    return da.reshape(H, W)


def pooled_partial_sums(dout, idx, act, xhat, h, w, mutant=None):
    """(dbeta, dgamma) of the fused backward's partial pass, fp64: per channel, the n oh ow pooled elements in chunks whose COUNT comes
    from n h w (the dense pass's workspace) - sum of dout [relu active at the winner] and of that times xhat at the winner.
    dout / idx [n][c][oh][ow], act / xhat [n][c][h][w] torch.  mutant "no_last_chunk": the last chunk left out."""
    n, c = dout.shape[:2]
    op = dout.shape[2] * dout.shape[3]
    fl = idx.reshape(n, c, op).long()
    dz = dout.reshape(n, c, op).double() * (torch.gather(act.reshape(n, c, -1), 2, fl) > 0)
    t1 = dz.transpose(0, 1).reshape(c, n * op)
    t2 = (dz * torch.gather(xhat.reshape(n, c, -1).double(), 2, fl)).transpose(0, 1).reshape(c, n * op)
    nch = nchunk(n * h * w)
    per = -(-(n * op) // nch)
    s1, s2 = torch.zeros(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
    for j in range(nch - 1 if mutant == "no_last_chunk" else nch):
        s1 += t1[:, j * per:(j + 1) * per].sum(1)
        s2 += t2[:, j * per:(j + 1) * per].sum(1)
    return s1, s2


# ------------------------------------------------------------------------------------ an honest fp32 BatchNorm (CPU, for the bars)
def honest_bn_forward(y, gamma, beta, eps=1e-5):
    """(mean32, invstd32, out32): double sums rounded once, the apply pass in fp32 - the design the bars of cnn_ref.py describe"""
    c = y.shape[1]
    cnt = y.numel() // c
    yd = y.double().transpose(0, 1).reshape(c, -1)
    m = yd.sum(1) / cnt
    v = ((yd * yd).sum(1) / cnt - m * m).clamp_min(0)
    m32, is32 = m.float(), (1.0 / (v + eps).sqrt()).float()
    out = torch.relu((y - cr._bc(m32, y)) * cr._bc(is32, y) * cr._bc(gamma, y) + cr._bc(beta, y))
    return m32, is32, out


def honest_bn_backward(da, y, mask, m32, is32, gamma):
    """(dy32, dgamma32, dbeta32): fp32 products, double sums, the fp32 expression of the apply pass"""
    c = y.shape[1]
    cnt = y.numel() // c
    red = [0] + list(range(2, y.dim()))
    xh = (y - cr._bc(m32, y)) * cr._bc(is32, y)
    dz = da * mask
    db, dg = dz.double().sum(red).float(), (dz * xh).double().sum(red).float()
    inv = torch.tensor(1.0 / cnt, dtype=torch.float32)
    dy = cr._bc(gamma * is32, y) * (dz - cr._bc(db * inv, y) - xh * cr._bc(dg * inv, y))
    return dy, dg, db


# ---------------------------------------------------------------------------------------------------------------- buffers
class Off(object):
    """A contiguous tensor `off_bytes` (4 or 8) behind a 16-byte boundary, as a Guarded: gemm_ref.Padded with one row.  data given: an
    operand between NaN; None: an output, NaN-filled between the sentinel pattern."""

    def __init__(self, shape, dev, data=None, off_bytes=4, name=""):
        numel = 1
        for s in shape:
            numel *= int(s)
        assert off_bytes in (4, 8)
        self.out, self.name = data is None, name
        self.p = Padded(None if data is None else data.reshape(1, numel), numel, off_bytes // 4, dev, sentinel=self.out, shape=(1, numel))
        self.t = self.p.buf[self.p.start:self.p.start + numel].view(tuple(shape))
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == off_bytes

    def outside_untouched(self):
        if self.out:
            return self.p.outside_untouched()
        b = self.p.buf
        return bool(torch.isnan(b[:self.p.start]).all()) and bool(torch.isnan(b[self.p.start + self.t.numel():]).all())

    def has_nan(self):
        return bool(torch.isnan(self.t).any())

    has_unwritten = has_nan

    def all_unwritten(self):
        return bool(torch.isnan(self.t).all())

    def bits(self):
        return self.t.reshape(-1).view(torch.int32)


def buf(shape, dev, data=None, off_bytes=0, name="", dtype=torch.float32, band=0):
    if off_bytes:
        assert dtype == torch.float32
        return Off(shape, dev, data, off_bytes, name)
    return Guarded(shape, dev, data=data, dtype=dtype, name=name, band=band)


# ------------------------------------------------------------------------------ the comparisons, shared by the CPU and the GPU test
def bn_forward_ratios(y, gamma, beta, got, rm0=None, rv0=None, momentum=0.1, eps=1e-5):
    """error / bar of a training-mode BatchNorm + ReLU forward against cnn_ref, on y's device.  got: mean, invstd, out and, where the
    call had them, running_mean, running_var, xhat_sum.  ReLU decisions come from got["out"]; every decision that differs from fp64 must
    be a near-tie inside the forward bar.  Returns ([(quantity, ratio)], what the backward comparison needs)."""
    cnt = y.numel() // y.shape[1]
    mean, invstd, var, rm, rv = cr.bn_stats(y, rm0, rv0, momentum, eps)
    e_mean, e_is, e_var = cr.bn_stat_bars(mean, var, invstd, eps)
    rows = [("mean", cr.ratio(got["mean"], mean, e_mean)), ("invstd", cr.ratio(got["invstd"], invstd, e_is * invstd))]
    var_unb = var * cnt / (cnt - 1) if cnt > 1 else var
    zero = torch.zeros_like(mean)
    brm, brv = cr.running_bars(zero if rm0 is None else rm0, zero if rv0 is None else rv0, mean, var_unb, e_mean, e_var, momentum, cnt)
    if rm0 is not None and "running_mean" in got:
        rows.append(("running_mean", cr.ratio(got["running_mean"], rm, brm)))
    if rv0 is not None and "running_var" in got:
        rows.append(("running_var", cr.ratio(got["running_var"], rv, brv)))
    if "xhat_sum" in got:
        rows.append(("xhat_sum", cr.ratio(got["xhat_sum"], torch.zeros_like(mean), 2 * cr.xhat_sum_bound(mean, invstd, cnt) + 1e-30)))
    pre = cr.bn_relu_pre(y, mean, invstd, gamma, beta)
    bar, e_xhat = cr.bn_apply_bar(y, mean, invstd, gamma, beta, e_mean, e_is)
    mask = got["out"].to(y.device) > 0
    flips = mask != (pre > 0)
    if bool(flips.any()):
        rows.append(("ReLU flips near-tie", float((pre[flips].abs() / bar[flips]).max())))
    rows.append(("apply", cr.ratio(got["out"], torch.where(mask, pre, torch.zeros_like(pre)), bar)))
    return rows, dict(mean=mean, invstd=invstd, mask=mask, e_xhat=e_xhat, bar=bar, pre=pre, count=cnt)


def bn_backward_ratios(da, y, gamma, ctx, got, mask=None):
    """error / bar of dy, dgamma, dbeta (and dconv_bias, against 0) for the gradient da of the activation; ctx from bn_forward_ratios"""
    mean, invstd, mask = ctx["mean"], ctx["invstd"], ctx["mask"] if mask is None else mask
    dy, dgamma, dbeta = cr.bn_relu_bwd(da, y, mask, mean, invstd, gamma)
    b_dy, b_dg, b_db = cr.bn_bwd_bars(da, y, mask, mean, invstd, gamma, dgamma, dbeta, ctx["e_xhat"])
    rows = [("dy", cr.ratio(got["dy"], dy, b_dy)), ("dgamma", cr.ratio(got["dgamma"], dgamma, b_dg)), ("dbeta", cr.ratio(got["dbeta"], dbeta, b_db))]
    if "dconv_bias" in got:
        rows.append(("dconv_bias", cr.ratio(got["dconv_bias"], torch.zeros_like(dgamma), cr.conv_bias_grad_bar(mean, invstd, gamma, dgamma, ctx["count"]))))
    return rows
