"""The case tables and the guarded 4-D buffers of the conv seam suite (tests/test_cnn_seams_gpu.py runs the tables on the GPU,
tests/test_cnn_ref_cpu.py holds them to being fair to an honest fp32 convolution and to rejecting the seam mutants of tests/cnn_ref.py).
Importing this module needs no GPU and no library.

Buffers are the guarded ones of tests/guarded.py (re-exported here): a tensor the kernel READS sits between guard bands of NaN, so a read
outside it reaches the result; a tensor the kernel WRITES (outputs, and workspaces of exactly the bytes their *_workspace_bytes query
answers) starts as NaN between bands of the sentinel bit pattern, so an element the kernel leaves out, or a workspace word it reads without
having written it, shows as NaN and a store outside shows as a touched band.

Tables: every row is a LAUNCH shape (n, cin, h, w, cout) - cin the contraction channels, cout the channels of the tensor written; a data
gradient of a layer (a -> b) is the launch (n, b, h, w, a) with the layer's data-gradient pack.  A table is not a cross product:
`cover2` lists rows until every value of every axis has met at least two values of every other axis, within a cap on the output's size.
The values of each axis sit on the seams of the kernels (conv_wino.hip, conv.hip, conv_f16.hip):
  forward / data gradient   W % 4 and W % 2 (column groups of F(4,3) / F(2,3)), n h (T + 1) % 32 (32-slot segments across rows and images),
                            the segments of a tile (2 / 4 / 8), H of 1 and 2 (both halo rows outside the image), Cin % 4 (half-chunks of 4
                            input channels), Cout around 32 / 64 / 128 and the F(2,3) / F(4,3) switch at 64
  weight gradient           odd H (a half-empty row pair), 8-slot segments, splits from the segment count, both reduce kernels, the
                            768-thread kernel (Cin Cout % 4 != 0), Cin / Cout around the 64-channel tile, the direct and one-channel kernels
  fp16                      tiles of 8 / 12 / 16 rows x 32 / 64 pixels, Cin in chunks of 16, Cout around 64 / 128, rows padded to ceil8(W) + 8"""
import torch

from tests.guarded import Guarded, workspace          # noqa: F401  (the guarded buffers live in tests/guarded.py; the conv, x6 and augment suites take them from here)


# ---------------------------------------------------------------------------------------------------------------- tables
def cover2(axes, size_axes=(), cap=None, first=()):
    """Rows over `axes` (name -> values, in order) such that every value of every axis appears with at least two values of every other
    axis (all of them where an axis has fewer).  `first`: rows the table starts with.  size_axes / cap: the product of those axes' values
    stays within cap.  Greedy and deterministic: the first unmet (value, other axis) seeds a row; every other axis takes the value that
    meets the most unmet pairs."""
    names = list(axes)
    vals = [list(axes[k]) for k in names]
    k = len(names)
    sized = [names.index(a) for a in size_axes]
    rows = [tuple(r) for r in first]

    def seen(a, v, b):
        return {r[b] for r in rows if r[a] == v}

    def lacks(a, v, b):
        return len(seen(a, v, b)) < min(2, len(vals[b]))

    def fits(row, b, u):
        if cap is None or b not in sized:
            return True
        prod = u
        for c in sized:
            if c != b:
                prod *= row[c] if row[c] is not None else min(vals[c])
        return prod <= cap

    while True:
        need = [(a, v, b) for a in range(k) for v in vals[a] for b in range(k) if b != a and lacks(a, v, b)]
        if not need:
            return rows
        a, v, _ = need[0]
        row = [None] * k
        row[a] = v
        for b in range(k):
            if b == a:
                continue

            def gain(u):
                g = 100 * (u not in seen(a, v, b) and lacks(a, v, b))
                g += 10 * sum(1 for c in range(k) if c != b and row[c] is not None and lacks(b, u, c) and row[c] not in seen(b, u, c))
                g += sum(1 for c in range(k) if c != b and lacks(b, u, c))
                return g
            ok = [u for u in vals[b] if fits(row, b, u)]
            assert ok, "cover2: the cap leaves no value for axis %s in a row with %s" % (names[b], row)
            row[b] = max(ok, key=lambda u: (gain(u), -vals[b].index(u)))
        short = lambda: sum(min(2, len(vals[b2])) - len(seen(a2, v2, b2)) for (a2, v2, b2) in need)
        before = short()
        rows.append(tuple(row))
        assert short() < before, "cover2: no progress on %s (cap too small?)" % (need[0],)


def covers2(rows, axes):
    """the property cover2 promises, checked from the rows alone"""
    names = list(axes)
    for a, ka in enumerate(names):
        for v in axes[ka]:
            for b, kb in enumerate(names):
                if b != a and len({r[b] for r in rows if r[a] == v}) < min(2, len(axes[kb])):
                    return False
    return True


# all rows (n, cin, h, w, cout)
_OUT = ("n", "cout", "h", "w")
SMALL_CAP = 8192                                                 # output elements of a small case

# ---- plain fp32 forward / data gradient: vocr_conv3x3_wino_fwd (cout % 4 == 0: plans 1, 3 and 4 at these grids) and the direct kernel
WINO_AXES = dict(n=(1, 3), cin=(1, 2, 3, 4, 5, 7, 8, 9, 12), h=(1, 2, 3, 5), w=(1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 33, 63, 65, 127, 129),
                 cout=(4, 12, 36, 60, 64, 68, 124, 128, 132, 260))
WINO_CASES = cover2(WINO_AXES, _OUT, SMALL_CAP)
DIRECT_AXES = dict(WINO_AXES, cout=(6, 10))
DIRECT_CASES = cover2(DIRECT_AXES, _OUT, SMALL_CAP)

# ---- the launch plans that need a large grid, one shape per W % 4 at Cin = 8: the smallest outputs the rule of wino_plan_of gives each
# id at 256 CUs (found by a search over vocr_conv3x3_wino_plan; the GPU test asserts the id the library reports on ITS device).
# 5 / 6: one 8-wave workgroup per CU (64 / 128 channels), 7 / 8: two 4-wave workgroups per CU, +16: direct-form tail pieces lead the launch
PLAN_CASES = {
    5: [(32, 8, 7, 580, 64), (32, 8, 30, 133, 64), (32, 8, 30, 134, 64), (32, 8, 30, 135, 64)],
    6: [(32, 8, 7, 580, 128), (32, 8, 7, 577, 128), (32, 8, 7, 578, 128), (32, 8, 7, 579, 128)],
    7: [(32, 8, 30, 408, 64), (32, 8, 30, 405, 64), (32, 8, 30, 406, 64), (32, 8, 30, 407, 64)],
    8: [(32, 8, 30, 204, 128), (32, 8, 30, 201, 128), (32, 8, 30, 202, 128), (32, 8, 30, 203, 128)],
    17: [(8, 8, 30, 272, 16), (8, 8, 30, 273, 16), (8, 8, 30, 274, 16), (32, 8, 30, 67, 16)],
    20: [(8, 8, 30, 272, 128), (32, 8, 30, 65, 128), (32, 8, 30, 66, 128), (32, 8, 30, 67, 128)],
    23: [(32, 8, 30, 272, 64), (32, 8, 30, 269, 64), (32, 8, 30, 270, 64), (32, 8, 30, 271, 64)],
    24: [(8, 8, 30, 544, 128), (32, 8, 30, 133, 128), (32, 8, 30, 134, 128), (32, 8, 30, 135, 128)],
}
# every id vocr_conv3x3_wino_plan can report in the shipped library (tests/test_cnn_fp64_gpu.py says why 2, 9, 10, 18, 19, 21, 22 cannot be)
REACHABLE_PLANS = {1, 3, 4, 5, 6, 7, 8, 17, 20, 23, 24}

# ---- weight gradient (cin, cout) is one axis: the pairs pick the kernel
WGRAD_PAIRS = ((4, 4), (8, 16), (5, 6), (7, 9), (60, 68), (64, 64), (68, 60), (124, 132), (2, 8), (3, 64), (1, 16), (1, 64))
WGRAD_AXES = dict(n=(1, 3, 17), h=(1, 2, 3, 4, 7), w=(1, 3, 4, 5, 8, 9, 33), pair=WGRAD_PAIRS)
# the first row: 85 segments of 8 slots and a small filter - the 1024-thread reduce (splits >= 64 and 3 Cout Cin / 4 < 4096)
WGRAD_CASES = [(n, p[0], h, w, p[1]) for n, h, w, p in cover2(WGRAD_AXES, first=[(17, 7, 33, (8, 16)), (17, 7, 33, (64, 64))])]


def wgrad_kernel(cin, cout):
    """which weight-gradient entry point the model's dispatch (ops.conv3x3_wgrad) gives the pair, and the family of its bar"""
    if cin == 1:
        return "c1", "direct"
    if cin <= 3:
        return "direct", "direct"
    return ("rowpair" if cin * cout % 4 == 0 else "wino3"), "wgrad"


def rowpair_splits(n, cin, h, w, cout, ncu=256):
    """the split count of the row-pair weight-gradient kernel (wgrad_wino2d_splits): 8-slot segments of the stream of row PAIRS, cut
    into one range per workgroup at one workgroup per CU and tile"""
    cdiv = lambda a, b: (a + b - 1) // b
    nseg = cdiv(n * cdiv(h, 2) * (cdiv(w, 4) + 1), 8)
    tiles = cdiv(cin, 64) * cdiv(cout, 64)
    s = max(1, min(cdiv(ncu, tiles), nseg))
    return cdiv(nseg, cdiv(nseg, s))


# ---- fp16 operands.  vocr_conv3x3_h16_fwd (forward and data-gradient packs): small rows, then one launch per plan the small ones miss
H16_AXES = dict(n=(1, 3), cin=(16, 32, 48, 80), h=(1, 7, 8, 9, 12, 13, 16, 17), w=(1, 31, 32, 33, 63, 64, 65), cout=(1, 16, 63, 64, 65, 129))
H16_CAP = 20000
H16_CASES = cover2(H16_AXES, _OUT, H16_CAP)
H16_PLAN_CASES = {3: (32, 16, 17, 65, 128), 4: (32, 16, 25, 65, 128), 5: (32, 16, 1, 257, 128)}
# vocr_conv3x3_f16_fwd (register-staged: any Cin) and vocr_conv3x3_wgrad_f16 at the input layers' channel counts
F16_AXES = dict(n=(1, 3), cin=(1, 3, 8), h=(1, 7, 9), w=(1, 31, 33, 65), cout=(16, 63, 65, 129))
F16_CASES = cover2(F16_AXES, _OUT, H16_CAP)
WGRAD_F16_AXES = dict(n=(1, 3), cin=(1, 3, 8), h=(1, 2, 7), w=(1, 9, 33, 65), cout=(16, 64, 68))
WGRAD_F16_CASES = cover2(WGRAD_F16_AXES)
# vocr_conv3x3_wgrad_h16: n h rows of ceil(w / 64) units each, few enough that every unit is a split of its own
WGRAD_H16_AXES = dict(nh=((1, 1), (1, 3), (2, 2), (3, 1)), w=(1, 7, 8, 9, 63, 64, 65), pair=((64, 64), (64, 128), (128, 256)))
WGRAD_H16_CASES = [(nh[0], p[0], nh[1], w, p[1]) for nh, w, p in cover2(WGRAD_H16_AXES)]
# vocr_f32_to_f16_layouts: (n, c, h, w); c = 8 takes the padded channel-major copy only
LAYOUT_AXES = dict(n=(1, 2), c=(8, 16, 48, 64, 80, 144), h=(1, 3), w=(1, 7, 8, 9, 56, 57, 63, 64, 65))
LAYOUT_CASES = cover2(LAYOUT_AXES)


def padded_row(w):
    """vocr_f16_padded_row: rows of the channel-major fp16 copy, ceil8(w) + 8"""
    return (w + 7) // 8 * 8 + 8


def f16_layouts_ref(x):
    """what vocr_f32_to_f16_layouts writes, by torch: (nhwc [n][c/16][h][w][16] or None when c % 16 != 0, nchwp [n][c][h][WP] with every
    element at w >= W zero)"""
    n, c, h, w = x.shape
    xh = x.half()
    nhwc = xh.view(n, c // 16, 16, h, w).permute(0, 1, 3, 4, 2).contiguous() if c % 16 == 0 else None
    nchwp = torch.zeros(n, c, h, padded_row(w), dtype=torch.float16, device=x.device)
    nchwp[..., :w] = xh
    return nhwc, nchwp


def rand(shape, seed, scale=1.0, dev=None):
    """uniform in [-scale, scale), from the CPU generator (the same data on every device)"""
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(shape, generator=g) * 2 - 1) * scale
    return t.to(dev) if dev is not None else t
