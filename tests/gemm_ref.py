"""Data, float64 reference, poisoned operand buffers and the case table of the fp32 GEMM suite (tests/test_gemm_fp64_gpu.py runs the
table on the GPU, tests/test_gemm_plan_cpu.py asks vocr_gemm_plan about every row of it without one).

Three kinds of operand data, each for a different kind of wrong kernel:
  ints      entries, bias and prior C uniform integers in [-8, 8]: every product and partial sum is an integer below 2^24 (k < 2^18), so
            fp32 is exact in ANY summation order, with any K cut, with or without FMA - the result equals the reference bit for bit.
            The indexing test: a dropped, duplicated or misplaced product fails whatever k is.
  selB/selA one operand has random fp32 values with all 24 significand bits in use, the other exactly one non-zero per column (selB) or
            per row (selA), +-2^e with e in [-3, 3], at a random k: each output is ONE exact product.  The precision test: an operand
            that loses significand bits between memory and the MFMA fails, which small integers cannot show.
  floats    N(0,1): max abs error <= FLOAT_BAR x max |reference| per output matrix (the bar test_gemm_pair_... already holds).

Every operand is a view into a larger allocation with a leading dimension above the natural one.  The row gaps and the guard bands of
A, B and the bias hold NaN (a NaN that is ever read reaches C); those of C hold a sentinel bit pattern that must survive bit for bit; C
itself starts as NaN unless the call accumulates; the workspace starts as NaN too."""
import numpy as np
import torch

LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))           # (transa, transb)
LAYOUT_NAMES = {(0, 0): "NN", (0, 1): "NT", (1, 0): "TN", (1, 1): "TT"}
KINDS = ("ints", "selB", "selA", "floats")
FLOAT_BAR = 2e-5
GUARD = 64                                            # floats in front of and behind every view (a multiple of 4: keeps the alignment)
SENTINEL = 0x7FC5A5A5                                 # a quiet NaN with a payload no kernel produces

# epilogue name -> (bias, relu, accumulate)
EPILOGUES = {"none": (0, 0, 0), "bias": (1, 0, 0), "relu": (0, 1, 0), "bias_relu": (1, 1, 0), "acc": (0, 0, 1), "acc_relu": (0, 1, 1)}
ALL_EPI = tuple(EPILOGUES)


# ---------------------------------------------------------------------------------------------------------------- data
def _full_mantissa(shape, g):
    """fp32 values whose 24 significand bits are all in play (lowest bit set), exponents in [-2, 2], random sign."""
    n = int(np.prod(shape))
    man = torch.randint(0, 1 << 23, (n,), generator=g, dtype=torch.int64) | 1
    exp = torch.randint(125, 130, (n,), generator=g, dtype=torch.int64)
    sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int64)
    bits = (sign << 31) | (exp << 23) | man
    bits = torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32)
    return bits.view(torch.float32).reshape(shape).clone()


def _ints(shape, g):
    return torch.randint(-8, 9, shape, generator=g).float()


def make_data(kind, m, n, k, seed):
    """(A [m][k], B [k][n], bias [n], prior C [m][n]) in fp32 on the CPU, and the float64 product A B.  k is the TOTAL k (both K
    segments of a mode-1 pair)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "ints":
        a, b = _ints((m, k), g), _ints((k, n), g)
        ab = a.double() @ b.double()
    elif kind == "selB":
        a = _full_mantissa((m, k), g)
        kidx = torch.randint(0, k, (n,), generator=g)
        s = torch.ldexp(torch.ones(n), torch.randint(-3, 4, (n,), generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
        b = torch.zeros(k, n)
        b[kidx, torch.arange(n)] = s
        ab = a.double()[:, kidx] * s.double()[None, :]
    elif kind == "selA":
        b = _full_mantissa((k, n), g)
        kidx = torch.randint(0, k, (m,), generator=g)
        s = torch.ldexp(torch.ones(m), torch.randint(-3, 4, (m,), generator=g)) * (torch.randint(0, 2, (m,), generator=g) * 2 - 1).float()
        a = torch.zeros(m, k)
        a[torch.arange(m), kidx] = s
        ab = s.double()[:, None] * b.double()[kidx, :]
    elif kind == "floats":
        a, b = torch.randn((m, k), generator=g), torch.randn((k, n), generator=g)
        ab = a.double() @ b.double()
    else:
        raise ValueError(kind)
    if kind == "floats":
        bias, c0 = torch.randn((n,), generator=g), torch.randn((m, n), generator=g)
    else:                                              # integers: the one fp32 addition of the epilogue rounds like the float64 one
        bias, c0 = _ints((n,), g), _ints((m, n), g)
    return a, b, bias, c0, ab


def reference(ab, bias, c0, epi):
    """float64: A B (+ bias) (+ prior C) (relu), in the order the library applies them."""
    has_bias, relu, acc = EPILOGUES[epi]
    r = ab.clone()
    if has_bias:
        r += bias.double()[None, :]
    if acc:
        r += c0.double()
    if relu:
        r = torch.relu(r)
    return r


# ---------------------------------------------------------------------------------------------------------------- poisoned buffers
class Padded(object):
    """A [rows][cols] matrix as a view with leading dimension ld into a larger device allocation, `offset` floats behind a 16-byte
    aligned address.  Everything that is not the matrix holds NaN, or (sentinel=True, for outputs) the sentinel bit pattern.
    mat: a CPU or device tensor, or None = the matrix itself starts as NaN (an output the call must fully write)."""

    def __init__(self, mat, ld, offset, dev, sentinel=False, shape=None):
        rows, cols = shape if mat is None else mat.shape
        assert ld >= cols
        n = GUARD + offset + rows * ld + GUARD
        if sentinel:
            self.buf = torch.full((n,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        else:
            self.buf = torch.full((n,), float("nan"), device=dev)
        self.rows, self.cols, self.ld, self.start = rows, cols, ld, GUARD + offset
        self.view = self.buf[self.start:self.start + rows * ld].view(rows, ld)[:, :cols]
        if mat is None:
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(mat.to(dev))
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.view.data_ptr()

    def outside_untouched(self):
        """every float of the allocation that is not the matrix still holds the sentinel, bit for bit"""
        t = self.buf.clone()
        t[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = \
            torch.full((1,), SENTINEL, dtype=torch.int32, device=t.device).view(torch.float32)
        return bool((t.view(torch.int32) == SENTINEL).all())


def stored(mat, trans):
    """the matrix as the library reads it: [rows][cols] (trans = 0) or its transpose"""
    return mat.t().contiguous() if trans else mat


# ---------------------------------------------------------------------------------------------------------------- the case table
class Case(object):
    """One row: a shape, how its operands sit in memory and the path each epilogue must take on 256 CUs.

    reach: "pad"   leading dimensions = natural + 4 / + 8 / + 12, every pointer 16-byte aligned
           "off1"  the same, A one float behind a 16-byte boundary (forces the tile kernel with 4-byte loads)
           "ldodd" lda, ldb = natural + 3 (the same, by the leading dimension)
    expect: {epilogue name or "*": path}; path = "<kernel>/<vec|scalar>/<whole|cut|ragged>" for the tile kernel (whole tiles only, every
            tile cut along K, whole tiles + tail pieces), "panel/<whole|split>"; a vocr_gemm_pair that falls back to two vocr_gemm calls
            names the path of each call with a "2x " in front.  `layout_expect` overrides it per layout.
    ws: "full" (the library's own size answer), "half", "null", "short1" (one byte less than the panel kernel's slabs need).
    pair: None = vocr_gemm; 0 / 1 = vocr_gemm_pair's mode (k is then the k of ONE product / ONE segment)."""

    def __init__(self, name, m, n, k, reach, expect, epis=("none",), layouts=LAYOUTS, ws="full", pair=None, tiles_only=False,
                 bias_off=0, plan=None, layout_expect=None, kinds=KINDS):
        self.name, self.m, self.n, self.k, self.reach = name, m, n, k, reach
        self.expect = expect if isinstance(expect, dict) else {"*": expect}
        self.epis, self.layouts, self.ws, self.pair, self.tiles_only, self.bias_off = tuple(epis), tuple(layouts), ws, pair, tiles_only, bias_off
        self.plan = plan or {}                            # exact plan fields the case is about, e.g. {"pieces_per_tile": 31}
        self.layout_expect = layout_expect or {}
        self.kinds = tuple(kinds)

    def __repr__(self):
        return self.name

    def lds(self, ta, tb):
        nat_a, nat_b = (self.m if ta else self.k), (self.k if tb else self.n)
        if self.reach == "ldodd":
            return nat_a + 3, nat_b + 3, self.n + 4
        return nat_a + 4, nat_b + 8, self.n + 12

    def a_offset(self):
        return 1 if self.reach == "off1" else 0

    def aligned(self, epi):
        """vocr_gemm_plan's alignment bits: bit 0 = a and b, bit 1 = c and the biases"""
        return (0 if self.reach == "off1" else 1) | (0 if self.bias_off and self.has_bias(epi) else 2)

    def expected_path(self, epi, layout):
        e = self.layout_expect.get(layout, self.expect)
        e = e if isinstance(e, dict) else {"*": e}
        return e.get(epi, e.get("*"))

    def has_bias(self, epi):
        return bool(EPILOGUES[epi][0])


def path_of(plan):
    """the path name of a vocr_gemm_plan answer (ops.gemm_plan's dict)"""
    if plan["kernel"] == "panel":
        return "panel/" + ("split" if plan["ksplit"] > 1 else "whole")
    cut = "whole" if plan["pieces_per_tile"] == 1 else ("cut" if plan["n_whole"] == 0 else "ragged")
    return "%s/%s/%s" % (plan["kernel"], "vec" if plan["vec"] else "scalar", cut)


def workspace_bytes(case, epi, lib, ta, tb):
    """bytes of workspace the case's call gets"""
    has_bias, relu, acc = EPILOGUES[epi]
    if case.pair is None:
        full = lib.vocr_gemm_workspace_bytes(case.m, case.n, case.k, int(bool(has_bias or relu)))
    else:
        full = lib.vocr_gemm_pair_workspace_bytes(case.m, case.n, case.k, case.pair)
    if case.ws == "full":
        return full
    if case.ws == "half":
        return full // 2
    if case.ws == "null":
        return 0
    assert case.ws == "short1"
    from vistaocr_amd import ops
    lda, ldb, ldc = case.lds(ta, tb)
    p = ops.gemm_plan(ta, tb, case.m, case.n, case.k, lda, ldb, ldc, aligned=case.aligned(epi), epilogue=bool(has_bias or relu), accumulate=bool(acc),
                      workspace_bytes=full, nprob=2 if case.pair == 0 else 1, nseg=2 if case.pair == 1 else 1, tiles_only=case.tiles_only)
    assert p["kernel"] == "panel" and p["ksplit"] > 1, "%s: 'short1' is for a call whose full workspace gives the panel kernel with K slabs" % case
    return p["workspace_bytes"] - 1


def plans_of(case, epi, layout, lib):
    """[(label, plan)] of every product launch the case's call makes, from vocr_gemm_plan: one entry, or the two vocr_gemm calls of a
    vocr_gemm_pair that does not run as one launch (mode 1: the second accumulates and carries the ReLU)."""
    from vistaocr_amd import ops
    ta, tb = layout
    lda, ldb, ldc = case.lds(ta, tb)
    has_bias, relu, acc = EPILOGUES[epi]
    ws = workspace_bytes(case, epi, lib, ta, tb)
    common = dict(aligned=case.aligned(epi), workspace_bytes=ws)
    if case.pair is None:
        return [("gemm", ops.gemm_plan(ta, tb, case.m, case.n, case.k, lda, ldb, ldc, epilogue=bool(has_bias or relu), accumulate=bool(acc), **common))]
    assert not acc
    p = ops.gemm_plan(ta, tb, case.m, case.n, case.k, lda, ldb, ldc, epilogue=bool(has_bias or relu), nprob=2 if case.pair == 0 else 1,
                      nseg=2 if case.pair == 1 else 1, tiles_only=case.tiles_only, **common)
    if p["launches"] == 1:
        return [("pair", p)]
    one = lambda e, a: ops.gemm_plan(ta, tb, case.m, case.n, case.k, lda, ldb, ldc, epilogue=e, accumulate=a, tiles_only=case.tiles_only, **common)
    if case.pair == 0:
        q = one(bool(has_bias or relu), False)
        return [("call 1", q), ("call 2", q)]
    # (the second call of mode 1 has no bias, so a misaligned bias does not keep IT off the panel kernel)
    second = ops.gemm_plan(ta, tb, case.m, case.n, case.k, lda, ldb, ldc, epilogue=bool(relu), accumulate=True, tiles_only=case.tiles_only,
                           aligned=case.aligned(epi) | 2, workspace_bytes=ws)
    return [("call 1", one(bool(has_bias), False)), ("call 2", second)]


def path_name(plans):
    if len(plans) == 1:
        return path_of(plans[0][1])
    a, b = path_of(plans[0][1]), path_of(plans[1][1])
    return "2x " + (a if a == b else a + " + " + b)


_T64S, _T64V = "tile64x64/scalar/", "tile64x64/vec/"


def _cases():
    c = []
    add = lambda *a, **k: c.append(Case(*a, **k))
    # ---- tile kernel, 64x64, whole tiles: degenerate, exact, one over / one under a tile, partial tiles with a K tail of 4
    add("t64 1x1x1", 1, 1, 1, "pad", _T64S + "whole", epis=ALL_EPI)
    add("t64 1x70x5", 1, 70, 5, "pad", _T64S + "whole", epis=ALL_EPI)
    add("t64 70x1x5", 70, 1, 5, "pad", _T64S + "whole", epis=ALL_EPI)
    add("t64 exact vec", 64, 64, 32, "pad", _T64V + "whole", epis=ALL_EPI)
    add("t64 exact off1", 64, 64, 32, "off1", _T64S + "whole", epis=ALL_EPI)
    add("t64 exact ldodd", 64, 64, 32, "ldodd", _T64S + "whole", epis=ALL_EPI)
    add("t64 over", 65, 67, 33, "pad", _T64S + "whole", epis=ALL_EPI)
    add("t64 under", 63, 61, 31, "pad", _T64S + "whole", epis=ALL_EPI)
    add("t64 partial vec ktail4", 132, 68, 100, "pad", _T64V + "whole", epis=ALL_EPI)
    add("t64 partial off1 ktail4", 132, 68, 100, "off1", _T64S + "whole", epis=ALL_EPI)
    # ---- 64x64, every tile cut along K (the K tail lands inside the last piece); an epilogue keeps K whole, accumulate does not
    cut_s = {"*": _T64S + "whole", "none": _T64S + "cut", "acc": _T64S + "cut"}
    cut_v = {"*": _T64V + "whole", "none": _T64V + "cut", "acc": _T64V + "cut"}
    add("t64 cut scalar", 70, 66, 1100, "pad", cut_s, epis=ALL_EPI, plan={"none": {"pieces_per_tile": 2}})
    add("t64 cut vec", 100, 96, 1028, "pad", cut_v, epis=ALL_EPI, plan={"none": {"pieces_per_tile": 2}})
    add("t64 cut scalar half ws", 70, 66, 2200, "pad", _T64S + "cut", epis=("none", "acc"), ws="half")
    add("t64 cut vec half ws", 100, 96, 2052, "pad", _T64V + "cut", epis=("none", "acc"), ws="half")
    add("t64 cut scalar no ws", 70, 66, 1100, "pad", _T64S + "whole", epis=("none", "acc"), ws="null")
    add("t64 cut vec no ws", 100, 96, 1028, "pad", _T64V + "whole", epis=("none", "acc"), ws="null")
    # ---- 128x128, every tile cut: 31 = 1 + 4*7 + 2 pieces (the reduce's 4-wide loop and its remainder)
    big_s = {"*": _T64S + "whole", "none": "tile128x128/scalar/cut", "acc": "tile128x128/scalar/cut"}
    big_v = {"*": _T64V + "whole", "none": "tile128x128/vec/cut", "acc": "tile128x128/vec/cut"}
    add("t128 cut scalar", 250, 250, 16384 + 20, "pad", big_s, epis=ALL_EPI, plan={"none": {"pieces_per_tile": 31}, "acc": {"pieces_per_tile": 31}})
    add("t128 cut vec", 252, 252, 16384 + 20, "pad", big_v, epis=ALL_EPI, plan={"none": {"pieces_per_tile": 31}, "acc": {"pieces_per_tile": 31}})
    # ---- 128x64 whole tiles (k < 64 keeps the panel kernel away)
    add("t128x64 whole vec", 1800, 1800, 60, "pad", "tile128x64/vec/whole", epis=ALL_EPI)
    add("t128x64 whole scalar", 1801, 1799, 61, "pad", "tile128x64/scalar/whole", epis=ALL_EPI)
    # ---- ragged grid: whole tiles + tail pieces, both big tile shapes, through a one-float offset and through `accumulate`
    for (m, n) in ((4200, 2048), (2900, 2904)):
        tile = "tile128x64" if m == 4200 else "tile128x128"
        for k in ((256, 260) if m == 4200 else (512, 516)):
            add("ragged %dx%dx%d off1" % (m, n, k), m, n, k, "off1", tile + "/scalar/ragged", epis=ALL_EPI)
            add("ragged %dx%dx%d acc" % (m, n, k), m, n, k, "pad", {"*": "panel/whole", "acc": tile + "/vec/ragged", "acc_relu": tile + "/vec/ragged"},
                epis=("acc", "acc_relu"))
    # ---- panel kernel, K whole.  On 256 CUs a product needs at least 2 row tiles per workgroup: 64 column panels leave 4 row groups.
    # `accumulate` without K slabs is the one thing it refuses (tile kernel, whole tiles: too few for a ragged grid)
    P, PS = "panel/whole", "panel/split"
    acc_t = "tile128x64/vec/whole"
    for k in (64, 68, 96, 100):                        # 64: shorter than the three-slot ring; 68, 100: a K tail
        add("panel 264x8192x%d" % k, 264, 8192, k, "pad", {"*": P, "acc": acc_t, "acc_relu": acc_t},
            epis=ALL_EPI, plan={"*": {"panels": 64, "groups": 4, "max_row_tiles": 3}})
    # a partial row tile (m % 4 != 0 is refused with a transposed A: those layouts are the scalar tile kernel's)
    for m in (257, 287):
        add("panel %dx8192x68" % m, m, 8192, 68, "pad", P, epis=("none", "bias_relu"), layout_expect={(1, 0): "tile128x64/scalar/whole", (1, 1): "tile128x64/scalar/whole"},
            plan={"*": {"max_row_tiles": 3}})
    # a partial last panel: 4 and 124 of its 128 columns
    for n in (8196, 8316):
        add("panel 264x%dx100" % n, 264, n, 100, "pad", P, epis=("none", "bias_relu"), plan={"*": {"panels": 65, "groups": 3, "max_row_tiles": 3}})
    # row groups of 2 .. 8 row tiles (one chunk; the wave halves take 1+1 .. 4+4), 9 = 5+4, 17 = 6+6+5, 19 = 7+6+6; the last tile is partial
    for L in (2, 3, 4, 5, 6, 7, 8, 9, 17, 19):
        add("panel group of %d" % L, max(256, 128 * L - 28), 8192, 68, "pad", P, epis=("none", "bias_relu"),
            plan={"*": {"groups": 4, "max_row_tiles": L}})
    # ---- panel kernel, K cut into slabs (a single panel is only legal when cut; last groups of 2 and of 1 row tiles; the K tail in the
    # last slab): every epilogue runs in the reduce.  One byte less workspace than the slabs need: another path, same values
    add("panel split 300x128x2052", 300, 128, 2052, "pad", PS, epis=ALL_EPI, plan={"*": {"panels": 1, "groups": 2, "ksplit": 8}})
    add("panel split 260x128x2052", 260, 128, 2052, "pad", PS, epis=("none", "acc_relu"), plan={"*": {"panels": 1, "groups": 2, "ksplit": 8}})
    add("panel split 1000x384x4100", 1000, 384, 4100, "pad", PS, epis=ALL_EPI, plan={"*": {"panels": 3, "groups": 4, "ksplit": 15}})
    short = {"*": "tile64x64/vec/whole", "none": "tile64x64/vec/cut", "acc": "tile64x64/vec/cut"}
    add("panel split 300x128x2052 ws short", 300, 128, 2052, "pad", short, epis=ALL_EPI, ws="short1")
    short = {"*": "tile64x64/vec/whole", "none": "tile128x128/vec/cut", "acc": "tile128x128/vec/cut"}
    add("panel split 1000x384x4100 ws short", 1000, 384, 4100, "pad", short, epis=("none", "bias_relu", "acc"), ws="short1")
    # ---- vocr_gemm_pair: two products (mode 0) and two K segments (mode 1), K whole and cut; the co-scheduling hint and a misaligned
    # bias send it to two vocr_gemm calls
    pe = ("none", "bias", "relu", "bias_relu")
    add("pair0 whole", 264, 8192, 68, "pad", P, epis=pe, pair=0, plan={"*": {"groups": 2, "max_row_tiles": 5}})
    add("pair0 split", 300, 128, 2052, "pad", PS, epis=pe, pair=0, plan={"*": {"groups": 2, "ksplit": 8}})
    add("pair1 whole", 264, 8192, 68, "pad", P, epis=pe, pair=1, plan={"*": {"groups": 4, "max_row_tiles": 3}})
    add("pair1 split", 300, 128, 1028, "pad", PS, epis=pe, pair=1, plan={"*": {"groups": 2, "ksplit": 4}})
    add("pair0 hint", 264, 8192, 68, "pad", "2x tile128x64/vec/whole", epis=("none", "bias_relu"), pair=0, tiles_only=True)
    add("pair1 hint", 264, 8192, 68, "pad", "2x tile128x64/vec/whole", epis=("none", "bias_relu"), pair=1, tiles_only=True)
    # (mode 1 as two calls: the first carries the bias, the second accumulates and carries the ReLU; an epilogue keeps a call's K whole)
    add("pair1 hint split", 300, 128, 1028, "pad", {"none": "2x tile64x64/vec/cut", "bias": "2x tile64x64/vec/whole + tile64x64/vec/cut",
                                                      "bias_relu": "2x tile64x64/vec/whole"}, epis=("none", "bias", "bias_relu"), pair=1, tiles_only=True)
    add("pair0 misaligned bias", 264, 8192, 68, "pad", "2x tile128x64/vec/whole", epis=("bias", "bias_relu"), pair=0, bias_off=1)
    add("pair1 misaligned bias", 264, 8192, 68, "pad", "2x tile128x64/vec/whole", epis=("bias", "bias_relu"), pair=1, bias_off=1)
    # (the second call has no bias: aligned again, and it accumulates through the panel kernel's slab reduce)
    add("pair1 misaligned bias split", 300, 128, 2052, "pad", "2x tile64x64/vec/whole + panel/split", epis=("bias", "bias_relu"), pair=1, bias_off=1)
    return c


CASES = _cases()
