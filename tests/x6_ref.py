"""Data, float64 bars, a numpy emulation, the fragment decoder and the case table of the split-operand GEMM suite (vocr_gemm_x6* = "bf16x6",
vocr_gemm_h3* = "fp16x3"; tests/test_x6_fp64_gpu.py runs the table on the GPU, tests/test_x6_plan_cpu.py asks vocr_gemm_x6_plan about every row
without one, tests/test_x6_ref_cpu.py shows with the emulation that the data kinds have teeth).

The data kinds, Padded, SENTINEL, GUARD and FLOAT_BAR are tests/gemm_ref.py's.  One kind is added:
  sel12A/B  one operand has one non-zero per row (A) / per output column (B), an odd integer of 9 - 12 bits with a random sign, the other is dense
            odd integers of 9 - 12 bits: every output is ONE product below 2^24 (exact in fp32), and both factors need TWO bf16 planes (more than 8
            significant bits), so the result is wrong unless a0 b0, a0 b1, a1 b0 AND a1 b1 are accumulated.  selA / selB (a power of two against a
            full 24-bit significand) pin a0 b1, a0 b2 / a1 b0, a2 b0, the integers a0 b0: all six products of bf16x6 are held by an exact test.

Bars (check()):
  bf16x6  ints, selA, selB, sel12A, sel12B bit-exact against float64; floats within FLOAT_BAR x max |reference| per output matrix.
  fp16x3  ints bit-exact (values in [-8, 8] fit one fp16 plane at any row scale); floats at FLOAT_BAR; the selector kinds per element within the
          bound include/vocr.h states, 2^-22 sum |a||b| + K 2^-39 max|a_row| max|b_row|, evaluated in float64 (+ one fp32 rounding of the result,
          2^-24 |reference|, where the epilogue adds a bias: the bound is the dot product's).

In this file B is [n][k]: the products are C = A . B^T, as the library takes them."""
import numpy as np
import torch

from tests import gemm_ref as gr

SCHEMES = ("bf16x6", "fp16x3")
NPLANES = {"bf16x6": 3, "fp16x3": 2}
KINDS = gr.KINDS + ("sel12A", "sel12B")
EXACT = {"bf16x6": ("ints", "selA", "selB", "sel12A", "sel12B"), "fp16x3": ("ints",)}
EPILOGUES = {"none": (0, 0), "bias": (1, 0), "bias_relu": (1, 1)}


# ---------------------------------------------------------------------------------------------------------------- data
def _odd12(shape, g):
    """odd integers with 9 .. 12 significant bits, random sign"""
    bits = torch.randint(9, 13, shape, generator=g)
    lo = torch.pow(2.0, (bits - 1).double())
    mag = lo + torch.floor(torch.rand(shape, generator=g, dtype=torch.float64) * lo)          # [2^(bits-1), 2^bits)
    mag = torch.floor(mag / 2) * 2 + 1
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return (mag * sign).float()


def make_data(kind, m, n, k, seed, dense_product=True):
    """(A [m][k], B [n][k], bias [n], float64 A B^T) on the CPU.  dense_product=False leaves the product of the two dense kinds (ints, floats)
    to the caller (None): the GPU suite forms it in float64 on the device."""
    if kind in ("ints", "floats") and not dense_product:
        g = torch.Generator().manual_seed(seed)
        gen = gr._ints if kind == "ints" else (lambda shape, g: torch.randn(shape, generator=g))
        return gen((m, k), g), gen((n, k), g), gen((n,), g), None
    if kind in gr.KINDS:
        a, b, bias, _, ab = gr.make_data(kind, m, n, k, seed)
        return a, b.t().contiguous(), bias, ab
    g = torch.Generator().manual_seed(seed)
    if kind == "sel12A":
        b = _odd12((n, k), g)
        kidx = torch.randint(0, k, (m,), generator=g)
        s = _odd12((m,), g)
        a = torch.zeros(m, k)
        a[torch.arange(m), kidx] = s
        ab = s.double()[:, None] * b.double()[:, kidx].t()
    elif kind == "sel12B":
        a = _odd12((m, k), g)
        kidx = torch.randint(0, k, (n,), generator=g)
        s = _odd12((n,), g)
        b = torch.zeros(n, k)
        b[torch.arange(n), kidx] = s
        ab = a.double()[:, kidx] * s.double()[None, :]
    else:
        raise ValueError(kind)
    bias = torch.randint(-8, 9, (n,), generator=g).float()
    return a, b, bias, ab


def reference(ab, bias, epi):
    has_bias, relu = EPILOGUES[epi]
    r = ab.clone()
    if has_bias:
        r += bias.double()[None, :].to(r.device)
    if relu:
        r = torch.relu(r)
    return r


def h3_bound(a, b, k, amax=None, bmax=None):
    """include/vocr.h's per-element bound of an fp16x3 dot product, float64: a [m][k], b [n][k]; amax / bmax: the maxima of the plane sets'
    rows where the product is a k window of longer rows"""
    a, b = a.double(), b.double()
    amax = a.abs().max(1).values if amax is None else amax.double()
    bmax = b.abs().max(1).values if bmax is None else bmax.double()
    return 2.0 ** -22 * (a.abs() @ b.abs().t()) + k * 2.0 ** -39 * amax[:, None] * bmax[None, :]


def check(scheme, kind, got, ref, a=None, b=None, k=0, with_bias=False, amax=None, bmax=None):
    """None if `got` (fp32) meets the scheme's bar for the kind against the float64 `ref`, else what is wrong.  Also returns the error as a
    fraction of the scale for floats: (message or None, max |got - ref| / max |ref| or None)."""
    got, ref = torch.as_tensor(got), torch.as_tensor(ref)
    if kind == "floats":
        scale = float(ref.abs().max())
        err = float((got.double() - ref).abs().max())
        rel = err / scale if err == err else float("inf")
        return (None if rel <= gr.FLOAT_BAR else "max abs error %.3e at scale %.3e (bar %.1e x scale)" % (err, scale, gr.FLOAT_BAR)), rel
    if kind in EXACT[scheme]:
        want = ref.float()
        if torch.equal(got, want):
            return None, None
        bad = torch.nonzero(~(got == want))
        r, q = int(bad[0][0]), int(bad[0][1])
        return "%d of %d elements differ from float64; first at [%d][%d]: got %r, want %r" % (bad.shape[0], want.numel(), r, q, float(got[r, q]),
                                                                                              float(want[r, q])), None
    dv = ref.device
    bound = h3_bound(a.to(dv), b.to(dv), k, None if amax is None else amax.to(dv), None if bmax is None else bmax.to(dv))
    if with_bias:
        bound = bound + 2.0 ** -24 * ref.abs()
    err = (got.double() - ref).abs()
    if bool((err <= bound).all()):
        return None, None
    over = torch.nan_to_num(err / bound.clamp_min(1e-300), nan=float("inf"))
    return "%d elements above the fp16x3 bound, worst %.3f x the bound" % (int((~(err <= bound)).sum()), float(over.max())), None


# ---------------------------------------------------------------------------------------------------------------- fragment decoder
def rt_of(rows):
    return (rows + 255) // 256 * 8


def kk_of(k):
    return (k + 31) // 32 * 2


def planes_bytes(scheme, rows, k):
    return NPLANES[scheme] * rt_of(rows) * kk_of(k) * 1024 + (rt_of(rows) * 32 * 4 if scheme == "fp16x3" else 0)


def decode(buf, scheme, rows, k):
    """A plane set (a byte / int16 tensor that starts at the planes) -> (planes [NP][padded rows][padded k] float64 on the CPU, the fp16x3 rows'
    maxima [padded rows] fp32 or None).  Fragment order: plane[p][row tile][k16 step][lane][8], lane (r = lane & 31, h = lane >> 5) holds
    X[32 rt + r][16 kk + 8 h + 0 .. 7]."""
    NP, RT, KK = NPLANES[scheme], rt_of(rows), kk_of(k)
    raw = buf.view(torch.uint8)[:planes_bytes(scheme, rows, k)]
    nb = NP * RT * KK * 1024
    el = raw[:nb].view(torch.bfloat16 if scheme == "bf16x6" else torch.float16)
    p = el.view(NP, RT, KK, 2, 32, 8).permute(0, 1, 4, 2, 3, 5).reshape(NP, RT * 32, KK * 16).double().cpu()
    amax = raw[nb:].view(torch.float32).cpu() if scheme == "fp16x3" else None
    return p, amax


# ---------------------------------------------------------------------------------------------------------------- numpy emulation
def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even) as fp32, by bit operations; the largest finite magnitudes, which would round to infinity, are
    truncated instead (as the split kernels do)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    t = (u & 0xFFFF0000).astype(np.uint32)
    special = (u & 0x7F800000) == 0x7F800000                        # Inf / NaN stay what they are
    overflow = ((r & 0x7FFFFFFF) == 0x7F800000) & ~special
    return np.where(special | overflow, t, r).astype(np.uint32).view(np.float32)


def split_bf16x6(x):
    x = np.asarray(x, dtype=np.float32)
    p0 = bf16_rne(x)
    r1 = x - p0
    p1 = bf16_rne(r1)
    p2 = bf16_rne(r1 - p1)
    return [p0, p1, p2], None


def h3_scale_exp(amax):
    e = (np.asarray(amax, dtype=np.float32).view(np.uint32) >> 23) & 0xFF
    return np.minimum(268 - e.astype(np.int64), 253)


def split_fp16x3(x):
    x = np.asarray(x, dtype=np.float32)
    amax = np.abs(x).max(1).astype(np.float32)
    se = h3_scale_exp(amax)
    s = np.ldexp(np.float32(1), (se - 127).astype(np.int32)).astype(np.float32)
    xs = (x * s[:, None]).astype(np.float32)
    with np.errstate(over="ignore"):
        h0 = xs.astype(np.float16)
        h1 = (xs - h0.astype(np.float32)).astype(np.float32).astype(np.float16)
    inv = np.ldexp(np.float32(1), (127 - se).astype(np.int32)).astype(np.float32)
    return [h0.astype(np.float32), h1.astype(np.float32)], inv


# (A plane, B plane) in the order the product kernel issues its MFMAs within a k16 step
PRODUCTS = {"bf16x6": ((1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0)), "fp16x3": ((0, 1), (1, 0), (0, 0))}


def emulate(scheme, a, b, drop=(), zero_a=(), zero_b=()):
    """C = A . B^T as the kernel forms it: the operands split into planes, per k16 step the scheme's partial products in the kernel's order, each
    a 16-term dot product (exact products, summed in float64 here) added to an fp32 accumulator; fp16x3 undoes the rows' scales at the end.
    drop: partial products (A plane, B plane) left out; zero_a / zero_b: planes of A / B replaced by zeros."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    m, k = a.shape
    kp = (k + 15) // 16 * 16
    a = np.pad(a, ((0, 0), (0, kp - k)))
    b = np.pad(b, ((0, 0), (0, kp - k)))
    pa, ia = (split_bf16x6 if scheme == "bf16x6" else split_fp16x3)(a)
    pb, ib = (split_bf16x6 if scheme == "bf16x6" else split_fp16x3)(b)
    pa = [np.zeros_like(p) if i in zero_a else p for i, p in enumerate(pa)]
    pb = [np.zeros_like(p) if i in zero_b else p for i, p in enumerate(pb)]
    acc = np.zeros((m, b.shape[0]), dtype=np.float32)
    for s in range(kp // 16):
        ks = slice(16 * s, 16 * s + 16)
        for (i, j) in PRODUCTS[scheme]:
            if (i, j) in drop:
                continue
            acc = (acc.astype(np.float64) + pa[i][:, ks].astype(np.float64) @ pb[j][:, ks].astype(np.float64).T).astype(np.float32)
    if scheme == "fp16x3":
        acc = (acc * ia[:, None]).astype(np.float32) * ib[None, :]
    return acc.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the case table
class Case(object):
    """One product: C[m][n] = A[a_row0 .., 16 a_kk0 ..] . B[b_row0 .., 16 b_kk0 ..]^T from plane sets written for (a_row0 + m + a_extra rows,
    16 a_kk0 + k) and (b_rows or b_row0 + n rows, 16 b_kk0 + k), and the path it must take on 256 CUs.

    path: "<narrow|wide>/<whole|cut|rounds+cut>" (256 x 128 or 256 x 256 tiles; one launch over the whole K, every tile cut along K, or whole
          rounds + a K-cut remainder), " wide-refused" behind it when the wide tile was not admissible.
    plan: exact vocr_gemm_x6_plan fields the case is about.  ws: the call gets a workspace.  two: b_row0 of the second view of a _two_views
    call (rows >= rsplit; its k16 offsets are the first view's, swapped), else None.
    what: the category the row is in the table for (tests/test_x6_plan_cpu.py requires every one of CATEGORIES to be present)."""

    def __init__(self, name, what, m, n, k, path, kinds=KINDS, epis=("none",), plan=None, ws=True, csplit=0, rsplit=0, a_row0=0, a_kk0=0, b_row0=0,
                 b_kk0=0, b_rows=None, two=None):
        self.name, self.what, self.m, self.n, self.k, self.path = name, what, m, n, k, path
        self.kinds, self.epis, self.plan, self.ws = tuple(kinds), tuple(epis), dict(plan or {}), ws
        self.csplit, self.rsplit, self.a_row0, self.a_kk0, self.b_row0, self.b_kk0, self.two = csplit, rsplit, a_row0, a_kk0, b_row0, b_kk0, two
        self.k16 = (k + 15) // 16 * 16
        assert not (a_kk0 or b_kk0 or two is not None) or k % 16 == 0
        # a view that starts late still reads whole 256-row / 128-column blocks of fragments: the plane sets hold that many (filler) rows
        self.a_rows, self.a_k = a_row0 + (256 * ((m + 255) // 256) if a_row0 else m), 16 * max(a_kk0, b_kk0 if two is not None else 0) + k
        b0 = max(b_row0, two or 0)
        self.b_rows = b_rows if b_rows is not None else b0 + (128 * ((n + 127) // 128) if b0 else n)
        self.b_k = 16 * max(b_kk0, a_kk0 if two is not None else 0) + k

    def __repr__(self):
        return self.name

    def ask(self, ops):
        return ops.gemm_x6_plan(self.m, self.n, self.k16, b_rows=self.b_rows, b_row0=self.b_row0, b_row0_2=-1 if self.two is None else self.two,
                                workspace=self.ws)


def path_of(plan):
    """the path name of a vocr_gemm_x6_plan answer (ops.gemm_x6_plan's dict)"""
    form = "whole" if plan["cut_tiles"] == 0 else ("cut" if plan["whole_tiles"] == 0 else "rounds+cut")
    return "%s/%s%s" % ({4: "narrow", 8: "wide"}[plan["tile"]], form, "" if plan["wide_ok"] else " wide-refused")


def path_problem(case, plan):
    """None if the plan is the path (and the exact plan fields) the case is about, else a sentence that names the plan"""
    if path_of(plan) != case.path:
        return "%s: the call takes %s, the case is about %s (plan %r)" % (case, path_of(plan), case.path, plan)
    for key, val in case.plan.items():
        if plan[key] != val:
            return "%s: %s = %r, the case is about %r (plan %r)" % (case, key, plan[key], val, plan)
    return None


CATEGORIES = ("short K narrow", "short K wide", "ragged", "cut 16 cap", "cut nkk/8 cap", "cut uneven", "cut fewer splits", "no workspace",
              "rounds+cut narrow", "rounds+cut wide", "wide cut", "wide refused", "epilogue direct", "epilogue reduce", "csplit direct",
              "csplit reduce", "rsplit direct", "rsplit reduce", "view a_row0", "view kk0", "view b_row0", "two views whole", "two views cut",
              "nonfinite direct", "nonfinite cut")
LARGE = ("ints", "floats", "sel12B")                 # the kinds of the large shapes
ALL_EPI = tuple(EPILOGUES)


def _cases():
    c = []
    add = lambda *a, **k: c.append(Case(*a, **k))
    # ---- short K: fewer k16 stages than the DMA ring has slots (4 / 3 for bf16x6 on the narrow / wide tile, 6 / 4 for fp16x3) .. one more.
    # One narrow tile; 8192 x 2048 = 256 wide tiles = one whole round, nothing to cut (and K < 512 is never cut)
    for k in (16, 32, 48, 64, 80, 96, 112):
        add("short narrow k%d" % k, "short K narrow", 200, 100, k, "narrow/whole", plan={"tiles": 1, "stages_per_split": k // 16})
    for k in (16, 32, 48, 64, 80, 96):
        add("short wide k%d" % k, "short K wide", 8192, 2048, k, "wide/whole", kinds=LARGE, plan={"tiles": 256, "stages_per_split": k // 16})
    # ---- ragged edges: grids of 1, 3, 4, 6, 9 and 5 x 3 workgroups (none a multiple of 8; 5 row tiles: a last panel of ONE row tile), K = 1 .. 40
    for (m, n, k, tiles) in ((1, 1, 1, 1), (255, 127, 7, 1), (1, 257, 17, 3), (257, 129, 33, 4), (255, 257, 40, 3), (257, 255, 9, 4), (257, 257, 31, 6),
                             (600, 300, 24, 9), (1100, 257, 40, 15)):
        add("ragged %dx%dx%d" % (m, n, k), "ragged", m, n, k, "narrow/whole", plan={"tiles": tiles, "whole_tiles": tiles})
    # ---- every tile cut along K (the remainder rule: at most half a round of tiles, K >= 512, a workspace)
    add("cut 16 cap", "cut 16 cap", 257, 129, 4096, "narrow/cut", plan={"cut_tiles": 4, "ksplit": 16, "stages_per_split": 16})
    add("cut nkk/8 cap", "cut nkk/8 cap", 257, 129, 512, "narrow/cut", plan={"cut_tiles": 4, "ksplit": 4, "stages_per_split": 8})
    add("cut uneven", "cut uneven", 257, 129, 528, "narrow/cut", plan={"ksplit": 4, "stages_per_split": 9})          # 33 stages: 9 + 9 + 9 + 6
    # 129 stages, 16 splits planned: 9 stages each are 15 splits (the last with 3)
    add("cut fewer splits", "cut fewer splits", 255, 127, 2064, "narrow/cut", plan={"cut_tiles": 1, "ksplit": 15, "stages_per_split": 9})
    add("cut uneven no ws", "no workspace", 257, 129, 528, "narrow/whole", ws=False, plan={"whole_tiles": 4, "ksplit": 1})
    # ---- whole rounds + a K-cut remainder in ONE call (tile0 > 0): 33 x 8 narrow tiles = 256 + 8 four ways; 33 x 8 wide tiles = 256 + 8 five
    # ways (at K = 512 the same shape is cheaper as two rounds + 16 of narrow tiles: the wide tile needs 5 splits to win, 40 k16 stages)
    add("rounds+cut narrow", "rounds+cut narrow", 8448, 1024, 512, "narrow/rounds+cut", kinds=LARGE,
        plan={"whole_tiles": 256, "cut_tiles": 8, "ksplit": 4})
    add("rounds+cut wide", "rounds+cut wide", 8448, 2048, 640, "wide/rounds+cut", kinds=LARGE, plan={"whole_tiles": 256, "cut_tiles": 8, "ksplit": 5})
    # ---- the wide tile cut along K: 64 wide tiles four ways
    add("wide cut", "wide cut", 2048, 2048, 512, "wide/cut", kinds=LARGE, plan={"cut_tiles": 64, "ksplit": 4})
    add("wide cut ragged", "wide cut", 2047, 2040, 520, "wide/cut", kinds=LARGE, plan={"cut_tiles": 64, "ksplit": 4, "stages_per_split": 9})
    # ---- the wide tile refused: B's view starts at row 128 of a 2304-row plane set, 9 blocks of 8 column tiles would end at tile 76 of 72.
    # (the test multiplies the same rows from a plane set of their own, where the wide tile is taken, and without a workspace, where it is not)
    add("wide refused", "wide refused", 2048, 2176, 512, "narrow/whole wide-refused", kinds=LARGE, b_row0=128, b_rows=2304, plan={"whole_tiles": 136})
    # ---- epilogues and output cuts through the direct store (K = 48) and through the reduce kernel (K = 512); the cuts fall inside a 32-block
    for k, how in ((48, "direct"), (512, "reduce")):
        path = "narrow/whole" if how == "direct" else "narrow/cut"
        add("epilogues %s" % how, "epilogue %s" % how, 257, 257, k, path, epis=ALL_EPI)
        add("csplit 100 %s" % how, "csplit %s" % how, 257, 257, k, path, epis=("none", "bias_relu"), csplit=100)
        add("rsplit 100 %s" % how, "rsplit %s" % how, 257, 257, k, path, epis=("none", "bias"), rsplit=100)
    # ---- views: rows of A from 32, of B from 32, odd k16 offsets; uncut and cut
    for k, path in ((48, "narrow/whole"), (512, "narrow/cut")):
        add("view a_row0 k%d" % k, "view a_row0", 257, 129, k, path, a_row0=32)
        add("view kk0 k%d" % k, "view kk0", 257, 129, k, path, a_kk0=3, b_kk0=1)
        add("view b_row0 k%d" % k, "view b_row0", 257, 129, k, path, b_row0=32)
    # ---- two products in one launch (rows >= 256 read other views), against two single-view calls
    add("two views whole", "two views whole", 512, 129, 48, "narrow/whole", rsplit=256, a_kk0=1, b_row0=0, b_kk0=0, two=160, kinds=("ints", "floats"))
    add("two views cut", "two views cut", 512, 129, 1024, "narrow/cut", rsplit=256, a_kk0=1, b_row0=0, b_kk0=0, two=160, kinds=("ints", "floats"),
        plan={"cut_tiles": 4, "ksplit": 8})
    # ---- one NaN / Inf element poisons its output row (A) or column (B), and nothing else
    add("nonfinite direct", "nonfinite direct", 257, 129, 48, "narrow/whole", kinds=("floats",))
    add("nonfinite cut", "nonfinite cut", 257, 129, 512, "narrow/cut", kinds=("floats",))
    return c


CASES = _cases()
PRODUCT_CASES = [c for c in CASES if c.two is None and not c.what.startswith(("nonfinite", "wide refused"))]


def case_named(name):
    return [c for c in CASES if c.name == name][0]
