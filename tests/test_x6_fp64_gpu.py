"""GPU: the split-operand GEMMs of gemm_x6.hip - vocr_gemm_x6* ("bf16x6") and vocr_gemm_h3* ("fp16x3") - against float64 on every launch path.

Each row of tests/x6_ref.py's table is named for one path (narrow / wide tile x whole K / K cut / whole rounds + a cut remainder, the wide tile
refused by a late view).  A test first asks vocr_gemm_x6_plan - the planner the entry points launch from - on the device it runs on and fails,
naming the plan, if the row does not take its path there; then it runs the data kinds of tests/x6_ref.py at their bars (bit-exact integers and
selectors, N(0,1) floats at gemm_ref.FLOAT_BAR, fp16x3's selectors at include/vocr.h's per-element bound), twice (bitwise reproducible), from
sources whose row gaps hold NaN, into a C with ldc > n inside sentinel memory, with a NaN workspace of exactly the bytes the plan names and a
sentinel behind it.  The split kernels are tested apart: the planes against the operand for both source orders at every row / K edge, the
padding, the bytes behind the plane set.  Worst float errors per scheme and path: profiles/gemm_x6_fp64_errors.txt."""
import ctypes

import pytest
import torch

from tests import gemm_ref as gr
from tests import x6_ref as xr

pytestmark = pytest.mark.gpu
TAIL = 256                                            # sentinel bytes behind a plane set
FILL = 0xA5
ENTRY = {"bf16x6": ("vocr_gemm_x6_planes_bytes", "vocr_gemm_x6_split", "vocr_gemm_x6", "vocr_gemm_x6_two_views"),
         "fp16x3": ("vocr_gemm_h3_planes_bytes", "vocr_gemm_h3_split", "vocr_gemm_h3", "vocr_gemm_h3_two_views")}


@pytest.fixture(scope="module")
def dev():
    from vistaocr_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _ptr(t):
    return ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------- plane sets
class Planes(object):
    """A plane set of exactly vocr_gemm_*_planes_bytes with a sentinel behind it; the planes start out as the sentinel too (non-zero 16-bit
    values: padding that reads zero afterwards was written)."""

    def __init__(self, scheme, rows, k, dev):
        from vistaocr_amd import _lib
        self.scheme, self.rows, self.k = scheme, rows, k
        self.nb = xr.planes_bytes(scheme, rows, k)
        assert self.nb == getattr(_lib.load(), ENTRY[scheme][0])(rows, k)
        self.buf = torch.full((self.nb + TAIL,), FILL, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0

    def tail_untouched(self):
        return bool((self.buf[self.nb:] == FILL).all())

    def decode(self):
        return xr.decode(self.buf, self.scheme, self.rows, self.k)


def _split(scheme, dev, x, ld, rows, k, kc, x2=None, seg=0, axis=0, mask=None, bound=0.0):
    """x, x2, mask: device addresses (int) or tensors"""
    from vistaocr_amd import _lib
    p = Planes(scheme, rows, k, dev)
    args = [_ptr(x), _ptr(x2), int(seg), int(axis), _ptr(mask), int(ld), int(rows), int(k), int(bool(kc))]
    if scheme == "fp16x3":
        args.append(float(bound))
    _lib.call(ENTRY[scheme][1], *(args + [_ptr(p.buf), _stream()]))
    return p


def _source(mat, kc, dev, offset=0, extra_ld=4):
    """the [rows][k] matrix as a K-contiguous ([rows][k]) or K-strided ([k][rows]) source with NaN row gaps and guards"""
    src = mat if kc else mat.t().contiguous()
    return gr.Padded(src, src.shape[1] + extra_ld, offset, dev)


def _planes_of(scheme, mat, kc, dev):
    rows, k = mat.shape
    s = _source(mat, kc, dev)
    p = _split(scheme, dev, s.ptr, s.ld, rows, k, kc)
    assert p.tail_untouched(), "the split wrote behind its plane set"
    return p


def _wide_range(rows, k, g):
    """all 24 significand bits in use, +-4 decades inside a row, +-10 decades between rows"""
    x = gr._full_mantissa((rows, k), g)
    x = x * torch.pow(10.0, (torch.rand(rows, k, generator=g) - 0.5) * 8.0) * torch.pow(10.0, (torch.rand(rows, 1, generator=g) - 0.5) * 20.0)
    return x.float()


def _absmax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _assert_split(p, x, what):
    """p: the plane set the split made of the [rows][k] matrix x (CPU, what the source holds after the mask)"""
    rows, k = x.shape
    planes, amax = p.decode()
    assert bool(torch.isfinite(planes).all()), what + ": a non-finite value reached a plane"
    assert p.tail_untouched(), what + ": the bytes behind the plane set were written"
    rec = planes.sum(0)
    assert _absmax(planes[:, rows:]) == 0.0 and _absmax(planes[:, :, k:]) == 0.0, what + ": padding is not zero"
    xd = x.double()
    if p.scheme == "bf16x6":
        assert torch.equal(rec[:rows, :k].float(), x) and torch.equal(rec[:rows, :k], xd), what + ": the three planes do not sum to the operand"
        return
    assert amax.numel() == planes.shape[1] and torch.equal(amax[:rows], x.abs().max(1).values), what + ": stored maxima are not the rows' maxima"
    assert _absmax(amax[rows:]) == 0.0, what + ": maxima of padding rows"
    am = amax[:rows].double().unsqueeze(1)
    e = torch.floor(torch.log2(torch.clamp(am, min=1e-300)))
    scale = torch.where(am > 0, torch.pow(2.0, 14.0 - e), torch.ones_like(am))
    if bool((am > 0).any()):
        assert float((am * scale)[am > 0].min()) >= 2.0 ** 14 and float((am * scale).max()) < 2.0 ** 15, what + ": the scale"
    err = (rec[:rows, :k] / scale - xd).abs()
    bound = torch.maximum(xd.abs() * 2.0 ** -22, am * 2.0 ** -39)
    assert bool((err <= bound).all()), "%s: %.3f x the representation bound" % (what, float((err / torch.clamp(bound, min=1e-300)).max()))


ROWS = (1, 31, 32, 33, 255, 256, 257)
KS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33)


@pytest.mark.parametrize("kc", [True, False], ids=["rk", "kr"])
@pytest.mark.parametrize("scheme", xr.SCHEMES)
def test_split_at_every_row_and_k_edge(dev, scheme, kc):
    """rows around the 32-row fragment and the 256-row padding, k around the 8 of a lane, the 16 of a fragment and the 32 of the padding; the
    source has ld > its row length with NaN in the gaps; every shape also from a source 4 bytes off 16-byte alignment (K-contiguous: the
    scalar-load branch)."""
    g = torch.Generator().manual_seed(21)
    for rows in ROWS:
        for k in KS:
            x = _wide_range(rows, k, g)
            if rows > 2:
                x[1] = 0.0                                                                # an all-zero row
            for off in (0, 1):
                s = _source(x, kc, dev, offset=off)
                assert s.ptr % 16 == 4 * off
                _assert_split(_split(scheme, dev, s.ptr, s.ld, rows, k, kc), x, "%s %s %dx%d off %d" % (scheme, "rk" if kc else "kr", rows, k, off))


@pytest.mark.parametrize("scheme", xr.SCHEMES)
def test_split_of_long_k_contiguous_rows(dev, scheme):
    """k around the 2048 one wave of the fp16x3 row-maximum pass covers: the maximum sits in the last chunk, at the chunk boundary or in the first"""
    g = torch.Generator().manual_seed(22)
    rows = 33
    for k in (2047, 2048, 2049, 2056):
        x = _wide_range(rows, k, g)
        big = x.abs().max(1).values * 3.0
        for r in range(rows):
            x[r, (k - 1, min(2047, k - 1), min(2048, k - 1), 5)[r % 4]] = big[r]
        for off in (0, 1):
            s = _source(x, True, dev, offset=off)
            _assert_split(_split(scheme, dev, s.ptr, s.ld, rows, k, True), x, "%s rk %dx%d off %d" % (scheme, rows, k, off))


@pytest.mark.parametrize("kc", [True, False], ids=["rk", "kr"])
@pytest.mark.parametrize("scheme", xr.SCHEMES)
def test_split_of_two_piece_sources(dev, scheme, kc):
    """the second piece starts at k = seg (axis 0) or at row = seg (axis 1): seg = 8 inside a k16 step / a 32-row tile, seg = 40 past the first"""
    g = torch.Generator().manual_seed(23)
    rows, k = 70, 50
    for axis in (0, 1):
        for seg in (8, 40):
            x = _wide_range(rows, k, g)
            first, second = (x[:, :seg], x[:, seg:]) if axis == 0 else (x[:seg], x[seg:])
            first, second = (first, second) if kc else (first.t(), second.t())
            ld = max(first.shape[1], second.shape[1]) + 4
            s1, s2 = gr.Padded(first.contiguous(), ld, 0, dev), gr.Padded(second.contiguous(), ld, 0, dev)
            p = _split(scheme, dev, s1.ptr, ld, rows, k, kc, x2=s2.ptr, seg=seg, axis=axis)
            _assert_split(p, x, "%s %s axis %d seg %d" % (scheme, "rk" if kc else "kr", axis, seg))


@pytest.mark.parametrize("scheme", xr.SCHEMES)
def test_split_with_the_mask_on_the_read(dev, scheme):
    """the mask has the source's addressing (ld > k): its row gaps hold NaN too"""
    g = torch.Generator().manual_seed(24)
    for rows, k in ((70, 50), (33, 17), (257, 32)):
        x = _wide_range(rows, k, g)
        mask = (torch.rand(rows, k, generator=g) > 0.5).float() * 2.0
        for off in (0, 1):
            s, mk = _source(x, True, dev, offset=off), _source(mask, True, dev, offset=off)
            assert s.ld == mk.ld
            p = _split(scheme, dev, s.ptr, s.ld, rows, k, True, mask=mk.ptr)
            _assert_split(p, x * mask, "%s masked %dx%d off %d" % (scheme, rows, k, off))


def _extremes():
    """fp32 magnitudes at the ends of the range, all with the lowest significand bit set"""
    def bits(lo, hi, n, g):
        u = torch.randint(lo, hi, (n,), generator=g, dtype=torch.int64) | 1
        sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int64) << 31
        u = u | sign
        return torch.where(u >= (1 << 31), u - (1 << 32), u).to(torch.int32).view(torch.float32)
    g = torch.Generator().manual_seed(25)
    e = lambda x: (x + 127) << 23
    return {"fp32 denormals": bits(1, 1 << 23, 512, g),
            "2^-126 .. 2^-110": bits(e(-126), e(-110), 512, g),
            "2^-110 .. 2^-108": bits(e(-110), e(-108), 512, g),
            "2^127 (2 - 2^-7) .. 2^127 (2 - 2^-8)": bits(0x7F7E0000, 0x7F7F8000, 512, g),
            "2^127 (2 - 2^-8) .. max": torch.cat([bits(0x7F7F8000, 0x7F800000, 508, g),
                                                  torch.tensor([0x7F7F8000, 0x7F7FFFFF, -0x00800001, -0x00807FFF - 1], dtype=torch.int32).view(torch.float32)])}


@pytest.mark.parametrize("kc", [True, False], ids=["rk", "kr"])
def test_bf16x6_split_at_the_ends_of_the_fp32_range(dev, kc):
    """include/vocr.h: the three planes sum to the operand EXACTLY for every finite |a| >= 2^-110 (at the top of the range, where rounding the
    first plane to nearest would overflow bf16, it is taken by truncation); below 2^-110 the last plane is a bf16 denormal, whose step 2^-133
    is coarser than the operand's: the sum is the operand rounded to a multiple of 2^-133, |error| <= 2^-134 (fp32 denormals included)."""
    for name, v in _extremes().items():
        x = v.reshape(16, 32).clone()
        planes, _ = _planes_of("bf16x6", x, kc, dev).decode()
        assert bool(torch.isfinite(planes).all()), name + ": a non-finite plane"
        err = (planes.sum(0)[:16, :32] - x.double()).abs()
        print("X6_EXTREME | %s | %s | max |sum of planes - a| = %.3e (2^-134 = %.3e), planes with a denormal value: %s"
              % ("rk" if kc else "kr", name, float(err.max()), 2.0 ** -134,
                 [bool(((planes[i].abs() > 0) & (planes[i].abs() < 2.0 ** -126)).any()) for i in range(3)]))
        if name in ("fp32 denormals", "2^-126 .. 2^-110"):
            assert float(err.max()) <= 2.0 ** -134, (name, float(err.max()))
        else:
            assert float(err.max()) == 0.0, (name, float(err.max()))


@pytest.mark.parametrize("scheme", xr.SCHEMES)
def test_product_with_a_tiny_operand(dev, scheme):
    """A = 12-bit odd integers x 2^-130 (below 2^-110: the second bf16 plane is a denormal), B = 12-bit odd integers x 2^100, one product per
    output: exact in fp32 (x 2^-30) if the matrix pipe takes denormal bf16 inputs as they are.  fp16x3 scales every row first and is held to its
    per-element bound, as on every selector kind."""
    m, n, k = 70, 50, 48
    a, b, _, ab = xr.make_data("sel12A", m, n, k, 31)
    a, b, ab = a * 2.0 ** -130, b * 2.0 ** 100, ab * 2.0 ** -30
    pa, pb = _planes_of(scheme, a, True, dev), _planes_of(scheme, b, False, dev)
    def run():
        C = [gr.Padded(None, n + 12, 0, dev, sentinel=True, shape=(m, n))]
        _gemm(scheme, dev, pa, pb, m, n, k, C, ldc=n + 12)
        return C
    c = _twice(run)[0]
    got, want = c.view.cpu(), ab.float()
    print("X6_EXTREME | %s | tiny operand product: %d of %d elements differ, max relative error %.3e"
          % (scheme, int((got != want).sum()), want.numel(), float(((got.double() - ab).abs() / ab.abs().clamp_min(1e-300)).max())))
    msg, _ = xr.check(scheme, "sel12A", got, ab, a, b, k)
    assert msg is None and c.outside_untouched(), msg


# ---------------------------------------------------------------------------------------------------------------- products
class Workspace(object):
    """NaN of exactly the bytes the plan names, a sentinel behind it"""

    def __init__(self, nbytes, dev):
        assert nbytes % 4 == 0
        self.n = nbytes // 4
        self.buf = torch.full((self.n + gr.GUARD,), float("nan"), device=dev)
        self.buf[self.n:] = torch.full((1,), gr.SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)

    def tail_untouched(self):
        return bool((self.buf[self.n:].view(torch.int32) == gr.SENTINEL).all())


def _guarded(vec, dev):
    """a vector between NaN guards"""
    buf = torch.full((gr.GUARD + vec.numel() + gr.GUARD,), float("nan"), device=dev)
    buf[gr.GUARD:gr.GUARD + vec.numel()] = vec.to(dev)
    return buf[gr.GUARD:gr.GUARD + vec.numel()]


def _gemm(scheme, dev, pa, pb, m, n, k16, C, ldc, a_row0=0, a_kk0=0, b_row0=0, b_kk0=0, csplit=0, rsplit=0, biases=(None, None), relu=0, ws=True,
          plan=None, two=None):
    """One call of the scheme's product (two: (a_kk0_2, b_row0_2, b_kk0_2) = the two-view form) on a fresh NaN workspace of the plan's size"""
    from vistaocr_amd import _lib, ops
    if plan is None:
        plan = ops.gemm_x6_plan(m, n, k16, b_rows=pb.rows, b_row0=b_row0, b_row0_2=-1 if two is None else two[1], workspace=ws)
    w = Workspace(plan["workspace_bytes"], dev) if ws else None
    c1 = _ptr(C[1].ptr) if len(C) > 1 else None
    if two is None:
        _lib.call(ENTRY[scheme][2], _ptr(pa.buf), pa.rows, pa.k, a_row0, a_kk0, _ptr(pb.buf), pb.rows, pb.k, b_row0, b_kk0, m, n, k16, _ptr(C[0].ptr), c1,
                  csplit, rsplit, ldc, _ptr(biases[0]), _ptr(biases[1]), relu, _ptr(w.buf) if w else None, _stream())
    else:
        _lib.call(ENTRY[scheme][3], _ptr(pa.buf), pa.rows, pa.k, a_row0, _ptr(pb.buf), pb.rows, pb.k, m, n, k16, rsplit, a_kk0, b_row0, b_kk0,
                  two[0], two[1], two[2], _ptr(C[0].ptr), c1, ldc, _ptr(w.buf) if w else None, _stream())
    assert w is None or w.tail_untouched(), "the product wrote behind the %d workspace bytes its plan names" % plan["workspace_bytes"]
    return plan


def _twice(run):
    """run() -> the Padded outputs of one call: two calls whose buffers must be bit-identical; the first call's outputs"""
    first, second = run(), run()
    for c, c2 in zip(first, second):
        assert torch.equal(c.buf.view(torch.int32), c2.buf.view(torch.int32)), "two runs differ"
    return first


def _embed(mat, rows, cols, r0, c0, g):
    """mat inside a [rows][cols] matrix of other integers (what a view must not read)"""
    full = torch.randint(-8, 9, (rows, cols), generator=g).float()
    full[r0:r0 + mat.shape[0], c0:c0 + mat.shape[1]] = mat
    return full


def _outputs(case, dev):
    m, n, ldc = case.m, case.n, case.n + 12
    if case.csplit:
        shapes = [(m, case.csplit), (m, n - case.csplit)]
    elif case.rsplit:
        shapes = [(case.rsplit, n), (m - case.rsplit, n)]
    else:
        shapes = [(m, n)]
    return [gr.Padded(None, ldc, 0, dev, sentinel=True, shape=s) for s in shapes], ldc


def _joined(case, C):
    if len(C) == 1:
        return C[0].view
    return torch.cat([C[0].view, C[1].view], 1 if case.csplit else 0)


def _assert_path(case):
    from vistaocr_amd import ops
    plan = case.ask(ops)
    problem = xr.path_problem(case, plan)
    assert problem is None, problem
    return plan


def _case_data(case, kind, seed, dev):
    """the product's operands inside their plane sets' matrices (CPU), bias, the float64 product on the device"""
    g = torch.Generator().manual_seed(seed + 1)
    a, b, bias, ab = xr.make_data(kind, case.m, case.n, case.k, seed, dense_product=False)
    ab = (a.to(dev).double() @ b.to(dev).double().t()) if ab is None else ab.to(dev)
    af = _embed(a, case.a_rows, case.a_k, case.a_row0, 16 * case.a_kk0, g)
    bf = _embed(b, case.b_rows, case.b_k, case.b_row0, 16 * case.b_kk0, g)
    if not (case.a_kk0 or case.b_kk0):
        assert af.shape[1] == case.k and bf.shape[1] == case.k
    return a, b, bias, ab, af, bf


def _run_case(case, scheme, dev, record):
    plan = _assert_path(case)                             # the path first, the values after
    for ki, kind in enumerate(case.kinds):
        a, b, bias, ab, af, bf = _case_data(case, kind, 3000 + 17 * ki, dev)
        pa, pb = _planes_of(scheme, af, True, dev), _planes_of(scheme, bf, ki % 2 == 1, dev)
        amax = af[case.a_row0:case.a_row0 + case.m].abs().max(1).values
        bmax = bf[case.b_row0:case.b_row0 + case.n].abs().max(1).values
        cs = case.csplit if case.csplit else case.n
        for epi in case.epis:
            has_bias, relu = xr.EPILOGUES[epi]
            biases = (_guarded(bias[:cs], dev), _guarded(bias[cs:], dev) if case.csplit else None) if has_bias else (None, None)
            what = "%s, %s, %s, %s" % (case, scheme, kind, epi)
            runs = []
            for _ in range(2):
                C, ldc = _outputs(case, dev)
                _gemm(scheme, dev, pa, pb, case.m, case.n, case.k16, C, ldc, a_row0=case.a_row0, a_kk0=case.a_kk0, b_row0=case.b_row0, b_kk0=case.b_kk0,
                      csplit=case.csplit, rsplit=case.rsplit, biases=biases, relu=relu, ws=case.ws, plan=plan)
                runs.append(C)
            for c, c2 in zip(*runs):
                assert torch.equal(c.buf.view(torch.int32), c2.buf.view(torch.int32)), what + ": two runs differ"
                assert c.outside_untouched(), what + ": a row gap or guard band of C was written"
            msg, rel = xr.check(scheme, kind, _joined(case, runs[0]), xr.reference(ab, bias, epi), a, b, case.k, with_bias=bool(has_bias), amax=amax,
                                bmax=bmax)
            if rel is not None:
                record(scheme, case, rel)
            assert msg is None, "%s: %s" % (what, msg)


def _record(scheme, case, rel):
    print("X6_ERR | %s | %s | %s | %.3e" % (scheme, case.path, case.name, rel))


@pytest.mark.parametrize("scheme", xr.SCHEMES)
@pytest.mark.parametrize("case", xr.PRODUCT_CASES, ids=[c.name.replace(" ", "_") for c in xr.PRODUCT_CASES])
def test_product_case(dev, case, scheme):
    _run_case(case, scheme, dev, _record)


@pytest.mark.parametrize("scheme", xr.SCHEMES)
def test_no_workspace_gives_the_cut_products_result(dev, scheme):
    """the same shape with and without a workspace: K cut four ways / uncut; bit-equal wherever the data is exact, both at the bar on floats"""
    cut, whole = xr.case_named("cut uneven"), xr.case_named("cut uneven no ws")
    assert (cut.m, cut.n, cut.k) == (whole.m, whole.n, whole.k)
    p_cut, p_whole = _assert_path(cut), _assert_path(whole)
    for ki, kind in enumerate(cut.kinds):
        a, b, bias, ab, af, bf = _case_data(cut, kind, 3100 + ki, dev)
        pa, pb = _planes_of(scheme, af, True, dev), _planes_of(scheme, bf, False, dev)
        out = []
        for case, plan in ((cut, p_cut), (whole, p_whole)):
            def run():
                C, ldc = _outputs(case, dev)
                _gemm(scheme, dev, pa, pb, case.m, case.n, case.k16, C, ldc, ws=case.ws, plan=plan)
                return C
            C = _twice(run)
            msg, _ = xr.check(scheme, kind, C[0].view, ab, a, b, case.k)
            assert msg is None and C[0].outside_untouched(), "%s, %s, %s: %s" % (case, scheme, kind, msg)
            out.append(C[0].view)
        if kind in xr.EXACT[scheme]:
            assert torch.equal(out[0], out[1]), "%s, %s: cut and uncut differ" % (scheme, kind)


@pytest.mark.parametrize("scheme", xr.SCHEMES)
def test_wide_tile_refused_by_a_late_view(dev, scheme):
    """B = rows 128 .. of a plane set that ends before the ninth block of 8 column tiles: narrow tiles.  The same rows as a plane set of their
    own: without a workspace the same narrow launch - bit-equal for every kind -, with one the wide tile cut along K - bit-equal where the data
    is exact, at the bar on floats."""
    from vistaocr_amd import ops
    case = xr.case_named("wide refused")
    plan = _assert_path(case)
    own_ws = ops.gemm_x6_plan(case.m, case.n, case.k16, b_rows=case.n, workspace=True)
    own_no = ops.gemm_x6_plan(case.m, case.n, case.k16, b_rows=case.n, workspace=False)
    assert xr.path_of(own_ws) == "wide/cut" and xr.path_of(own_no) == "narrow/whole", (own_ws, own_no)
    for ki, kind in enumerate(case.kinds):
        a, b, bias, ab, af, bf = _case_data(case, kind, 3200 + ki, dev)
        pa, pb = _planes_of(scheme, af, True, dev), _planes_of(scheme, bf, True, dev)
        pb_own = _planes_of(scheme, bf[case.b_row0:case.b_row0 + case.n].contiguous(), True, dev)
        amax, bmax = af.abs().max(1).values, bf[case.b_row0:case.b_row0 + case.n].abs().max(1).values
        outs = []
        for pbx, row0, ws, pl in ((pb, case.b_row0, True, plan), (pb_own, 0, False, own_no), (pb_own, 0, True, own_ws)):
            def run():
                C, ldc = _outputs(case, dev)
                _gemm(scheme, dev, pa, pbx, case.m, case.n, case.k16, C, ldc, b_row0=row0, ws=ws, plan=pl)
                return C
            C = _twice(run)
            msg, rel = xr.check(scheme, kind, C[0].view, ab, a, b, case.k, amax=amax, bmax=bmax)
            if rel is not None:
                print("X6_ERR | %s | %s | %s | %.3e" % (scheme, xr.path_of(pl), case.name, rel))
            assert msg is None and C[0].outside_untouched(), "%s, %s, %s: %s" % (case, scheme, kind, msg)
            outs.append(C[0].view)
        assert torch.equal(outs[0], outs[1]), "%s, %s: the shifted view and the unshifted planes differ on the same launch path" % (scheme, kind)
        if kind in xr.EXACT[scheme]:
            assert torch.equal(outs[0], outs[2]), "%s, %s: narrow (refused) and wide differ" % (scheme, kind)


@pytest.mark.parametrize("scheme", xr.SCHEMES)
@pytest.mark.parametrize("name", ["two views whole", "two views cut"])
def test_two_views_against_two_single_view_calls(dev, scheme, name):
    """rows < 256 read (a_kk0 = 1 | b_row0 = 0, b_kk0 = 0), rows >= 256 read (a_kk0 = 0 | b_row0 = 160, b_kk0 = 1): ONE launch must give the
    bits of the two launches it stands for (same tiles, same K splits), and both the float64 products"""
    from vistaocr_amd import ops
    case = xr.case_named(name)
    plan = _assert_path(case)
    m, n, k, half = case.m, case.n, case.k, case.rsplit
    v0, v1 = (case.a_kk0, case.b_row0, case.b_kk0), (case.b_kk0, case.two, case.a_kk0)
    single = [ops.gemm_x6_plan(half, n, k, b_rows=case.b_rows, b_row0=v[1]) for v in (v0, v1)]
    for s in single:
        assert xr.path_of(s) == case.path and (s["ksplit"], s["stages_per_split"]) == (plan["ksplit"], plan["stages_per_split"]), (s, plan)
    for ki, kind in enumerate(case.kinds):
        g = torch.Generator().manual_seed(3300 + ki)
        gen = (lambda *s: torch.randint(-8, 9, s, generator=g).float()) if kind == "ints" else (lambda *s: torch.randn(*s, generator=g))
        af, bf = gen(case.a_rows, case.a_k), gen(case.b_rows, case.b_k)
        pa, pb = _planes_of(scheme, af, False, dev), _planes_of(scheme, bf, False, dev)
        def both():
            C = [gr.Padded(None, n + 12, 0, dev, sentinel=True, shape=(half, n)) for _ in range(2)]
            _gemm(scheme, dev, pa, pb, m, n, k, C, n + 12, a_kk0=v0[0], b_row0=v0[1], b_kk0=v0[2], rsplit=half, two=v1, plan=plan)
            return C
        C = _twice(both)
        for i, v in enumerate((v0, v1)):
            asub, bsub = af[half * i:half * (i + 1), 16 * v[0]:16 * v[0] + k], bf[v[1]:v[1] + n, 16 * v[2]:16 * v[2] + k]
            def one():
                D = [gr.Padded(None, n + 12, 0, dev, sentinel=True, shape=(half, n))]
                _gemm(scheme, dev, pa, pb, half, n, k, D, n + 12, a_row0=half * i, a_kk0=v[0], b_row0=v[1], b_kk0=v[2], plan=single[i])
                return D
            D = _twice(one)[0]
            what = "%s, %s, %s, view %d" % (case, scheme, kind, i)
            assert torch.equal(C[i].view, D.view), what + ": one launch and two launches differ"
            assert C[i].outside_untouched() and D.outside_untouched(), what + ": wrote outside C"
            ref = asub.to(dev).double() @ bsub.to(dev).double().t()
            msg, rel = xr.check(scheme, kind, C[i].view, ref)
            if rel is not None:
                print("X6_ERR | %s | %s | %s | %.3e" % (scheme, case.path, case.name, rel))
            assert msg is None, "%s: %s" % (what, msg)


@pytest.mark.parametrize("scheme", xr.SCHEMES)
@pytest.mark.parametrize("name", ["nonfinite direct", "nonfinite cut"])
def test_one_nonfinite_element_poisons_its_row_and_nothing_else(dev, scheme, name):
    """a NaN or an Inf in A makes every element of its output row non-finite (a gradient's NaN must reach the weights) and leaves every other
    row bit-equal to the clean run; likewise for B and its output column - through the direct store and through the K slabs"""
    case = xr.case_named(name)
    plan = _assert_path(case)
    m, n, k = case.m, case.n, case.k
    a, b, _, _, _, _ = _case_data(case, "floats", 3400, dev)
    pb = _planes_of(scheme, b, False, dev)

    def run(pa_, pb_):
        def once():
            C, ldc = _outputs(case, dev)
            _gemm(scheme, dev, pa_, pb_, m, n, case.k16, C, ldc, plan=plan)
            return C
        C = _twice(once)
        assert C[0].outside_untouched()
        return C[0].view.clone()

    pa = _planes_of(scheme, a, True, dev)
    clean = run(pa, pb)
    assert bool(torch.isfinite(clean).all())
    r0, c0, k0 = 100, 77, k - 3
    for bad in (float("nan"), float("inf"), float("-inf")):
        for kc in (True, False):
            a2 = a.clone()
            a2[r0, k0] = bad
            got = run(_planes_of(scheme, a2, kc, dev), pb)
            what = "%s, %s, %r in A (%s source)" % (case, scheme, bad, "rk" if kc else "kr")
            assert not bool(torch.isfinite(got[r0]).any()), what + ": finite elements in the poisoned row"
            keep = torch.arange(m, device=dev) != r0
            assert torch.equal(got[keep], clean[keep]), what + ": another row changed"
            b2 = b.clone()
            b2[c0, k0] = bad
            got = run(pa, _planes_of(scheme, b2, kc, dev))
            what = "%s, %s, %r in B (%s source)" % (case, scheme, bad, "rk" if kc else "kr")
            assert not bool(torch.isfinite(got[:, c0]).any()), what + ": finite elements in the poisoned column"
            keep = torch.arange(n, device=dev) != c0
            assert torch.equal(got[:, keep], clean[:, keep]), what + ": another column changed"

