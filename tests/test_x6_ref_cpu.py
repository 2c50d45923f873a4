"""CPU: the split-operand GEMM suite's own tools (tests/x6_ref.py) - do its data kinds have teeth?

A numpy emulation of both schemes (bf16 by round-to-nearest-even bit operations, fp16 by np.float16 with the per-row power-of-two scale, the
partial products of a k16 step added to an fp32 accumulator in the kernel's order) meets every bar of the suite on small shapes; the same
emulation with any ONE partial product left out, or any ONE operand plane zeroed, fails at least one of the kinds that carry no float
tolerance (bf16x6: bit-exact kinds; fp16x3: the bit-exact integers and the selector kinds at include/vocr.h's per-element bound).  That is the
evidence that sel12 is needed (nothing else catches a missing a1 b1) and that the kinds together are sufficient.  Also: the fragment decoder
against the layout's definition, the bf16 rounding against torch's, the properties sel12 claims."""
import numpy as np
import pytest
import torch

from tests import x6_ref as xr

SHAPES = ((33, 17, 40), (70, 50, 100))
NOFLOAT = tuple(k for k in xr.KINDS if k != "floats")


def _fails(scheme, drop=(), zero_a=(), zero_b=()):
    """the kinds (and floats) whose bar the emulated scheme misses on either shape"""
    failed = []
    for kind in xr.KINDS:
        for (m, n, k) in SHAPES:
            a, b, _, ab = xr.make_data(kind, m, n, k, 100 + m)
            c = xr.emulate(scheme, a.numpy(), b.numpy(), drop=drop, zero_a=zero_a, zero_b=zero_b)
            msg, _ = xr.check(scheme, kind, torch.from_numpy(c), ab, a, b, k)
            if msg is not None:
                failed.append(kind)
                break
    return failed


@pytest.mark.parametrize("scheme", xr.SCHEMES)
def test_the_full_scheme_meets_every_bar(scheme):
    assert _fails(scheme) == []


@pytest.mark.parametrize("scheme", xr.SCHEMES)
def test_every_missing_product_and_every_zeroed_plane_is_caught_without_a_tolerance(scheme):
    np_ = xr.NPLANES[scheme]
    holes = []
    for what, kw in ([("product a%d b%d" % p, dict(drop=(p,))) for p in xr.PRODUCTS[scheme]] +
                     [("plane a%d zeroed" % i, dict(zero_a=(i,))) for i in range(np_)] + [("plane b%d zeroed" % i, dict(zero_b=(i,))) for i in range(np_)]):
        caught = [k for k in _fails(scheme, **kw) if k in NOFLOAT]
        print("X6_TEETH | %s | %-18s | caught by %s" % (scheme, what, ", ".join(caught) or "NOTHING"))
        if not caught:
            holes.append(what)
    assert not holes, "%s: no kind without a float tolerance notices %s" % (scheme, holes)


def test_sel12_is_what_catches_a1_b1():
    """without sel12 nothing exact notices a missing a1 b1 (N(0,1) floats stay under their norm-wise bar too): the kind is needed"""
    caught = _fails("bf16x6", drop=((1, 1),))
    assert set(caught) <= {"sel12A", "sel12B"} and caught, caught


def test_sel12_data_is_what_it_claims():
    for kind in ("sel12A", "sel12B"):
        a, b, bias, ab = xr.make_data(kind, 40, 30, 64, 3)
        sel, dense = (a, b) if kind == "sel12A" else (b, a)
        assert bool(((sel != 0).sum(1) == 1).all())
        for t in (sel[sel != 0], dense.reshape(-1)):
            mag = t.abs().double()
            assert bool((mag % 2 == 1).all()) and float(mag.min()) >= 256 and float(mag.max()) < 4096
            planes, _ = xr.split_bf16x6(t.numpy())
            assert np.all(planes[1] != 0) and np.all(planes[2] == 0) and np.array_equal(planes[0] + planes[1], t.numpy())
        assert float(ab.abs().max()) < 2.0 ** 24 and torch.equal(ab, a.double() @ b.double().t())


def test_bf16_rounding_by_bits_is_torchs_and_the_planes_sum_exactly():
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(4096, generator=g) * torch.pow(10.0, (torch.rand(4096, generator=g) - 0.5) * 70)).float()
    edge = torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 2.0 ** -126, 2.0 ** -133, 2.0 ** -149, 3.0e38, -3.3e38], dtype=torch.float32)
    x = torch.cat([x, edge])
    assert np.array_equal(xr.bf16_rne(x.numpy()).view(np.uint32), x.bfloat16().float().numpy().view(np.uint32))
    # the top of the range: rounding to nearest would give infinity, the split truncates and stays exact
    top = np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, np.float32(2.0 ** 127 * (2 - 2.0 ** -8)), np.float32(2.0 ** 127 * (2 - 2.0 ** -7))])
    x = np.concatenate([x.numpy(), top.astype(np.float32)])
    planes, _ = xr.split_bf16x6(x)
    assert all(np.isfinite(p).all() for p in planes)
    # exact from 2^-110 up (an fp32 ulp there is bf16's smallest denormal, 2^-133); below, half of that at the most
    err = np.abs(planes[0].astype(np.float64) + planes[1] + planes[2] - x.astype(np.float64))
    small = np.abs(x) < 2.0 ** -110
    assert small.sum() > 50 and err[small].max() > 0 and not err[~small].any() and err.max() <= 2.0 ** -134
    for p in planes:
        assert not np.any(p.view(np.uint32) & 0xFFFF)


@pytest.mark.parametrize("scheme", xr.SCHEMES)
def test_fragment_decoder_against_the_layouts_definition(scheme):
    """encode a matrix lane by lane as the split kernels' header comment defines the order, decode it vectorised"""
    rows, k = 300, 40
    RT, KK, NP = xr.rt_of(rows), xr.kk_of(k), xr.NPLANES[scheme]
    dt = torch.bfloat16 if scheme == "bf16x6" else torch.float16
    g = torch.Generator().manual_seed(6)
    x = torch.zeros(NP, RT * 32, KK * 16)
    x[:, :rows, :k] = torch.randint(-64, 65, (NP, rows, k), generator=g).float()
    frag = torch.zeros(NP, RT, KK, 64, 8, dtype=dt)
    for lane in range(64):
        r, h = lane & 31, lane >> 5
        for kk in range(KK):
            frag[:, :, kk, lane, :] = x[:, r::32, 16 * kk + 8 * h:16 * kk + 8 * h + 8].to(dt)
    raw = frag.view(torch.uint8).reshape(-1)
    amax = torch.arange(RT * 32, dtype=torch.float32)
    if scheme == "fp16x3":
        raw = torch.cat([raw, amax.view(torch.uint8)])
    assert raw.numel() == xr.planes_bytes(scheme, rows, k)
    p, am = xr.decode(torch.cat([raw, torch.full((64,), 0xA5, dtype=torch.uint8)]), scheme, rows, k)
    assert torch.equal(p, x.double())
    assert (am is None) if scheme == "bf16x6" else torch.equal(am, amax)
