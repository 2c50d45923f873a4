"""GPU: vocr_augment_lines against the numpy restatement of tests/augment_ref.py.  Exact where the arithmetic is exact (identity,
integer shifts, which pixels a draw selects, stripes, the clamp, a line alone against the same line in a batch); elsewhere the
kernel's distance from the float64 restatement is held to 4 x the distance of the float32 restatement - the same operations in the
same order - on the test's own inputs: the margin covers the kernel's fused multiply-adds and its logf / cosf.  Both numbers of every
such comparison go to profiles/augment_fp64_errors.txt."""
import os

import numpy as np
import pytest
import torch

from tests import augment_ref as ar
from tests.gemm_ref import GUARD, Padded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERRORS = os.path.join(ROOT, "profiles", "augment_fp64_errors.txt")
SMALL = (67, 64, 33, 16, 1)
SEAMS = (259, 257, 256, 65, 64, 63, 17)                       # around the 256-column tile and the 64-lane wave
SHAPES = [(SMALL, 7, 1), (SMALL, 7, 3), (SMALL, 30, 1), (SMALL, 30, 3), (SEAMS, 30, 1), ((1200,), 60, 1)]
IDS = ["%dx%dx%dx%d" % (len(w), c, h, w[0]) for w, h, c in SHAPES]
MARGIN = 4.0
_LOG = {}


def _images(widths, h, c, seed, lo=0.0, hi=1.0, nan_pad=True):
    """x [B, c, h, Wmax] fp32 uniform in [lo, hi), the pad columns NaN"""
    rng = np.random.default_rng(seed)
    x = (lo + (hi - lo) * rng.random((len(widths), c, h, widths[0]))).astype(np.float32)
    if nan_pad:
        for i, w in enumerate(widths):
            x[i, :, :, w:] = np.nan
    return x


def _run(x, widths, params, mesh=None, gh=0, with_filter=None):
    from vistaocr_amd import ops
    dev = "cuda"
    if with_filter is None:
        with_filter = bool((params[:, 17] & ar.FLAG_FILTER).any())
    md = torch.from_numpy(np.ascontiguousarray(mesh).reshape(-1)).to(dev) if mesh is not None else None
    y = ops.augment_lines(torch.from_numpy(x).to(dev), torch.as_tensor(np.asarray(widths), dtype=torch.int32).to(dev),
                          torch.from_numpy(np.ascontiguousarray(params).view(np.int32).reshape(-1)).to(dev), md, gh,
                          mesh.shape[3] - 1 if mesh is not None else 0, with_filter)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mesh(widths, h, seed, interval=(25.0, 12.0), std=(2.0, 1.0)):
    """(mesh [B, 2, gh + 1, gw_max + 1], gh, gw [B]) as DeviceAugmenter.draw lays it out"""
    rng = np.random.default_rng(seed)
    gw = np.maximum(1, np.rint(np.asarray(widths) / interval[0])).astype(np.int64)
    gh = max(1, int(round(h / interval[1])))
    m = rng.normal(size=(len(widths), 2, gh + 1, int(gw.max()) + 1)) * np.array(std).reshape(1, 2, 1, 1)
    for i, g in enumerate(gw):
        m[i, :, :, g + 1:] = 0.0
    return m.astype(np.float32), gh, gw


def _affines(widths, h, seed):
    """one affine per line: rotation, zoom in or out and a shift; the widest excursions leave the line on every side"""
    from vistaocr_amd.augment import compose_affine
    rng = np.random.default_rng(seed)
    out = []
    for w in widths:
        out.append(compose_affine(w, h, angle_deg=rng.uniform(-4, 4), zoom_x=rng.uniform(0.85, 1.15), zoom_y=rng.uniform(0.8, 1.2),
                                  shift_x=rng.uniform(-3, 3), shift_y=rng.uniform(-1.5, 1.5)).reshape(-1))
    return np.stack(out)


def _held(name, y, x, widths, params, mesh=None, gh=0):
    """the kernel's y against the float64 restatement, at MARGIN x the float32 restatement's own distance from it"""
    ref = ar.augment(x, widths, params, mesh, gh, np.float64)
    r32 = ar.augment(x, widths, params, mesh, gh, np.float32)
    assert r32.dtype == np.float32
    e32, ek = float(np.abs(r32.astype(np.float64) - ref).max()), float(np.abs(y.astype(np.float64) - ref).max())
    print("%s: fp32 restatement %.3e, kernel %.3e, bar %.3e" % (name, e32, ek, MARGIN * e32))
    _LOG[name] = (e32, ek)
    assert np.isfinite(y).all() and e32 > 0
    assert ek <= MARGIN * e32, (name, ek, e32)
    return ref


@pytest.fixture(scope="module", autouse=True)
def _write_errors():
    yield
    if _LOG:
        with open(ERRORS, "w") as fh:
            fh.write("vocr_augment_lines against the float64 restatement of tests/augment_ref.py: largest |difference| over the outputs of a case.\n"
                     "fp32: the float32 restatement (same operations, same order, no fused multiply-add); kernel: the device; bar = %g x fp32.\n"
                     "%-44s %12s %12s %8s\n" % (MARGIN, "case", "fp32", "kernel", "ratio"))
            for name in sorted(_LOG):
                e32, ek = _LOG[name]
                fh.write("%-44s %12.3e %12.3e %8.2f\n" % (name, e32, ek, ek / e32))


@pytest.mark.parametrize("widths,h,c", SHAPES, ids=IDS)
def test_identity_is_bitwise_and_pad_is_zero(widths, h, c):
    x = _images(widths, h, c, 1)
    for with_filter in (False, True):                           # the filter's pass launched with no line flagged changes nothing
        y = _run(x, widths, ar.make_params(len(widths)), with_filter=with_filter)
        for i, w in enumerate(widths):
            assert np.array_equal(_bits(y[i, :, :, :w]), _bits(x[i, :, :, :w])), (i, w)
            assert not _bits(y[i, :, :, w:]).any(), (i, w)


@pytest.mark.parametrize("widths,h,c", SHAPES, ids=IDS)
def test_integer_shifts_replicate_the_border_bit_for_bit(widths, h, c):
    x = _images(widths, h, c, 2)
    shifts = [(3, 1), (-3, 1), (3, -1), (-3, -1)]
    a = np.array([[1, 0, shifts[i % 4][0], 0, 1, shifts[i % 4][1]] for i in range(len(widths))], dtype=np.float32)
    y = _run(x, widths, ar.make_params(len(widths), A=a))
    for i, w in enumerate(widths):
        dx, dy = shifts[i % 4]
        cols, rows = np.clip(np.arange(w) + dx, 0, w - 1), np.clip(np.arange(h) + dy, 0, h - 1)
        want = x[i][:, rows][:, :, cols]
        assert np.array_equal(_bits(y[i, :, :, :w]), _bits(want)), (i, w)
        assert not _bits(y[i, :, :, w:]).any()


@pytest.mark.parametrize("widths,h,c", SHAPES, ids=IDS)
def test_affine_and_mesh_against_fp64(widths, h, c):
    x = _images(widths, h, c, 3)
    b = len(widths)
    a = _affines(widths, h, 4)
    _held("affine %s" % IDS[SHAPES.index((widths, h, c))], _run(x, widths, ar.make_params(b, A=a)), x, widths, ar.make_params(b, A=a))
    mesh, gh, gw = _mesh(widths, h, 5)
    p = ar.make_params(b, A=a, flags=ar.FLAG_MESH, gw=gw)
    p[1::2, 0:6] = ar.make_params(1)[0, 0:6]                   # every other line: the mesh alone
    ref = _held("affine+mesh %s" % IDS[SHAPES.index((widths, h, c))], _run(x, widths, p, mesh, gh), x, widths, p, mesh, gh)
    assert np.abs(ref - ar.augment(x, widths, ar.make_params(b, A=a))).max() > 1e-2        # the mesh did move something
    # the mesh flag off: D is exactly 0, whatever the table holds
    p_off = ar.make_params(b, gw=gw)
    y = _run(x, widths, p_off, mesh, gh)
    for i, w in enumerate(widths):
        assert np.array_equal(_bits(y[i, :, :, :w]), _bits(x[i, :, :, :w]))


@pytest.mark.parametrize("widths,h,c", SHAPES, ids=IDS)
def test_block_filter_and_renormalisation_against_fp64(widths, h, c):
    x = _images(widths, h, c, 6)
    b = len(widths)
    const = 2 if b > 2 else None
    rng = np.random.default_rng(7)
    taps = rng.normal(size=(b, 5)).astype(np.float32)
    taps[0] = 1.0                                               # TessBlockConv(1, 1)
    if const is not None:                                       # a constant line under a filter without the padded taps: max = min
        x[const, :, :, :widths[const]] = np.float32(0.375)
        taps[const] = (0.0, 0.0, 0.0, 1.5, 0.25)
    p = ar.make_params(b, taps=taps, flags=ar.FLAG_FILTER)
    y = _run(x, widths, p)
    ref = _held("filter %s" % IDS[SHAPES.index((widths, h, c))], y, x, widths, p)
    for i, w in enumerate(widths):
        if i == const:
            assert not _bits(y[i]).any() and not ref[i].any()   # max = min gives 0, never NaN
        else:                                                   # the renormalisation reaches both ends of [0, 1] exactly
            assert y[i, :, :, :w].min() == 0.0 and y[i, :, :, :w].max() == 1.0
    # with an affine map in front and the contrast behind
    a = _affines(widths, h, 8)
    p2 = ar.make_params(b, A=a, taps=taps, flags=ar.FLAG_FILTER, alpha=rng.uniform(0.5, 2.0, b))
    _held("affine+filter+contrast %s" % IDS[SHAPES.index((widths, h, c))], _run(x, widths, p2), x, widths, p2)


@pytest.mark.parametrize("widths,h,c", [SHAPES[1], SHAPES[4], SHAPES[5]], ids=[IDS[1], IDS[4], IDS[5]])
def test_photometric_draws_stripes_and_clamp(widths, h, c):
    b = len(widths)
    x = _images(widths, h, c, 9, lo=0.3, hi=0.7)                # room for the noise: no clamp in the first half
    keys = np.arange(b, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(12345)
    base = ar.make_params(b, alpha=0.9, key=keys)
    on = ar.make_params(b, alpha=0.9, key=keys, p_noise=0.25, sigma=0.0625, p_del=0.125, del_value=0.875)
    y0, y1 = _run(x, widths, base), _run(x, widths, on)
    n_noised = n_deleted = 0
    for i, w in enumerate(widths):
        noised, deleted = ar.decisions(on[i], c, h, w)
        n_noised, n_deleted = n_noised + int(noised.sum()), n_deleted + int(deleted.sum())
        a, bb = y0[i, :, :, :w], y1[i, :, :, :w]
        assert (bb[deleted] == np.float32(0.875)).all()
        untouched = ~noised & ~deleted
        assert np.array_equal(_bits(bb[untouched]), _bits(a[untouched]))
        assert (bb[noised & ~deleted] != a[noised & ~deleted]).mean() > 0.999        # (a draw of n = 0 to the last bit is possible)
    total = sum(widths) * h * c
    assert abs(n_noised / total - 0.25) < 5 * np.sqrt(0.25 * 0.75 / total)
    assert n_noised > 0 and n_deleted > 0
    _held("noise+delete %s" % IDS[SHAPES.index((widths, h, c))], y1, x, widths, on)
    # another key selects other pixels
    other = ar.make_params(b, alpha=0.9, key=keys + np.uint64(1), p_noise=0.25, sigma=0.0625, p_del=0.125, del_value=0.875)
    assert not np.array_equal(ar.decisions(other[0], c, h, widths[0])[0], ar.decisions(on[0], c, h, widths[0])[0])
    # stripes and the clamp: a strong contrast and invert push values out of [0, 1]; rows [r0, r1) hold the stripe value exactly
    x = _images(widths, h, c, 10)
    r0 = np.arange(b) % max(h - 2, 1)
    r1 = np.minimum(h, r0 + 1 + np.arange(b) % 4)
    p = ar.make_params(b, alpha=2.0, flags=ar.FLAG_INVERT, r0=r0, r1=r1, stripe_value=0.625, key=keys, p_noise=0.5, sigma=0.5)
    y = _run(x, widths, p)
    pre = ar.make_params(b, alpha=2.0, flags=ar.FLAG_INVERT, key=keys, p_noise=0.5, sigma=0.5)
    for i, w in enumerate(widths):
        assert (y[i, :, r0[i]:r1[i], :w] == np.float32(0.625)).all()
        rows = np.ones(h, dtype=bool)
        rows[r0[i]:r1[i]] = False
        got = y[i][:, rows, :w]
        assert (got >= 0).all() and (got <= 1).all()
        # where the float64 value before the clamp is clearly outside, the result is the bound itself
        f = pre[i].view(np.float32).astype(np.float64)
        noised, _ = ar.decisions(pre[i], c, h, w)
        v = 1.0 - ((x[i, :, :, :w].astype(np.float64) - 0.5) * f[11] + 0.5)
        quiet = ~noised[:, rows]
        vq, gq = v[:, rows][quiet], got[quiet]
        assert (gq[vq > 1 + 1e-5] == 1.0).all() and (gq[vq < -1e-5] == 0.0).all() and (vq > 1 + 1e-5).any() and (vq < -1e-5).any()
    _held("contrast+invert+noise+stripe+clamp %s" % IDS[SHAPES.index((widths, h, c))], y, x, widths, p)


def _everything(widths, h, c, seed):
    """tables with every stage on for every line"""
    b = len(widths)
    rng = np.random.default_rng(seed)
    mesh, gh, gw = _mesh(widths, h, seed + 1)
    keys = rng.integers(0, 1 << 63, b, dtype=np.uint64)
    r0 = rng.integers(0, h, b)
    p = ar.make_params(b, A=_affines(widths, h, seed + 2), taps=rng.normal(size=(b, 5)), flags=ar.FLAG_MESH | ar.FLAG_FILTER | ar.FLAG_INVERT,
                       gw=gw, alpha=rng.uniform(0.5, 2.0, b), p_noise=0.25, sigma=0.0625, p_del=0.0625, del_value=0.875, r0=r0,
                       r1=np.minimum(h, r0 + 2), stripe_value=0.125, key=keys)
    return p, mesh, gh, gw


@pytest.mark.parametrize("widths,h,c", [SHAPES[3], SHAPES[4]], ids=[IDS[3], IDS[4]])
def test_a_line_alone_equals_the_line_in_its_batch_and_runs_repeat(widths, h, c):
    x = _images(widths, h, c, 11)
    p, mesh, gh, gw = _everything(widths, h, c, 12)
    y = _run(x, widths, p, mesh, gh)
    assert np.array_equal(_bits(y), _bits(_run(x, widths, p, mesh, gh)))                  # two runs: the same bits
    _held("everything %s" % IDS[SHAPES.index((widths, h, c))], y, x, widths, p, mesh, gh)
    for i, w in enumerate(widths):                              # B = 1, Wmax = w, the line's own mesh stride
        alone = _run(np.ascontiguousarray(x[i:i + 1, :, :, :w]), [w], p[i:i + 1], np.ascontiguousarray(mesh[i:i + 1, :, :, :gw[i] + 1]), gh)
        assert np.array_equal(_bits(alone[0]), _bits(y[i, :, :, :w])), (i, w)


def test_rgb_channels_share_one_geometry():
    widths, h = SMALL, 30
    g = _images(widths, h, 1, 13)
    x = np.ascontiguousarray(np.repeat(g, 3, axis=1))
    p, mesh, gh, gw = _everything(widths, h, 3, 14)
    p[:, 12] = p[:, 14] = 0                                     # no per-pixel draws: they differ per channel by design
    y = _run(x, widths, p, mesh, gh)
    assert np.array_equal(_bits(y[:, 0]), _bits(y[:, 1])) and np.array_equal(_bits(y[:, 0]), _bits(y[:, 2]))
    # and a grey call of the same tables gives that picture (the line's min / max over three equal channels is the channel's own)
    y1 = _run(g, widths, p, mesh, gh)
    assert np.array_equal(_bits(y1[:, 0]), _bits(y[:, 0]))
    # with the draws on, the channels get different noise
    p[:, 12] = ar.make_params(1, p_noise=0.25)[0, 12]
    yn = _run(x, widths, p, mesh, gh)
    assert not np.array_equal(yn[:, 0], yn[:, 1])


@pytest.mark.parametrize("widths,h,c", [SHAPES[3], SHAPES[4]], ids=[IDS[3], IDS[4]])
def test_guarded_buffers(widths, h, c):
    """x between NaN guard bands (GUARD floats and PR whole rows on either side, its pad columns NaN as well), y and the workspace
    between sentinels.  The maps leave every line by up to 42 columns (< GUARD) and 6 rows (< PR): a tap that is not clamped reads a
    NaN inside the allocation, never memory outside it."""
    from vistaocr_amd import _lib
    PR = 8
    dev = "cuda"
    b, wmax = len(widths), widths[0]
    x = _images(widths, h, c, 15)
    rows = b * c * h
    framed = np.full((rows + 2 * PR, wmax), np.nan, dtype=np.float32)
    framed[PR:PR + rows] = x.reshape(rows, wmax)
    xp = Padded(torch.from_numpy(framed), wmax, 0, dev)
    yp = Padded(None, wmax, 0, dev, sentinel=True, shape=(rows, wmax))
    lib = _lib.load()
    nbytes = lib.vocr_augment_workspace_bytes(b, c, h, wmax)
    assert nbytes > 0 and nbytes % 8 == 0
    wp = Padded(None, nbytes // 4, 0, dev, sentinel=True, shape=(1, nbytes // 4))
    from vistaocr_amd.augment import compose_affine
    mesh, gh, gw = _mesh(widths, h, 16, std=(1.0, 0.25))
    moves = [dict(shift_x=38, shift_y=2.5), dict(shift_x=-38, shift_y=-2.5), dict(zoom_x=1.25, zoom_y=1.15, angle_deg=0.5),
             dict(shift_x=30.5, shift_y=-2.0, angle_deg=-1.0)]
    a = np.stack([compose_affine(w, h, **moves[i % 4]).reshape(-1) for i, w in enumerate(widths)])
    rng = np.random.default_rng(17)
    p = ar.make_params(b, A=a, taps=rng.normal(size=(b, 5)), flags=ar.FLAG_MESH | ar.FLAG_FILTER, gw=gw, alpha=1.25, p_noise=0.25, sigma=0.03125,
                       key=rng.integers(0, 1 << 63, b, dtype=np.uint64))
    wd = torch.as_tensor(np.asarray(widths), dtype=torch.int32).to(dev)
    pd = torch.from_numpy(p.view(np.int32).reshape(-1)).to(dev)
    md = torch.from_numpy(mesh.reshape(-1)).to(dev)
    x_ptr = xp.ptr + PR * wmax * 4
    assert x_ptr % 4 == 0 and wp.ptr % 8 == 0 and GUARD > 42
    _lib.call("vocr_augment_lines", x_ptr, wd.data_ptr(), b, c, h, wmax, pd.data_ptr(), md.data_ptr(), gh, mesh.shape[3] - 1, 1, yp.ptr,
              wp.ptr, nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y = yp.view.cpu().numpy().reshape(b, c, h, wmax)
    assert np.isfinite(y).all()
    assert yp.outside_untouched() and wp.outside_untouched()
    _held("guarded %s" % IDS[SHAPES.index((widths, h, c))], y, x, widths, p, mesh, gh)


def test_train_takes_an_augmented_batch():
    import vistaocr_amd as va
    al = va.english_alphabet()
    B, W, L = 3, 120, 4
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 1, 30, W, generator=g)
    widths = torch.tensor([120, 100, 61], dtype=torch.int32)
    for i in range(B):
        x[i, :, :, int(widths[i]):] = 0
    tgt = torch.randint(1, len(al), (B * L,), generator=g).to(torch.int32)
    tl = torch.full((B,), L, dtype=torch.int32)
    batch = (x, tgt, widths, tl, {"utt-ids": ["a", "b", "c"]})

    def loss_of(b):
        torch.manual_seed(0)
        model = va.CnnOcrModel(alphabet=al, verbose=False, input_line_height=30, rds_line_height=30, lstm_input_dim=32, num_lstm_layers=1,
                               num_lstm_hidden_units=32, p_lstm_dropout=0.0, num_in_channels=1)
        model.train()
        opt = va.make_optimizer(model, lr=1e-3)
        torch.manual_seed(1)
        torch.cuda.manual_seed(1)
        return va.train(b, model, va.CTCLoss(), opt)

    def augmented():
        aug = va.DeviceAugmenter(seed=3, p_rotate=1.0, p_filter_rand=1.0, p_contrast=1.0, p_mesh=1.0, p_noise=1.0, noise_p=0.3, p_stripe=1.0)
        aug.step = 7
        out = aug(batch)
        assert aug.step == 8 and out[0].is_cuda and out[0].shape == x.shape and out[1] is tgt and out[2] is widths and out[3] is tl and out[4] is batch[4]
        return out

    plain, first, second = loss_of(batch), loss_of(augmented()), loss_of(augmented())
    assert np.isfinite(plain) and np.isfinite(first)
    assert first == second
    assert first != plain
    ya = augmented()[0].cpu().numpy()
    assert np.isfinite(ya).all() and ya.min() >= 0 and ya.max() <= 1 and not ya[2, :, :, 61:].any()
    aug = va.DeviceAugmenter(seed=3, p_rotate=1.0, p_filter_rand=1.0, p_contrast=1.0, p_mesh=1.0, p_noise=1.0, noise_p=0.3, p_stripe=1.0)
    pr = aug.draw(widths, 30, 7)
    _held("the augmenter's own tables", ya, x.numpy(), pr.widths, pr.records, pr.mesh, pr.gh)    # ... through the restatement: the same picture
