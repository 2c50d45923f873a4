"""CPU: tests/step_glue_ref.py held to itself, so that the bars test_step_glue_gpu.py asserts are neither loose nor unreachable.

  * adam_step32 - the kernel's operation order in numpy float32, one rounding per operation, no FMA - sits inside adam_bars on every
    input family of adam_inputs (every step, weight decay and gradient scale of the case lists, a count above the launch cap);
  * each of the six wrong Adams of MUTANTS leaves a bar by more than 100 x at every setting where it computes something else;
  * adam_step64 is torch.optim.Adam: twenty steps of the real optimiser in float64 (with the clamp in front) reproduce it to 1e-12;
  * dropout_mask_ref's hash is vistaocr_amd/augment.py's and plain integer arithmetic's; the mask's statistics and prefix property;
  * the special values clamp_data promises are there.
Run with -s for the ratios (profiles/step_glue_errors.txt keeps them)."""
import numpy as np
import pytest
import torch

from tests import step_glue_ref as sg

HYPER = (sg.LR, sg.BETA1, sg.BETA2, sg.EPS)
CPU_COUNT = 1 << 16                                         # every family of adam_inputs 512 times over
SETTINGS = [(step, wd, gs) for step in sg.ADAM_STEPS for wd in sg.ADAM_WDS for gs in sg.ADAM_SCALES]


def _args(wd, gs, step):
    return HYPER + (wd, sg.CLAMP, gs, step)


def _worst(ratios):
    return max(r for r, _ in ratios.values())


def test_fp32_restatement_sits_inside_the_bars():
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for count in (257, CPU_COUNT):
        for step, wd, gs in SETTINGS:
            state = sg.adam_inputs(count, step, seed=11)
            a = _args(wd, gs, step)
            ref, bars = sg.adam_step64(*state, *a), sg.adam_bars(*state, *a)
            r = sg.adam_ratios(sg.adam_step32(*state, *a), ref, bars)
            for k in worst:
                worst[k] = max(worst[k], r[k][0])
                assert r[k][0] <= 1.0, "fp32 restatement outside the %s bar: %.3f at element %d, count %d step %d wd %g gs %g" % (
                    (k,) + r[k] + (count, step, wd, gs))
    print("\nadam cpu fp32 restatement, %d settings x counts 257 and %d: worst ratio p %.3f  m %.3f  v %.3f" % (
        len(SETTINGS), CPU_COUNT, worst["p"], worst["m"], worst["v"]))
    # the bars are not slack either: the restatement uses a tenth of each at least
    assert min(worst.values()) > 0.1, worst


def test_fp32_restatement_above_the_launch_cap():
    """the GPU suite's largest buffer: nothing in the generator or the bars depends on the count"""
    count = sg.ADAM_LARGE_COUNTS[-1]
    for step, wd, gs in sg.ADAM_LARGE_SETTINGS:
        state = sg.adam_inputs(count, step, seed=11)
        a = _args(wd, gs, step)
        r = sg.adam_ratios(sg.adam_step32(*state, *a), sg.adam_step64(*state, *a), sg.adam_bars(*state, *a))
        print("\nadam cpu fp32 restatement, count %d step %d wd %g gs %.3g: p %.3f  m %.3f  v %.3f" % (
            count, step, wd, gs, r["p"][0], r["m"][0], r["v"][0]))
        assert _worst(r) <= 1.0, r


@pytest.mark.parametrize("mutant", sg.MUTANTS)
def test_bars_tell_a_wrong_adam_from_rounding(mutant):
    least, ran = float("inf"), 0
    for step, wd, gs in SETTINGS:
        if not sg.mutant_applies(mutant, step, wd, gs):
            continue
        state = sg.adam_inputs(CPU_COUNT, step, seed=11)
        a = _args(wd, gs, step)
        ref, bars = sg.adam_step64(*state, *a), sg.adam_bars(*state, *a)
        w = _worst(sg.adam_ratios(sg.adam_step64(*state, *a, variant=mutant), ref, bars))
        assert w > 100.0, "%s leaves the bars by only %.1f x at step %d wd %g gs %g" % (mutant, w, step, wd, gs)
        least, ran = min(least, w), ran + 1
    assert ran >= 4, ran
    print("\nadam mutant %-18s %2d settings: leaves a bar by at least %.3g x" % (mutant, ran, least))


def test_mutants_that_do_not_apply_are_the_reference():
    """mutant_applies is not an excuse list: where it says no, the variant equals Adam to double rounding"""
    for mutant in sg.MUTANTS:
        for step, wd, gs in SETTINGS:
            if sg.mutant_applies(mutant, step, wd, gs):
                continue
            state = sg.adam_inputs(4096, step, seed=11)
            a = _args(wd, gs, step)
            w = _worst(sg.adam_ratios(sg.adam_step64(*state, *a, variant=mutant), sg.adam_step64(*state, *a), sg.adam_bars(*state, *a)))
            assert w < 1e-3, (mutant, step, wd, gs, w)


def test_reference_is_torch_adam_in_double():
    """twenty steps of torch.optim.Adam on float64 tensors, gradients scaled and clamped as the reference's loop does, against adam_step64
    chained in double; the betas are the fp32-rounded ones the C entry receives (module docstring)"""
    n, wd, gs = 4096, 0.01, 0.5
    b1, b2 = float(np.float32(sg.BETA1)), float(np.float32(sg.BETA2))
    lr, eps, wdf, gsf, clampf = (float(np.float32(x)) for x in (sg.LR, sg.EPS, wd, gs, sg.CLAMP))
    p0, _, _, _ = sg.adam_inputs(n, 1, seed=3)
    param = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.Adam([param], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wdf)
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for step in range(1, 21):
        g = sg.adam_inputs(n, step + 1, seed=3)[1]
        param.grad = (torch.from_numpy(g.astype(np.float64)) * gsf).clamp_(-clampf, clampf)
        opt.step()
        p, m, v = sg.adam_step64(p, g, m, v, sg.LR, sg.BETA1, sg.BETA2, sg.EPS, wd, sg.CLAMP, gs, step)
        st = opt.state[param]
        for name, ours, theirs in (("p", p, param.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
            theirs = theirs.numpy()
            err = np.abs(ours - theirs).max() / max(np.abs(theirs).max(), 1e-300)
            assert err < 1e-12, (name, step, err)


def test_nan_and_inf_gradients_in_the_reference():
    p, g, m, v = sg.adam_inputs(64, 10, seed=5)
    g[3], g[10], g[11] = np.nan, np.inf, -np.inf
    a = _args(0.0, 0.5, 10)
    p2, m2, v2 = sg.adam_step64(p, g, m, v, *a)
    bars = sg.adam_bars(p, g, m, v, *a)
    assert all(np.isnan(x[3]) for x in (p2, m2, v2)) and all(np.isnan(b[3]) for b in bars)
    keep = np.arange(64) != 3
    assert all(np.isfinite(x[keep]).all() for x in (p2, m2, v2)) and all(np.isfinite(b[keep]).all() for b in bars)
    g2 = g.copy()
    g2[10], g2[11] = 2 * sg.CLAMP, -2 * sg.CLAMP                 # +-inf * 0.5 clamps to what +-2 clamp * 0.5 clamps to
    assert all(np.array_equal(x[keep], y[keep]) for x, y in zip((p2, m2, v2), sg.adam_step64(p, g2, m, v, *a)))
    # adam_ratios leaves the NaN element out and reports a NaN where the reference is finite as infinite
    got = [x.copy() for x in (p2, m2, v2)]
    assert _worst(sg.adam_ratios(got, (p2, m2, v2), bars)) == 0.0
    got[0][5] = np.nan
    assert sg.adam_ratios(got, (p2, m2, v2), bars)["p"] == (float("inf"), 5)


def test_input_families():
    p, g, m, v = sg.adam_inputs(4096, 10, seed=1)
    assert all(x.dtype == np.float32 for x in (p, g, m, v))
    for val in (0.0, sg.CLAMP, -sg.CLAMP, 2 * sg.CLAMP, -2 * sg.CLAMP):
        assert (g == val).sum() >= 4096 // 16 - 8
    free = np.abs(g[(g != 0) & (np.abs(g) != sg.CLAMP) & (np.abs(g) != 2 * sg.CLAMP)])
    assert free.min() < 1e-8 and free.max() > 1.0 and (m[::7] == 0).all() and (v[::7] == 0).all() and (v >= 0).all()
    assert sg.adam_idle(g, m, v).sum() >= 30
    p1, g1, m1, v1 = sg.adam_inputs(4096, 1, seed=1)
    assert not m1.any() and not v1.any() and g1.any()
    assert all(np.array_equal(a, b) for a, b in zip(sg.adam_inputs(257, 2, seed=1), sg.adam_inputs(257, 2, seed=1)))
    assert sg.adam_inputs(1, 2, seed=1)[1].shape == (1,)
    # the GPU cases: the cap is the launch's (4096 workgroups of 256), the largest buffer about 2.1 M floats
    assert sg.ADAM_GRID_CAP == 1048576 and sg.ADAM_LARGE_COUNTS[-1] == 2097157 and sg.EW_GRID_CAP + 1029 == 2098181


def test_dropout_reference_is_the_augmenter_hash_and_plain_integers():
    from vistaocr_amd import augment
    z = np.random.default_rng(0).integers(0, 1 << 64, 4096, dtype=np.uint64)
    z[:4] = (0, 1, (1 << 64) - 1, 1 << 63)
    with np.errstate(over="ignore"):
        ours, theirs = sg.mix64(z), augment._mix64(z)
    assert np.array_equal(ours, theirs)
    assert [int(x) for x in ours[:64]] == [sg.mix64_int(int(x)) for x in z[:64]]
    # splitmix64's published first output from state 0 is the finaliser of the golden-ratio increment
    assert sg.mix64_int(0x9e3779b97f4a7c15) == 0xe220a8397b1dcdaf
    # the stream: element e of seed s, written out in integers - the wrap of seed * golden and of + e included
    for seed in sg.DROPOUT_SEEDS:
        u = sg.dropout_uniform_ref(33, seed)
        for e in (0, 1, 32):
            bits = sg.mix64_int(((seed * 0x9e3779b97f4a7c15) + e) & ((1 << 64) - 1)) >> 32
            assert float(u[e]) == (bits >> 8) / 16777216.0, (seed, e)
    far = sg.dropout_uniform_ref(4, 1, start=(1 << 32) + 5)                      # element indices are 64-bit
    assert float(far[0]) == (sg.mix64_int((0x9e3779b97f4a7c15 + (1 << 32) + 5) & ((1 << 64) - 1)) >> 40) / 16777216.0


def test_dropout_mask_reference():
    n = 1 << 16
    for p in sg.DROPOUT_PS:
        for seed in sg.DROPOUT_SEEDS:
            mk = sg.dropout_mask_ref(n, p, seed)
            scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
            assert mk.dtype == np.float32 and set(np.unique(mk).tolist()) <= {0.0, float(scale)}
            assert abs(float((mk != 0).mean()) - (1.0 - p)) < 4.0 * (0.25 / n) ** 0.5 + 1e-9, (p, seed)
            assert np.array_equal(mk[:1025], sg.dropout_mask_ref(1025, p, seed))        # a function of (seed, element) only
    assert (sg.dropout_mask_ref(4096, 0.0, 7) == 1.0).all()
    a, b = sg.dropout_mask_ref(n, 0.5, 0), sg.dropout_mask_ref(n, 0.5, 1)
    assert 0.4 < float((a != b).mean()) < 0.6                                          # neighbouring seeds are unrelated streams


def test_clamp_data_holds_what_it_promises():
    x = sg.clamp_data(1025, 5.0, seed=2)
    bits = x.view(np.int32)
    assert (bits == np.float32(-0.0).view(np.int32)).any() and (bits == 0).any()
    for val in (5.0, -5.0, np.inf, -np.inf, np.nextafter(np.float32(5), np.float32(9)), -np.nextafter(np.float32(5), np.float32(0))):
        assert (x == np.float32(val)).any(), val
    assert ((x != 0) & (np.abs(x) < 1.1754944e-38)).sum() >= 4 and not np.isnan(x).any() and (np.abs(x) > 5).sum() > 100
    assert np.isnan(sg.clamp_data(5, 5.0, seed=2, nan_at=(4,))[4])
    ref = torch.clamp(torch.from_numpy(x), -5.0, 5.0).numpy()
    assert np.array_equal(ref.view(np.int32)[(np.abs(x) <= 5)], bits[(np.abs(x) <= 5)])     # in range: untouched bit for bit, -0.0 too
    assert sg.clamp_data(1, 5.0, seed=2).shape == (1,)
    # the other kind: no element survives the clamp unchanged, so a skipped one cannot hide
    for count in (1, 5, 1025):
        y = sg.clamp_data(count, 5.0, seed=2, outside=True)
        assert y.dtype == np.float32 and (np.abs(y) > 5.0).all() and np.isfinite(y).all()
        assert (y > 0).any() and (y < 0).any() or count == 1


def test_permute_shapes_cover_every_seam():
    shapes = sg.permute_shapes()
    assert len(set(shapes)) == len(shapes)
    for b in (1, 3):
        for w in sg.PERMUTE_WS:
            for ch in sg.PERMUTE_CHS:
                assert (b, ch, 1, w) in shapes
    assert (1, 9, 7, 32) in shapes and (3, 13, 5, 65) in shapes and (1, 26, 5, 1) in shapes and (2, 256, 7, 45) in shapes
    assert (1, 1, 1, 1) in shapes and (1, 64, 1, 32) in shapes                          # one element; exactly one tile
    x = sg.permute_data((3, 13, 5, 33), seed=1)
    assert x.shape == (3, 13, 5, 33) and not np.isnan(x).any() and (x.view(np.int32) == np.float32(-0.0).view(np.int32)).any()
