"""References, inputs and case lists of the step-glue suite (tests/test_step_glue_gpu.py runs them against vocr_clamp_adam, vocr_clamp,
the two permutes and the dropout draw on the GPU; tests/test_step_glue_ref_cpu.py holds this module to itself without one).  Importing
it needs numpy only.

vocr_clamp_adam
  adam_step64   one step of torch.optim.Adam (weight_decay added to the gradient, lerp of exp_avg, sqrt(v) / sqrt(bc2) + eps, lr / bc1)
                behind the reference's clamp of g * grad_scale, in float64.  Every scalar the C entry receives as `float` (lr, both betas,
                eps, weight_decay, clamp, grad_scale) is rounded to fp32 FIRST and 1 - beta, both bias corrections and lr / bc1 are then
                derived in double from the rounded values, as the entry point's host code does: the reference is the Adam the entry point
                was ASKED to run.  (That is not torch's Adam to the last bit: float(0.999) = 0.99900001287, so 1 - beta2 differs from
                Python's by 1.3e-5 relative - 216 u - and so does every v.  It is Adam with that beta2; the step count enters the bias
                corrections through the same value, so the two stay consistent.  A float ABI cannot do otherwise.)
  adam_bars     what one fp32 evaluation may differ from it by, per element, from the operands' magnitudes alone (u = 2^-24):
                    G     = |clamp(g gs)| + wd |p|         NOT |clamp(g gs) + wd p|: that sum can cancel, its rounding error cannot
                    bar_m = 4 u (|m| + G)                  m + (1 - b1)(g' - m): three roundings on terms bounded by |m| + G, one for 1 - b1
                    bar_v = 8 u (b2 v + (1 - b2) G^2)      v b2 + (1 - b2)(g' g'): g' carries 2 u, its square 4 u, + product, scale and sum
                    bar_p = 2 u |p'| + step_size bar_m / denom + 8 u |U|
                            the final subtraction (and its operand's), m's error carried through, and for U = step_size m' / denom:
                            half of v's relative error (< 2 u), sqrt, sqrt(bc2)'s own rounding, the division, + eps, m' / denom,
                            step_size's rounding and the product - eight roundings, each <= u with correctly rounded sqrt and division
                each with an absolute floor of 2^-100.
  adam_step32   the kernel's operation order in numpy float32 (no FMA), for the CPU test: it must sit inside the bars by itself.
  MUTANTS       six wrong Adams as variants of adam_step64; the CPU test shows that each leaves a bar by more than 100 x where it applies.
  adam_inputs   ONE generator for the CPU and the GPU test: p ~ N(0,1); gradient magnitudes log-uniform over 1e-9 .. 10; runs of eight
                exact 0, +clamp, -clamp, 2 clamp, -2 clamp; moments of the gradient's scale with every 7th pair zero; step 1: zero moments.

vocr_dropout_fwd / vocr_dropout_mask
  dropout_mask_ref   the stream's definition in numpy uint64: z = seed * 0x9e3779b97f4a7c15 + e (mod 2^64), splitmix64's finaliser, the
                     upper 32 bits >> 8, times 2^-24, keep iff u >= float32(p), scale float32(1) / (float32(1) - float32(p)).
vocr_clamp
  clamp_data    N(0, 4^2) with +-0, +-clamp, the floats next to +-clamp on both sides, +-inf and denormals at every third element; or
                every element beyond the clamp (an in-place kernel that skips an element shows only where the operation changes it)."""
import math

import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -100
F32 = np.float32

# ---------------------------------------------------------------------------------------------------------------- vocr_clamp_adam
ADAM_GRID_CAP = 4096 * 256                                  # threads of the capped launch: one trip of the grid-stride loop
ADAM_SMALL_COUNTS = (1, 255, 256, 257)
ADAM_LARGE_COUNTS = (ADAM_GRID_CAP - 1, ADAM_GRID_CAP, ADAM_GRID_CAP + 1, 2 * ADAM_GRID_CAP + 5)   # the last: a third trip
ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_WDS = (0.0, 0.01)
ADAM_SCALES = (1.0, 0.5, 1.0 / 3.0)
LR, BETA1, BETA2, EPS, CLAMP = 1e-3, 0.9, 0.999, 1e-8, 5.0
# every large count at these (step, wd, grad_scale): fresh moments + nothing else; saturating corrections + decay + a scale that rounds
ADAM_LARGE_SETTINGS = ((1, 0.0, 1.0), (1000, 0.01, 1.0 / 3.0))

MUTANTS = ("scale_after_clamp", "clamp_after_wd", "step_off_by_one", "eps_inside_bc2", "no_bc2", "decoupled_wd")


def mutant_applies(name, step, wd, grad_scale):
    """whether the wrong variant computes something else than Adam at this setting at all"""
    if name == "scale_after_clamp":
        return grad_scale != 1.0
    if name == "clamp_after_wd":                               # some gradient has to reach the clamp: adam_inputs' largest is 2 clamp
        return wd != 0.0 and 2.0 * _f(grad_scale) >= 1.0
    if name == "decoupled_wd":
        return wd != 0.0
    # the bias corrections: float(0.999) ** 100000 = e^-100 and 0.9 ** 1000 = 1.7e-46 are below double's resolution of 1
    return step <= 1000


def _f(x):
    return float(F32(x))


def _adam64(p, g, m, v, lr, beta1, beta2, eps, wd, clamp, grad_scale, step, variant=None):
    assert variant is None or variant in MUTANTS, variant
    lr, beta1, beta2, eps, wd, clamp, gs = (_f(x) for x in (lr, beta1, beta2, eps, wd, clamp, grad_scale))
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    s = step + 1 if variant == "step_off_by_one" else step
    bc1, bc2 = 1.0 - beta1 ** s, 1.0 - beta2 ** s
    with np.errstate(invalid="ignore", over="ignore"):
        gc = np.clip(g, -clamp, clamp) * gs if variant == "scale_after_clamp" else np.clip(g * gs, -clamp, clamp)   # NaN stays NaN
        base = p
        if variant == "clamp_after_wd":
            gd = np.clip(g * gs + wd * p, -clamp, clamp)
        elif variant == "decoupled_wd":
            gd, base = gc, p * (1.0 - lr * wd)
        else:
            gd = gc + wd * p
        m2 = m + (1.0 - beta1) * (gd - m)
        v2 = beta2 * v + (1.0 - beta2) * (gd * gd)
        root = np.sqrt(v2)
        if variant == "eps_inside_bc2":
            denom = (root + eps) / math.sqrt(bc2)
        elif variant == "no_bc2":
            denom = root + eps
        else:
            denom = root / math.sqrt(bc2) + eps
        step_size = lr / bc1
        upd = step_size * (m2 / denom)
        p2 = base - upd
    return p2, m2, v2, dict(gc=gc, denom=denom, upd=upd, step_size=step_size, beta2=beta2, wd=wd)


def adam_step64(p, g, m, v, lr, beta1, beta2, eps, wd, clamp, grad_scale, step, variant=None):
    """(p', m', v') in float64 from fp32 (or any) state; `variant`: one of MUTANTS, a wrong Adam"""
    return _adam64(p, g, m, v, lr, beta1, beta2, eps, wd, clamp, grad_scale, step, variant)[:3]


def adam_bars(p, g, m, v, lr, beta1, beta2, eps, wd, clamp, grad_scale, step):
    """(bar_p, bar_m, bar_v) per element (module docstring); NaN where the gradient is NaN"""
    p2, m2, v2, a = _adam64(p, g, m, v, lr, beta1, beta2, eps, wd, clamp, grad_scale, step)
    p, m, v = (np.asarray(x, dtype=np.float64) for x in (p, m, v))
    with np.errstate(invalid="ignore"):
        G = np.abs(a["gc"]) + a["wd"] * np.abs(p)
        bar_m = np.maximum(4 * U * (np.abs(m) + G), FLOOR)
        bar_v = np.maximum(8 * U * (a["beta2"] * v + (1.0 - a["beta2"]) * G * G), FLOOR)
        bar_p = np.maximum(2 * U * np.abs(p2) + a["step_size"] * bar_m / a["denom"] + 8 * U * np.abs(a["upd"]), FLOOR)
    return bar_p, bar_m, bar_v


def adam_ratios(got, ref, bars):
    """{"p" / "m" / "v": (worst |got - ref| / bar over the elements whose reference is finite, its element)}; got, ref, bars: (p, m, v)"""
    out = {}
    for name, x, r, b in zip("pmv", got, ref, bars):
        ok = np.isfinite(r)
        q = np.zeros(r.shape)
        with np.errstate(invalid="ignore"):
            q[ok] = np.abs(np.asarray(x, dtype=np.float64)[ok] - r[ok]) / b[ok]
        q[ok & ~np.isfinite(q)] = np.inf                       # a NaN or inf where the reference is finite
        i = int(np.argmax(q)) if q.size else 0
        out[name] = (float(q[i]) if q.size else 0.0, i)
    return out


def adam_step32(p, g, m, v, lr, beta1, beta2, eps, wd, clamp, grad_scale, step):
    """the kernel's operation order, one rounding per operation, in numpy float32; the host scalars as the entry point derives them"""
    lr, b1, b2, eps, wd, c, gs = (F32(x) for x in (lr, beta1, beta2, eps, wd, clamp, grad_scale))
    bc1, bc2 = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
    step_size, bc2_sqrt = F32(float(lr) / bc1), F32(math.sqrt(bc2))
    omb1, omb2 = F32(1.0 - float(b1)), F32(1.0 - float(b2))
    p, g, m, v = (np.asarray(a, dtype=F32) for a in (p, g, m, v))
    with np.errstate(invalid="ignore", over="ignore"):
        gr = g * gs
        gr = np.where(np.isnan(gr), gr, np.minimum(np.maximum(gr, -c), c))
        if wd != 0:
            gr = gr + wd * p
        mi = m + omb1 * (gr - m)
        vi = v * b2 + omb2 * (gr * gr)
        denom = np.sqrt(vi) / bc2_sqrt + eps
        p2 = p - step_size * (mi / denom)
    assert p2.dtype == F32 and mi.dtype == F32 and vi.dtype == F32
    return p2, mi, vi


def adam_inputs(count, step, seed, clamp=CLAMP):
    """(p, g, m, v) fp32 [count] (module docstring); a function of (count, step, seed) alone"""
    rng = np.random.default_rng([int(seed), int(count), int(step)])
    p = rng.standard_normal(count).astype(F32)
    mag = 10.0 ** rng.uniform(-9.0, 1.0, count)
    g = (mag * (rng.integers(0, 2, count) * 2 - 1)).astype(F32)
    run = (np.arange(count) // 8) % 16                          # runs of eight: the first run of a buffer keeps its random gradient
    for k, val in ((3, 0.0), (5, clamp), (6, -clamp), (7, 2 * clamp), (9, -2 * clamp)):
        g[run == k] = val
    if step == 1:
        return p, g, np.zeros(count, F32), np.zeros(count, F32)
    m = (mag * rng.standard_normal(count)).astype(F32)
    v = (mag * mag * rng.uniform(0.25, 4.0, count)).astype(F32)
    m[::7] = 0
    v[::7] = 0
    return p, g, m, v


def adam_idle(g, m, v):
    """elements with g = 0, m = 0, v = 0: without weight decay the step must keep p bit for bit"""
    return (g == 0) & (m == 0) & (v == 0)


# ---------------------------------------------------------------------------------------------------------------- vocr_clamp
EW_GRID_CAP = 2048 * 256 * 4                                # elements of one trip of the capped 16-byte loop
CLAMP_COUNTS = (1, 3, 4, 5, 1023, 1024, 1025, EW_GRID_CAP + 1029)
CLAMP_VALUES = (5.0, float("inf"))
OFFSETS = (0, 1, 2, 3)                                      # floats behind a 16-byte boundary; 1 .. 3: the all-scalar path


def clamp_data(count, clamp, seed, nan_at=(), outside=False):
    """outside=False: the special values among N(0, 4^2).  outside=True: every element beyond +-clamp (1.1 .. 3 clamp), so that the
    operation changes every element in place and one it skips shows - an element already in range looks the same clamped or not."""
    c = F32(clamp if math.isfinite(clamp) else 5.0)
    inf = F32(np.inf)
    rng = np.random.default_rng([int(seed), int(count), int(outside)])
    if outside:
        x = (c * rng.uniform(1.1, 3.0, count) * (rng.integers(0, 2, count) * 2 - 1)).astype(F32)
    else:
        specials = np.array([0.0, -0.0, c, -c, np.nextafter(c, inf), np.nextafter(c, F32(0)), -np.nextafter(c, inf), -np.nextafter(c, F32(0)),
                             inf, -inf, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.17549435e-38, 3.4028235e38, -3.4028235e38], dtype=F32)
        x = (rng.standard_normal(count) * 4.0).astype(F32)
        at = np.arange(0, count, 3)
        x[at] = specials[(at // 3) % len(specials)]
    for i in nan_at:
        x[i] = np.nan
    return x


# ---------------------------------------------------------------------------------------------------------------- the dropout draw
DROPOUT_COUNTS = (1, 3, 4, 5, 1025, EW_GRID_CAP + 1029)
DROPOUT_PS = (0.0, 0.3, 0.5)
DROPOUT_SEEDS = (0, 1, 0x5EED + 1000003 * 3, 1 << 63, (1 << 64) - 1)       # the third: what seed_rank gives rank 3
_GOLDEN = 0x9e3779b97f4a7c15
_M64 = (1 << 64) - 1


def mix64(z):
    """splitmix64's finaliser on a uint64 array"""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def mix64_int(z):
    """the same on one Python int (no numpy: what the array form is checked against)"""
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & _M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & _M64
    return z ^ (z >> 31)


def dropout_uniform_ref(n, seed, start=0):
    """fp32 [n]: the uniform of elements start .. start + n - 1 of stream `seed` (24 bits, in [0, 1))"""
    base = (int(seed) & _M64) * _GOLDEN & _M64
    z = mix64(np.uint64(base) + np.arange(start, start + n, dtype=np.uint64))          # (array arithmetic wraps mod 2^64)
    return ((z >> np.uint64(32)) >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)


def dropout_mask_ref(n, p, seed):
    """fp32 [n]: the pre-scaled keep mask of vocr_dropout_fwd / vocr_dropout_mask"""
    pf = F32(p)
    scale = F32(1.0) / (F32(1.0) - pf)
    return np.where(dropout_uniform_ref(n, seed) >= pf, scale, F32(0.0)).astype(F32)


def dropout_data(count, seed):
    """finite fp32 with -0.0 and denormals among N(0,1) (x * 0 and x * scale are then exact statements about bits)"""
    rng = np.random.default_rng([int(seed) & 0xFFFFFFFF, int(count)])
    x = rng.standard_normal(count).astype(F32)
    x[1::5] = -0.0
    x[2::11] = 1e-40
    x[3::13] = -1.4e-45
    return x


# ---------------------------------------------------------------------------------------------------------------- the permutes
PERMUTE_WS = (1, 31, 32, 33, 64, 65)                        # the 32-wide side of the LDS tile
PERMUTE_CHS = (1, 63, 64, 65, 128, 130)                     # the 64-wide side


def permute_shapes():
    """[(b, c, h, w)]: every w x every c h, reached as (c h, 1) and as (c h / h, h) for h = 5, 7 where it divides, b = 1 and 3; and the
    last CNN layer of the full-size model (256 channels x 7 rows: 28 tiles of 64) at a reduced width"""
    out = []
    for b in (1, 3):
        for w in PERMUTE_WS:
            for ch in PERMUTE_CHS:
                out.append((b, ch, 1, w))
                for h in (5, 7):
                    if ch % h == 0 and ch > h:
                        out.append((b, ch // h, h, w))
    out.append((2, 256, 7, 45))
    return out


def permute_data(shape, seed):
    rng = np.random.default_rng([int(seed)] + [int(s) for s in shape])
    x = rng.standard_normal(int(np.prod(shape))).astype(F32)
    x[1::7] = -0.0
    x[3::11] = 1e-40
    x[4::13] = 0.0
    return x.reshape(shape)
