"""The cases tests/test_lstm_fp64_gpu.py (every sweep kind against fp64) and tests/test_lstm_guarded_gpu.py (every LSTM entry point in
guarded memory) share: the host plan's sweep rule restated, ragged length lists, random inputs of three regimes and their fp64 / fp32
restatements (tests/lstm_ref.py), computed once per case.  Data only; importing this module needs no GPU and no library.

GUARDED_CASES are the smallest shapes at which each sweep kind can still go wrong: T = 11 wraps the forward hand-off ring's 4 step
slots more than twice and passes both parities of the backward partial blocks; ragged lengths run from 11 down to 1."""
import torch

from tests import lstm_ref as lr

CUS = 256          # MI355X compute units: resident_workgroup_capacity() of lstm.hip
_ALL = ("wide4", "chain4", "chain16", "step")
# every setting of the library's two switches (one child process each); write-through only changes the persistent kinds
SETTINGS = ("step", "wide4", "chain4", "chain16", "wide4/wt", "chain4/wt", "chain16/wt")


def sweep_kind(backward, B, H, floor, rows=None, cap=CUS):
    """lstm_sweep_kind of lstm.hip (the table at its head) for floor = VOCR_LSTM_SWEEP: wide4 < chain4 < chain16 < step."""
    order = ("wide4", "chain4", "chain16", "step")
    fl = order.index(floor)
    if backward:
        ok = H in (128, 256, 512) and 8 * (H // 16) <= cap
    else:
        ok = H in (64, 128, 256, 512) and (rows if rows else 0) * 2 * H * 4 < 2 ** 31 and 8 * (H // 16) <= cap
    if not ok or fl == 3:
        return "step"
    nt4 = (B + 3) // 4
    if fl <= 0 and H == 512 and 4 < nt4 <= 8 and 256 <= cap:
        return "wide4"
    if fl <= 1 and 2 * nt4 <= 16 and H in (256, 512) and (16 if 2 * nt4 > 8 else 8) * (H // 16) <= 2 * cap:
        return "chain4"
    return "chain16"


def _ragged(T, B):
    """descending, first T, last 1"""
    if B == 1:
        return [T]
    return sorted([max(1, T - (T * i) // (B - 1)) for i in range(B)], reverse=True)


def make_inputs(T, B, H, lens, regime, seed):
    """fp32 inputs of one case (the kernels' own values; the references read them exactly): xproj [2][T][B][4H], W_hh [2][4H][H],
    dy [T][B][2H], dy_mask [T][B][2H] (0 or 2: dy * mask is exact in fp32, so vocr_lstm_bwd_bias on the product and vocr_lstm_bwd_parts on
    the pair answer to one reference)."""
    g = torch.Generator().manual_seed(seed)

    def u(*s):
        return torch.rand(*s, generator=g) * 2 - 1

    if regime == "ref":                       # the reference model's init scale
        xproj, whh = u(2, T, B, 4 * H) * 0.5, u(2, 4 * H, H) * 0.08
    elif regime == "sat":                     # gates at 0 or 1, tanh at +-1, and a few pre-activations whose exp overflows to inf
        xproj, whh = u(2, T, B, 4 * H) * 8, u(2, 4 * H, H) * 0.3
        n = xproj.numel()
        idx = torch.randint(0, n, (max(8, n // 500),), generator=g)
        xproj.view(-1)[idx] = torch.where(torch.rand(idx.numel(), generator=g) < 0.5, -100.0, 100.0)
    else:                                     # small cells: f ~ 0.0025, i ~ 1, g in +-0.2 - |c| straddles tanhf_'s switch at 0.1
        xproj = torch.empty(2, T, B, 4, H)
        xproj[:, :, :, 0] = 6 + u(2, T, B, H) * 0.5
        xproj[:, :, :, 1] = -6 + u(2, T, B, H) * 0.5
        xproj[:, :, :, 2] = u(2, T, B, H) * 0.2
        xproj[:, :, :, 3] = u(2, T, B, H) * 0.5
        xproj = xproj.reshape(2, T, B, 4 * H)
        whh = u(2, 4 * H, H) * 0.02
    for b in range(B):
        xproj[:, lens[b]:, b] = 0.37              # junk past the lengths must not leak
    dy = u(T, B, 2 * H)
    mask = (torch.rand(T, B, 2 * H, generator=g) < 0.5).float() * 2.0
    return xproj.contiguous(), whh.contiguous(), dy, mask


_CACHE = {}


def case(T, B, H, lens_kind, regime):
    key = (T, B, H, lens_kind, regime)
    if key not in _CACHE:
        lens = [T] * B if lens_kind == "full" else _ragged(T, B)
        seed = (T * 1000 + B) * 10000 + H + ("ref", "sat", "small").index(regime)
        xproj, whh, dy, mask = make_inputs(T, B, H, lens, regime, seed)
        refs = lr.Refs(xproj, whh, lens, dy, mask)
        if regime == "small":
            c = refs.f64[2].abs()[:, refs.valid]
            frac = float(((c >= 0.05) & (c <= 0.15)).double().mean())
            assert frac >= 0.10, "small-cell regime: only %.3f of the valid cells have |c| in [0.05, 0.15]" % frac
        _CACHE[key] = (lens, xproj, whh, dy, mask, refs)
    return _CACHE[key]


# ---- the guarded suite's table: (T, B, H, lens kind).  What each (B, H) reaches forward / backward at the floors that change it
# (sweep_kind above; a floor below a shape's own kind changes nothing, floor `step` gives step / step everywhere):
#   32, 17 x 512    wide4: wide4 / wide4     chain4: chain4 / chain4    chain16: chain16 / chain16
#   16 x 512        wide4, chain4: chain4 / chain4 (nt4 = 4: no wide members)             chain16: chain16 / chain16
#   7, 30 x 256     wide4, chain4: chain4 / chain4 (a partial last chain)                 chain16: chain16 / chain16
#   33 x 128        every floor but step: chain16 / chain16
#   64 x 512        every floor but step: chain16 / chain16 (nt4 = 16)
#   48 x 64         every floor but step: chain16 forward / step backward (no backward fast path below H = 128)
#   5 x 48, 3 x 16  step / step (the generic per-step kernels) at every floor
#   1 x 1 x 256 (T = 1, full) and 2 x 3 x 512 (T = 2): wide4, chain4: chain4 / chain4       chain16: chain16 / chain16
GUARDED_T = 11
GUARDED_CASES = [
    (11, 32, 512, "ragged"),
    (11, 17, 512, "ragged"),
    (11, 16, 512, "ragged"),
    (11, 7, 256, "ragged"),
    (11, 30, 256, "ragged"),
    (11, 33, 128, "ragged"),
    (11, 64, 512, "ragged"),
    (11, 48, 64, "ragged"),
    (11, 5, 48, "ragged"),
    (11, 3, 16, "ragged"),
    (1, 1, 256, "full"),
    (2, 3, 512, "ragged"),
]
# the case whose leftovers a case finds in its workspace in the "foreign workspace" run: another shape, and at the default setting
# another kind (wide4 <-> chain16, chain4 <-> chain16 / step, step <-> chain4)
DONOR = {
    (11, 32, 512): (11, 33, 128), (11, 17, 512): (11, 64, 512), (11, 16, 512): (11, 48, 64), (11, 7, 256): (11, 64, 512),
    (11, 30, 256): (11, 5, 48), (11, 33, 128): (11, 32, 512), (11, 64, 512): (11, 30, 256), (11, 48, 64): (11, 17, 512),
    (11, 5, 48): (11, 7, 256), (11, 3, 16): (11, 16, 512), (1, 1, 256): (11, 33, 128), (2, 3, 512): (11, 3, 16),
}
# shapes of the unaligned-pointer runs (H = 128 and 512: the generic per-step kernels at sizes the fast paths otherwise take)
UNALIGNED_CASES = [(11, 33, 128), (11, 17, 512)]
RANGE_CUTS = (1, 4, 5, GUARDED_T - 1)
# the packed child: wide members, a partial last chain at H = 256, fewer than two whole chains, exactly one chain
PACKED_CASES = [(11, 32, 512), (11, 30, 256), (11, 7, 256), (11, 4, 256)]


def guarded_case(T, B, H):
    """(lens kind, case(...)) of a shape of GUARDED_CASES / PACKED_CASES (regime "ref")"""
    kinds = [c[3] for c in GUARDED_CASES if c[:3] == (T, B, H)]
    lk = kinds[0] if kinds else "ragged"
    return lk, case(T, B, H, lk, "ref")


def packed_layout(lens, T, B):
    """The packed row layout's definition (include/vocr.h): groups [zero][chain 0][zero][chain 1]...[zero], 4 rows per group ->
    (rows, to_packed [T*B], to_dense [rows]) as lists, -1 where the other layout has no such row."""
    nch = (B + 3) // 4
    rows = 4 * (sum(min(lens[4 * c], T) for c in range(nch)) + nch + 1)
    to_packed, to_dense = [-1] * (T * B), [-1] * rows
    g = 1
    for c in range(nch):
        L = min(lens[4 * c], T)
        for t in range(L):
            for j in range(4):
                b = 4 * c + j
                if b < B:
                    to_packed[t * B + b] = 4 * (g + t) + j
                    to_dense[4 * (g + t) + j] = t * B + b
        g += L + 1
    return rows, to_packed, to_dense
