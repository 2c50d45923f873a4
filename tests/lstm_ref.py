"""A CPU restatement of the BiLSTM recurrence of include/vocr.h (vocr_lstm_fwd / vocr_lstm_bwd_bias / vocr_lstm_bwd_parts), the yardstick of
tests/test_lstm_fp64_gpu.py.  Plain torch on the CPU, in float64 (the reference) or float32 (the same formulas in the library's sigmoid / tanh:
how far an exact-formula fp32 sweep lands from fp64, which the GPU bars are scaled by).  Vectorised over the batch, one loop over time.

Layouts (include/vocr.h): xproj [2][T][B][4H] (gate-major i, f, g, o: the x-projection plus both biases), W_hh [2][4H][H], lens descending.
Forward: y [T][B][2H] (zeros past lens), gates [2][T][B][H][4] (post-activation, interleaved per unit), cell [2][T][B][H]; the reverse
direction starts at each sequence's own last frame lens[b] - 1 with zero state.  Backward: dgates [2][T][B][4H] (the gradient with respect to
xproj = the pre-activation gates; zeros past lens) and dbias [2][4H] (its sum over frames).

`mutant` (tests of the bars only - tests/test_lstm_ref_cpu.py): "sigmoid" (a sigmoid 3e-4 too large), "stale" (the forward direction reads
h_{t-2} instead of h_{t-1} at one step), "rev_start" (the reverse direction starts every row at T - 1), "no_mask" (dy_mask ignored)."""
import torch

MUTANTS = ("sigmoid", "stale", "rev_start", "no_mask")
_STALE_STEP = 5          # the step whose recurrent input the "stale" mutant takes from one step too early


def _act(mutant):
    if mutant == "sigmoid":
        return lambda v: torch.sigmoid(v) * (1 + 3e-4)
    return torch.sigmoid


def _steps(T, d):
    return range(T) if d == 0 else range(T - 1, -1, -1)


def lstm_fwd(xproj, whh, lens, dtype=torch.float64, mutant=None):
    """-> (y [T][B][2H], gates [2][T][B][H][4], cell [2][T][B][H]) in `dtype`."""
    xp = xproj.to(dtype)
    w = whh.to(dtype)
    _, T, B, G = xp.shape
    H = G // 4
    lens_t = torch.as_tensor(list(lens), dtype=torch.int64)
    sig = _act(mutant)
    y = torch.zeros(T, B, 2 * H, dtype=dtype)
    gates = torch.zeros(2, T, B, H, 4, dtype=dtype)
    cell = torch.zeros(2, T, B, H, dtype=dtype)
    for d in range(2):
        h = torch.zeros(B, H, dtype=dtype)
        c = torch.zeros(B, H, dtype=dtype)
        hprev = h                                       # h two steps back (the "stale" mutant)
        wt = w[d].t()
        for t in _steps(T, d):
            act = (t < lens_t) if not (d == 1 and mutant == "rev_start") else torch.ones(B, dtype=torch.bool)
            hin = hprev if (d == 0 and mutant == "stale" and t == _STALE_STEP) else h
            pre = xp[d, t] + hin @ wt
            i, f, g, o = sig(pre[:, :H]), sig(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), sig(pre[:, 3 * H:])
            cn = f * c + i * g
            hn = o * torch.tanh(cn)
            a = act.unsqueeze(1)
            c = torch.where(a, cn, torch.zeros_like(cn))
            hprev, h = h, torch.where(a, hn, torch.zeros_like(hn))
            valid = (t < lens_t).unsqueeze(1)
            y[t, :, d * H:(d + 1) * H] = torch.where(valid, h, torch.zeros_like(h))
            cell[d, t] = torch.where(valid, c, torch.zeros_like(c))
            gates[d, t] = torch.where(valid.unsqueeze(2), torch.stack((i, f, g, o), dim=2), torch.zeros(1, 1, 1, dtype=dtype))
    return y, gates, cell


def lstm_bwd(dy, whh, lens, gates, cell, dy_mask=None, dtype=torch.float64, mutant=None):
    """dy [T][B][2H] (times dy_mask where given) -> (dgates [2][T][B][4H], dbias [2][4H]), from the forward's own gates and cell."""
    g_all = gates.to(dtype)
    c_all = cell.to(dtype)
    w = whh.to(dtype)
    dyv = dy.to(dtype)
    if dy_mask is not None and mutant != "no_mask":
        dyv = dyv * dy_mask.to(dtype)
    T, B = dyv.shape[:2]
    H = c_all.shape[-1]
    lens_t = torch.as_tensor(list(lens), dtype=torch.int64)
    dgates = torch.zeros(2, T, B, 4 * H, dtype=dtype)
    for d in range(2):
        dpre = torch.zeros(B, 4 * H, dtype=dtype)
        dcar = torch.zeros(B, H, dtype=dtype)             # dc_{t} f_{t} of the step processed before (the later one in the direction's order)
        for t in reversed(list(_steps(T, d))):
            valid = (t < lens_t).unsqueeze(1)
            tp = t - 1 if d == 0 else t + 1               # the direction's previous step
            cprev = c_all[d, tp] if 0 <= tp < T else torch.zeros(B, H, dtype=dtype)
            i, f, g, o = g_all[d, t].unbind(2)
            c = c_all[d, t]
            dh = dyv[t, :, d * H:(d + 1) * H] + dpre @ w[d]
            tc = torch.tanh(c)
            dc = dcar + dh * o * (1 - tc * tc)
            dpre = torch.cat((dc * g * i * (1 - i), dc * cprev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)), dim=1)
            dpre = torch.where(valid, dpre, torch.zeros_like(dpre))
            dcar = torch.where(valid, dc * f, torch.zeros_like(dc))
            dgates[d, t] = dpre
    return dgates, dgates.sum(dim=(1, 2))


def max_err(got, ref, valid=None):
    """max |got - ref| in float64 over the entries `valid` selects (a bool mask broadcast from the leading dims), every entry without it."""
    e = (got.double() - ref.double()).abs()
    if valid is not None:
        e = e[valid.expand(e.shape[:valid.dim()])]
    return float(e.max()) if e.numel() else 0.0


def valid_mask(T, B, lens):
    """[T][B] bool: frame (t, b) exists."""
    return torch.arange(T).unsqueeze(1) < torch.as_tensor(list(lens)).unsqueeze(0)


# ---- the bars of tests/test_lstm_fp64_gpu.py (the mutant tests of tests/test_lstm_ref_cpu.py hold them to having teeth).
# e_k = a kernel's max abs error against the fp64 restatement over valid entries; e_32 = the fp32 restatement's.  An fp32 sweep carries
# rounding through every step of the recurrence, so e_32 sets the floor no fp32 kernel can beat: 4 e_32 leaves room for the kernels'
# approximate transcendentals (v_exp / v_rcp sigmoid, the backward's polynomial tanh below |x| = 0.1: <= 2e-6 relative) and their own
# summation order.  The absolute terms come from bars the suite already holds fp32 kernels to: 3e-5 x max|X| between two persistent sweeps
# that differ only in summation order (test_persistent_sweeps_match_per_step_launches), 2e-5 for gemm_pair against fp64 (test_ops_gpu.py).
# A state (y, cell, gates) lies in [-1, 1] except a cell, which can grow with T: the bar scales with max(1, max|X64|).  A gradient has no
# natural scale: 5e-5 of its largest element; dbias sums T x B of them, so 5e-5 of the largest column sum of |dg64|.
STATE_ABS = 2e-5
GRAD_REL = 5e-5
E32_FACTOR = 4.0


def bar(what, ref64, e32):
    """The bar of quantity `what` ("y", "cell", "gates", "dgates", "dbias") whose fp64 reference is `ref64` (valid entries only for the
    states; dgates: the whole tensor, zeros past lens; dbias: the [2][T][B][4H] dgates it sums)."""
    r = ref64.double().abs()
    if what in ("y", "cell", "gates"):
        base = STATE_ABS * max(1.0, float(r.max()) if r.numel() else 0.0)
    elif what == "dgates":
        base = GRAD_REL * float(r.max())
    elif what == "dbias":
        base = GRAD_REL * float(r.sum(dim=(1, 2)).max())
    else:
        raise ValueError(what)
    return max(base, E32_FACTOR * e32)


class Refs(object):
    """fp64 and fp32 restatements of one case (forward, and backward from dy / dy_mask)."""

    def __init__(self, xproj, whh, lens, dy, dy_mask=None):
        T, B = xproj.shape[1:3]
        self.lens, self.valid = list(lens), valid_mask(T, B, lens)
        self.f64 = lstm_fwd(xproj, whh, lens, torch.float64)
        self.f32 = lstm_fwd(xproj, whh, lens, torch.float32)
        self.b64 = lstm_bwd(dy, whh, lens, self.f64[1], self.f64[2], dy_mask, torch.float64)
        self.b32 = lstm_bwd(dy, whh, lens, self.f32[1], self.f32[2], dy_mask, torch.float32)

    def errors(self, fwd, bwd=None):
        """[(name, e_k, e_32, bar)] of a candidate's forward (y, gates, cell in the restatement's layouts) and backward (dgates, dbias)."""
        v = self.valid
        vd = v.unsqueeze(0).expand(2, *v.shape)          # [2][T][B]
        out = []
        for nm, k, r64, r32, m in (("y", fwd[0], self.f64[0], self.f32[0], v), ("gates", fwd[1], self.f64[1], self.f32[1], vd),
                                   ("cell", fwd[2], self.f64[2], self.f32[2], vd)):
            e32 = max_err(r32, r64, m)
            out.append((nm, max_err(k, r64, m), e32, bar(nm, r64[m], e32)))
        if bwd is not None:
            e32 = max_err(self.b32[0], self.b64[0], vd)
            out.append(("dgates", max_err(bwd[0], self.b64[0], vd), e32, bar("dgates", self.b64[0], e32)))
            if bwd[1] is not None:
                e32 = max_err(self.b32[1], self.b64[1])
                out.append(("dbias", max_err(bwd[1], self.b64[1]), e32, bar("dbias", self.b64[0], e32)))
        return out


def failures(errs):
    return [(nm, ek, e32, b) for nm, ek, e32, b in errs if not ek <= b]
