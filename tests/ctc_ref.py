"""An fp64 restatement of the CTC criterion of include/vocr.h (vocr_ctc_loss_grad: per-line negative log-likelihood and its gradient
with respect to the pre-softmax activations), the yardstick of tests/test_ctc_fp64_gpu.py.  Plain torch on the CPU, vectorised over the
extended-label positions and the batch, one loop over time.  Conventions are those of include/vocr.h and oracle/ctc_ref.c: blank 0, the
skip s-2 -> s only between different labels, gradient rows zero for t >= act_len, act_len == 0: nll 0 for an empty labelling and +inf
otherwise, an infeasible line: nll +inf and zero occupancy (its gradient is the softmax row, finite).

`ctc(..., dtype=torch.float32)` runs the KERNEL's formulas in fp32 (form="kernel": the max-shifted three-way logsumexp of lse3, nll from
the last two positions, the blank occupancy as one max-shifted sum and the label occupancies folded in label order,
exp(lp) - exp(acc + nll - lp)) or those of oracle/ctc_ref.c (form="pairwise": nested two-way logsumexps everywhere).  Their distance from
fp64 is e_32; both must stay within a quarter of every bar, so no bar is tuned to one summation order.

---- the bars.  Fixed constants times scales computed from fp64 quantities only; nothing comes from a kernel's output.
ulp32(v) is the spacing of fp32 numbers at |v|.  First-order error propagation of the fp32 computation:

* one log-softmax element lp = x - (m + logf(sum)): the rounding of lse at |lse|, of logf(sum) at |lse - m| <= max|x| + |lse| and of the
  subtraction at |lp| <= max|x| + |lse|:                       e_lp[t,b] = ulp32(max_v |x[t,b,v]| + |lse[t,b]|)     (one number per row).
* one recursion step alpha_t(s) = lse3(...) + lp_t(l'_s) commits e_lp, the rounding of the log term (a value in [0, ln 3]: ulp32(2)) and
  the rounding of the sum at |alpha_t(s)|.  d nll / d alpha_t(s) is the posterior occupancy g_t(s) of state s at frame t (sum_s g_t(s)
  = 1), so the local errors reach nll weighted by g and ADD over the frames:
      s_a[b] = sum_{t < act_len} ( e_lp[t,b] + ulp32(2) + sum_s g_t(s) ulp32(|alpha_t(s)|) ) + ulp32(|nll|)
  and s_b[b] the same with beta.  The nll error is therefore ABSOLUTE, linear in the number of frames and in the per-frame rounding of
  x - lse; it grows with |nll| only through the ulp of the running alpha on the occupied states.  This is the worst case (every rounding
  in the same direction); random roundings land ~ 1 / sqrt(frames) below it, which is why the fp32 restatements use under 6% of the nll
  bar at T >= 294 and up to 14% at T <= 21 (measured fractions below).
      nll bar  = C_NLL * s_a[b]
* grad = y - occ, y = expf(lp), occ = expf(acc + nll - lp), acc = logsumexp_{s: l'_s = v} (alpha_t(s) + beta_t(s)):
      err(y)   <= y (e_lp + 2 U)                                              (argument error, expf and its rounding)
      err(occ) <= occ (err(alpha) + err(beta) + err(nll) + e_lp + roundings of the sums at |alpha + beta|, |acc + nll - lp|)
               <= occ (2 s_a + s_b + e_lp + 2 ulp32(|acc| + |nll| + |lp|))
      grad bar = C_GRAD * ( y (e_lp + 2 U) + occ (2 s_a + s_b + e_lp + 2 ulp32(|acc| + |nll| + |lp|)) ) + 2^-126
  (2^-126: a device expf may flush a subnormal result).  Rows t >= act_len, +-inf and the nll of empty / infeasible lines carry a bar of
  0: they are compared exactly.

C_NLL = 2, C_GRAD = 6.  The analysis bounds the error by ~1x the scale for correctly rounded libm functions.  The gradient has millions of
elements, so some element does meet the worst rounding of x - lse: the fp32 restatements sit at ~1.2x the y-term of the scale on every
case, and 6 puts that at a fifth of the bar.  The nll of a line is one number per line; 2 leaves the shortest lines (T <= 21, where the
roundings cannot average out) at <= 0.14.  Both leave the quarter of headroom the device needs: its expf / logf are 1-2 ulp functions where
libm's are <= 1, and the kernel's blank reduction sums in wave order.  Measured on the CPU over every (case, regime) of GPU_CASES, both fp32
formulations (tests/test_ctc_ref_cpu.py asserts <= 0.25 for each):
      worst fraction of the nll bar used   0.136   (both forms: the 21-frame B70 lines; 0.10 at the 7-frame V = 4096 lines, <= 0.06 at T >= 294)
      worst fraction of the grad bar used  0.207   (both forms: B70 dense; 0.14 - 0.20 on every other case)
These are numbers of the CPU's libm, not of the MI355X; the GPU run's own table is `profiles/ctc_fp64_errors.txt` (the kernels used at most
0.17 of an nll bar and 0.28 of a gradient bar).

What each regime can judge.  The occupancy part of the gradient scale is linear in T and, through ulp32(|alpha|), in |nll|.  On the dense
1200-frame case (nll ~ 6000, two full-length lines) it is ~0.2 occ, and the subtle mutants pass or nearly pass (measured on the CPU: dup
and beta_start 0.19 of a bar, nll_one 0.31, seam 3.4); only what shows in the y term or moves whole occupancies misses by >= 10x there
(lp_eps 15.7x, prefetch 58x, skip_repeat 368x).  `peaky` (nll <= ~160, ulp32(|alpha|) <= 1.6e-5) and `tight` (one feasible path: closed
form) catch every mutant by >= 10x, which tests/test_ctc_ref_cpu.py asserts on MUTANT_CASES (measured: lp_eps 25 - 41x through the nll bar,
dup and beta_start >= 167x, seam 6e39x on the peaky 588 x 32 x 166 case, the rest >= 1e4x; seam needs a line with L >= 32, beta_start a
ragged batch, dup a repeated class).
"""
import numpy as np
import torch

U = 2.0 ** -24                       # unit roundoff of fp32
C_NLL = 2.0
C_GRAD = 6.0
NEG = float("-inf")
PF = 8                               # prefetch depth of the register kernels of ctc.hip

MUTANTS = ("skip_repeat", "seam", "prefetch", "beta_start", "dup", "nll_one", "lp_eps", "no_mask")


def ulp32(v):
    """spacing of fp32 at |v| (v a float64 tensor; inf and nan map to the spacing at 2^-126)"""
    v = torch.nan_to_num(v.abs(), nan=0.0, posinf=0.0).clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(v)) - 23)


# ------------------------------------------------------------------------------------------------------------------- the restatement
def _lse2(a, b):
    m = torch.maximum(a, b)
    ms = torch.where(m == NEG, torch.zeros_like(m), m)
    return torch.log(torch.exp(a - ms) + torch.exp(b - ms)) + ms


def _lse3(a, b, c, form):
    if form == "pairwise":
        return _lse2(_lse2(a, b), c)
    m = torch.maximum(a, torch.maximum(b, c))
    ms = torch.where(m == NEG, torch.zeros_like(m), m)
    return torch.log(torch.exp(a - ms) + torch.exp(b - ms) + torch.exp(c - ms)) + ms


def _shift(x, k):
    """y[..., s] = x[..., s - k] (k > 0) or x[..., s + |k|] (k < 0), -inf shifted in"""
    pad = torch.full_like(x[..., :abs(k)], NEG)
    if k > 0:
        return torch.cat((pad, x[..., :-k]), -1)
    return torch.cat((x[..., -k:], pad), -1)


def _layout(labels, label_lens, V):
    """ext [B,Sm] (0 = blank, also past S), valid [B,Sm], offsets"""
    ll = [int(v) for v in label_lens]
    lab = [int(v) for v in labels]
    assert sum(ll) <= len(lab)
    B = len(ll)
    sm = 2 * max(ll + [0]) + 1
    sm = max(sm, 3)
    ext = torch.zeros(B, sm, dtype=torch.long)
    valid = torch.zeros(B, sm, dtype=torch.bool)
    off = 0
    for b, L in enumerate(ll):
        row = lab[off:off + L]
        assert all(1 <= v < V for v in row), "labels must lie in [1, V)"
        ext[b, 1:2 * L:2] = torch.tensor(row, dtype=torch.long)
        valid[b, :2 * L + 1] = True
        off += L
    return ext, valid, ll


def _run(logits, labels, label_lens, act_lens, dtype=torch.float64, mutant=None, form="kernel"):
    assert mutant is None or mutant in MUTANTS
    assert form in ("kernel", "pairwise")
    T, B, V = logits.shape
    ext, valid, ll = _layout(labels, label_lens, V)
    sm = ext.shape[1]
    tb = torch.tensor([int(v) for v in act_lens], dtype=torch.long)
    assert int(tb.max()) <= T and int(tb.min()) >= 0
    S = torch.tensor([2 * L + 1 for L in ll], dtype=torch.long)
    x = logits.to(dtype)
    m = x.max(2, keepdim=True)[0]
    lse = m + torch.log(torch.exp(x - m).sum(2, keepdim=True))
    lp = x - lse
    if mutant == "lp_eps":
        lp = lp + 1e-4
    lpe = lp.gather(2, ext.unsqueeze(0).expand(T, B, sm))                     # lp[t][b][l'_s]
    pos = torch.arange(sm).unsqueeze(0)
    e_m2, e_p2 = torch.roll(ext, 2, 1), torch.roll(ext, -2, 1)
    if mutant == "skip_repeat":
        skip_a = (pos >= 2) & (ext != 0)
        skip_b = (pos + 2 < S.unsqueeze(1)) & (ext != 0)
    else:
        skip_a = (pos >= 2) & (ext != 0) & (ext != e_m2)
        skip_b = (pos + 2 < S.unsqueeze(1)) & (ext != 0) & (ext != e_p2)
    ninf = torch.full((B, sm), NEG, dtype=dtype)
    bi = torch.arange(B)

    alpha = torch.full((T, B, sm), NEG, dtype=dtype)
    a0 = ninf.clone()
    a0[:, 0] = lp[0, :, 0]
    a0[:, 1] = torch.where(S > 1, lpe[0, :, 1], a0[:, 1])
    alpha[0] = torch.where((tb > 0).unsqueeze(1), a0, ninf)
    for t in range(1, T):
        prev = alpha[t - 1]
        a2 = _shift(prev, 1)
        if mutant == "seam" and sm > 64:
            a2 = a2.clone()
            a2[:, 64] = NEG
        a3 = torch.where(skip_a, _shift(prev, 2), ninf)
        l = _lse3(prev, a2, a3, form)
        e = lpe[t]
        if mutant == "prefetch" and t == PF + 1:
            e = lpe[torch.minimum(torch.full_like(tb, t + 1), (tb - 1).clamp_min(0)), bi]
        new = torch.where(valid & (l != NEG), l + e, ninf)
        alpha[t] = torch.where((t < tb).unsqueeze(1), new, ninf)

    beta = torch.full((T, B, sm), NEG, dtype=dtype)
    start = torch.where(tb > 0, torch.full_like(tb, T), tb) if mutant == "beta_start" else tb
    for t in range(T - 1, -1, -1):
        if t + 1 < T:
            nxt = beta[t + 1]
            b3 = torch.where(skip_b, _shift(nxt, -2), ninf)
            l = _lse3(nxt, _shift(nxt, -1), b3, form)
            new = torch.where(valid & (l != NEG), l + lpe[t], ninf)
        else:
            new = ninf
        first = ninf.clone()
        first[bi, S - 1] = lp[t, :, 0]
        sl = (S - 2).clamp_min(0)
        first[bi, sl] = torch.where(S > 1, lpe[t, bi, sl], first[bi, sl])
        new = torch.where((start - 1 == t).unsqueeze(1), first, new)
        beta[t] = torch.where((t < start).unsqueeze(1), new, ninf)

    last = alpha[(tb - 1).clamp_min(0), bi]                                     # [B, sm]
    a = last[bi, S - 1]
    c = torch.where(S > 1, last[bi, (S - 2).clamp_min(0)], torch.full_like(a, NEG))
    if mutant == "nll_one":
        c = torch.full_like(a, NEG)
    nll = -_lse2(a, c)
    nll = torch.where(tb > 0, nll, torch.where(S == 1, torch.zeros_like(nll), torch.full_like(nll, float("inf"))))

    ab = alpha + beta
    acc = torch.full((T, B, V), NEG, dtype=dtype)
    if form == "kernel":
        xb = ab[:, :, 0::2]
        mb = xb.max(2, keepdim=True)[0]
        ms = torch.where(mb == NEG, torch.zeros_like(mb), mb)
        acc[:, :, 0:1] = ms + torch.log(torch.exp(xb - ms).sum(2, keepdim=True))
        order = range(1, sm, 2)
    else:
        order = range(sm)
    for s in order:
        idx = ext[:, s].view(1, B, 1).expand(T, B, 1)
        cur = acc.gather(2, idx)
        xs = ab[:, :, s:s + 1]
        new = _lse2(cur, xs)
        if mutant == "dup" and (s & 1):
            new = torch.where(valid[:, s].view(1, B, 1), xs, cur)
        acc.scatter_(2, idx, new)
    y = torch.exp(lp)
    nl = nll.view(1, B, 1)
    occ = torch.where((acc == NEG) | torch.isinf(nl), torch.zeros_like(acc), torch.exp(acc + nl - lp))
    grad = y - occ
    live = (torch.arange(T).unsqueeze(1) < tb.unsqueeze(0)).unsqueeze(2)       # [T,B,1]
    if mutant != "no_mask":
        grad = torch.where(live, grad, torch.zeros_like(grad))
    return dict(nll=nll, grad=grad, alpha=alpha, beta=beta, lp=lp, lse=lse, lpe=lpe, acc=acc, y=y, occ=occ, live=live, x=x, tb=tb, S=S)


def ctc(logits, labels, label_lens, act_lens, dtype=torch.float64, mutant=None, form="kernel"):
    """(nll [B], grad [T,B,V], alpha [T,B,Sm], beta [T,B,Sm]) of logits [T,B,V] (pre-softmax), flat labels, label_lens [B], act_lens
    [B], computed in `dtype`; rows t >= act_len of alpha / beta are -inf.  `mutant`: one of MUTANTS (for testing the bars only)."""
    r = _run(logits, labels, label_lens, act_lens, dtype, mutant, form)
    return r["nll"], r["grad"], r["alpha"], r["beta"]


class Reference:
    """the fp64 answer of one case and its bars (see the head of the file)"""

    def __init__(self, logits, labels, label_lens, act_lens):
        r = _run(logits, labels, label_lens, act_lens, torch.float64)
        self.nll, self.grad, self.alpha, self.beta = r["nll"], r["grad"], r["alpha"], r["beta"]
        T, B, V = logits.shape
        nll, live = r["nll"], r["live"]
        finite = torch.isfinite(nll) & (r["tb"] > 0)
        e_lp = ulp32(r["x"].abs().max(2, keepdim=True)[0] + r["lse"].abs())      # [T,B,1]
        nl = torch.where(finite, nll, torch.zeros_like(nll)).view(1, B, 1)
        gam = torch.exp(r["alpha"] + r["beta"] - r["lpe"] + nl)                    # posterior occupancy of (t, s); 0 where unreachable
        gam = torch.where(finite.view(1, B, 1), gam, torch.zeros_like(gam))

        def side(v):
            w = torch.where(gam > 0, gam * ulp32(v), torch.zeros_like(gam)).sum(2, keepdim=True)
            per_t = torch.where(live, e_lp + ulp32(torch.tensor(2.0, dtype=torch.float64)) + w, torch.zeros_like(e_lp))
            return per_t.sum(0).view(B) + ulp32(nll)
        s_a, s_b = side(r["alpha"]), side(r["beta"])
        self.s_a = s_a
        self.nll_bar = torch.where(finite, C_NLL * s_a, torch.zeros_like(s_a))
        mag = torch.nan_to_num(r["acc"].abs(), posinf=0.0) + nl.abs() + r["lp"].abs()
        e_occ = (2 * s_a + s_b).view(1, B, 1) + e_lp + 2 * ulp32(mag)
        bar = C_GRAD * (r["y"] * (e_lp + 2 * U) + r["occ"] * e_occ) + 2.0 ** -126
        self.grad_bar = torch.where(live, bar, torch.zeros_like(bar))


def ratio(got, ref, bar):
    """max over elements of |got - ref| / bar; elements that are EQUAL (+-inf included) count 0, a difference where the bar is 0
    (rows and values that are compared exactly) counts inf, and so does a NaN."""
    got = got.double()
    d = torch.where(got == ref, torch.zeros_like(ref), (got - ref).abs())
    d = torch.nan_to_num(d, nan=float("inf"), posinf=float("inf"))
    r = torch.where(d == 0, torch.zeros_like(d), d / bar)                     # x / 0 = inf
    return float(r.max()) if r.numel() else 0.0


def max_err(got, ref):
    """max |got - ref| over the elements where both are finite"""
    got = got.double()
    ok = torch.isfinite(got) & torch.isfinite(ref)
    return float((got - ref)[ok].abs().max()) if bool(ok.any()) else 0.0


# ------------------------------------------------------------------------------------------------------------------------- builders
def need(lab):
    """the fewest frames a labelling takes: one per label and a blank between equal neighbours"""
    return len(lab) + sum(1 for i in range(1, len(lab)) if lab[i] == lab[i - 1])


def make_labels(rng, V, L, kind):
    """"random": uniform in [1, V) with a repeat at the front, class 1 and class V - 1 present; "equal": one class L times (the skip is
    never legal); "abab": two classes alternating (the skip is always legal, each class accumulates from L / 2 positions)"""
    if L == 0:
        return []
    if kind == "equal" or V == 2:
        return [int(rng.integers(1, V))] * L
    if kind == "abab":
        a = int(rng.integers(1, V))
        b = 1 + (a % (V - 1))
        return [a if i % 2 == 0 else b for i in range(L)]
    lab = [int(v) for v in rng.integers(1, V, L)]
    if L >= 2:
        lab[1] = lab[0]
    if L >= 4:
        lab[2], lab[-1] = 1, V - 1
    return lab


def random_alignment(rng, lab, Tb):
    """a random valid CTC path (class per frame, length Tb) of `lab`, or None if Tb < need(lab); optional blanks are kept with
    probability 1/2 where the length allows, the spare frames spread at random"""
    if Tb < need(lab) or Tb == 0:
        return None
    toks = []                                                 # [class, is an optional blank]
    for i, v in enumerate(lab):
        if i > 0 and lab[i - 1] == v:
            toks.append([0, False])
        elif rng.random() < 0.5:
            toks.append([0, True])
        toks.append([v, False])
    if not lab or rng.random() < 0.5:
        toks.append([0, bool(lab)])
    while len(toks) > Tb:
        opt = [i for i, tk in enumerate(toks) if tk[1]]
        del toks[opt[int(rng.integers(len(opt)))]]
    toks = [tk[0] for tk in toks]
    dur = np.ones(len(toks), dtype=np.int64) + rng.multinomial(Tb - len(toks), np.ones(len(toks)) / len(toks))
    return [v for v, d in zip(toks, dur) for _ in range(int(d))]


def build_logits(rng, T, B, V, labs, act, regime):
    """fp32 logits [T,B,V] of one regime:
    ("dense", a): uniform +-a;   ("peaky", margin, noise): N(0, noise) plus `margin` on a random valid alignment of each feasible line;
    ("saturated",): uniform +-scale with a scale in [30, 60] per line (log-probabilities near -100) and every 7th row all equal."""
    kind = regime[0]
    if kind == "dense":
        return torch.from_numpy(((rng.random((T, B, V)) * 2 - 1) * regime[1]).astype(np.float32))
    if kind == "saturated":
        x = (rng.random((T, B, V)) * 2 - 1) * rng.uniform(30, 60, (1, B, 1))
        x[::7] = rng.uniform(-40, 40, (len(range(0, T, 7)), B, 1))
        return torch.from_numpy(x.astype(np.float32))
    assert kind == "peaky"
    margin, noise = regime[1], regime[2]
    x = rng.normal(0, noise, (T, B, V))
    for b in range(B):
        path = random_alignment(rng, labs[b], act[b])
        if path is not None:
            x[np.arange(act[b]), b, np.array(path)] += margin
    return torch.from_numpy(x.astype(np.float32))


def _ragged(T, B, needs):
    """descending from T to ~T / 10, never below what the line's labelling takes (so late long lines are exactly tight)"""
    return [max(needs[i], 1, int(round(T * (1 - 0.9 * i / max(B - 1, 1))))) for i in range(B)]


DENSE, PEAKY8, PEAKY15, PEAKY4, SAT = ("dense", 3.0), ("peaky", 8.0, 1.0), ("peaky", 15.0, 1.0), ("peaky", 4.0, 2.0), ("saturated",)
_L_BENCH = [31, 20, 12, 31, 25, 1, 17, 30, 8, 31, 22, 0, 14, 29, 5, 31, 19, 27, 3, 16, 31, 10, 24, 2, 28, 13, 21, 7, 30, 18, 26, 9]
_L_C4 = [63, 62, 33, 32, 31, 7, 0, 63, 40, 50, 33, 32, 31, 7, 0, 62, 63, 45, 36, 32, 31, 7, 0, 33, 58, 12, 63, 32, 31, 7, 0, 3]

# name, T, B, V, label counts, label kinds (one, or one per line), act_lens ("full", "ragged", "tight", or a list; "tight": need(lab)
# for the first half of the lines and need(lab) + 1 for the second), regimes
GPU_CASES = [
    ("bench_full", 294, 32, 96, _L_BENCH, "random", "full", (DENSE, PEAKY8)),
    ("bench_ragged", 294, 32, 96, _L_BENCH, "random", "ragged", (DENSE, PEAKY8, SAT)),
    ("c4_ragged", 588, 32, 166, _L_C4, "random", "ragged", (DENSE, PEAKY8, PEAKY15, PEAKY4)),
    ("generic_long", 1200, 2, 166, [120, 64], "random", [1200, 1100], (DENSE, PEAKY8)),
    ("generic_L210", 700, 2, 96, [210, 5], "random", [700, 333], (DENSE, PEAKY8)),
    # act_len 0 (empty: nll 0; labelled: +inf), 1, 2 and around the prefetch depth, in one batch; T * B = 170 is not a multiple of 4
    ("act_edges", 17, 10, 63, [0, 2, 1, 0, 1, 3, 4, 4, 6, 5], "random", [0, 0, 1, 1, 2, 8, 9, 10, 16, 17], (DENSE, PEAKY8, SAT)),
    ("T1", 1, 5, 64, [0, 1, 1, 2, 0], "random", [1, 1, 1, 1, 0], (DENSE, PEAKY8)),
    ("B1", 50, 1, 65, [12], "random", "full", (DENSE, PEAKY8)),
    ("V2", 40, 3, 2, [5, 1, 0], "equal", [40, 17, 9], (DENSE, PEAKY8)),
    # more lines than one row split of the batch sum (vocr_colsum splits above 32 rows); T * B = 1470 is not a multiple of 4
    ("B70", 21, 70, 33, [(7 * i) % 9 for i in range(70)], "random", "ragged", (DENSE, PEAKY8)),
    # no label anywhere: CTCLoss passes a one-entry placeholder for the empty label array
    ("empty_all", 12, 5, 20, [0, 0, 0, 0, 0], "random", [12, 7, 1, 0, 3], (DENSE,)),
    ("V257", 33, 3, 257, [10, 3, 16], "random", "ragged", (DENSE, PEAKY8)),
    ("V4096", 7, 3, 4096, [3, 1, 0], "random", [7, 5, 2], (DENSE, PEAKY8)),
    # all-equal and a b a b labellings; the GPU file runs each batch through every kernel that admits it
    ("patterns64", 160, 6, 96, [20, 31, 31, 10, 25, 0], ["equal", "abab", "equal", "abab", "random", "random"], "ragged", (DENSE, PEAKY8)),
    ("patterns128", 200, 4, 96, [40, 63, 32, 33], ["equal", "abab", "abab", "random"], [200, 190, 90, 67], (DENSE, PEAKY8)),
    ("patterns_generic", 300, 3, 96, [70, 100, 65], ["equal", "abab", "random"], [300, 250, 131], (DENSE, PEAKY8)),
    # one feasible path (closed form) and that plus one frame
    ("tight64", 64, 6, 50, [5, 31, 12, 5, 31, 12], "random", "tight", (DENSE, SAT)),
    ("tight128", 130, 6, 50, [40, 63, 33, 40, 63, 33], "random", "tight", (DENSE,)),
    ("tight_generic", 150, 4, 50, [70, 64, 70, 64], "random", "tight", (DENSE,)),
    # an infeasible and an empty line beside feasible ones, in each of the three kernels
    ("mix64", 60, 4, 96, [31, 0, 10, 31], "random", [20, 33, 60, 59], (DENSE, PEAKY8)),
    ("mix128", 130, 4, 96, [63, 0, 40, 7], "random", [50, 130, 100, 9], (DENSE, PEAKY8)),
    ("mix_generic", 150, 4, 96, [70, 0, 70, 64], "random", [60, 77, 150, 149], (DENSE, PEAKY8)),
]
# where the mutants are judged (every mutant must miss a bar by >= 10x on at least one of these)
MUTANT_CASES = [("c4_ragged", PEAKY8), ("patterns64", PEAKY8), ("tight128", DENSE), ("act_edges", PEAKY8)]


def regime_name(regime):
    return regime[0] + "".join("_%g" % v for v in regime[1:])


def build_case(name, regime, seed=0):
    """(logits fp32 [T,B,V], labels int32 flat (at least one entry), label_lens list, act_lens list, per-line label lists)"""
    spec = [c for c in GPU_CASES if c[0] == name][0]
    _, T, B, V, ls, kinds, act, regimes = spec
    assert regime in regimes
    rng = np.random.default_rng([seed, GPU_CASES.index(spec), regimes.index(regime)])
    kinds = [kinds] * B if isinstance(kinds, str) else kinds
    labs = [make_labels(rng, V, ls[b], kinds[b]) for b in range(B)]
    needs = [need(l) for l in labs]
    if act == "full":
        act = [T] * B
    elif act == "ragged":
        act = _ragged(T, B, needs)
    elif act == "tight":
        act = [needs[b] + (1 if b >= B // 2 else 0) for b in range(B)]
    act = [int(v) for v in act]
    assert len(act) == B and max(act) <= T
    x = build_logits(rng, T, B, V, labs, act, regime)
    flat = torch.tensor([v for l in labs for v in l] or [0], dtype=torch.int32)
    return x, flat, [len(l) for l in labs], act, labs


def all_cases():
    for spec in GPU_CASES:
        for regime in spec[7]:
            yield spec[0], regime


def tight_closed_form(logits, lab, Tb):
    """the one path of a line with act_len == need(lab): (nll, grad [Tb,V]) = (-sum of lp along it, softmax - one-hot), fp64, without
    any recursion"""
    path = []
    for i, v in enumerate(lab):
        if i > 0 and lab[i - 1] == v:
            path.append(0)
        path.append(v)
    assert len(path) == Tb
    lp = torch.log_softmax(logits[:Tb].double(), 1)
    idx = torch.tensor(path, dtype=torch.long)
    g = torch.exp(lp)
    g[torch.arange(Tb), idx] -= 1.0
    return -lp[torch.arange(Tb), idx].sum(), g


def count_paths(lab, Tb):
    """the number of CTC paths of `lab` over Tb frames, by brute-force enumeration of the collapse rule on a small alphabet (exponential:
    small examples only)"""
    import itertools
    syms = sorted(set(lab) | {0})
    n = 0
    for p in itertools.product(syms, repeat=Tb):
        out, prev = [], None
        for v in p:
            if v != prev and v != 0:
                out.append(v)
            prev = v
        n += out == list(lab)
    return n
