"""An fp64 restatement of vocr_ctc_entropy (include/vocr.h): ln P, the alignment entropy H and the closed-form gradient of
w_ctc ln P + w_ent H with respect to the raw logits, with symbol classes.  numpy on the CPU, vectorised over the extended positions, one
loop over the frames.  Test helper only; it shares no code with the product.  Conventions are vocr_ctc_align's: blank 0, S = 2L+1, the
skip s-2 -> s iff position s is not blank and its CLASS differs from that of s-2, classes from `canon` (align_ref.classes_of).

A path assigns one CLASS to every frame; p(pi) = prod_t P_t(pi_t), P = sum p, N = sum p * (-ln p), H = N / P + ln P.
Forward pair (a, h) = ln sum p, ln sum p * (-ln p) over the partial paths that end in (t, s), frame t's emission included.
Backward pair (bx, gx) the same over the partial paths that START in a successor of s at frame t + 1: frame t's emission is NOT in
it, so for the paths through (t, s)
    sum p            = exp(a + bx)
    sum p * (-ln p)  = exp(h + bx) + exp(a + gx)                           every term has one sign: no subtraction anywhere
(the kernel combines two lattices that both include frame t and subtracts the emission once; this is the other way round on purpose).
    occ(t, c) = sum over the positions of class c of exp(a + bx) / P,     occN(t, c) = the same of (exp(h + bx) + exp(a + gx)) / P
    dlnP/du_t(c) = occ,    dH/du_t(c) = occN - (N / P) occ                (sums to 0 over c)
    grad[t][v] = share_t(v) * (w_ctc occ + w_ent (occN - (N / P) occ)) - y_t(v) * w_ctc,     share = y_t(v) / P_t(class(v))
Cells that no path reaches hold -inf and are left out of every sum (never an inf - inf)."""
import itertools

import numpy as np

from tests.align_ref import classes_of

NEG = -np.inf


def class_logprobs(x, cls):
    """(lp, clp) [T,V] fp64 of logits x [T,V]: the row log-softmax and at every column the log-probability of its class; a row of
    -inf stays -inf"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = x.max(1, keepdims=True)
        dead = ~np.isfinite(m)
        ms = np.where(dead, 0.0, m)
        lp = x - (ms + np.log(np.exp(x - ms).sum(1, keepdims=True)))
        lp = np.where(dead, NEG, lp)
        clp = lp.copy()
        for c in np.unique(cls):
            mem = np.nonzero(cls == c)[0]
            if len(mem) > 1:
                sub = lp[:, mem]
                mm = sub.max(1, keepdims=True)
                mz = np.where(np.isfinite(mm), mm, 0.0)
                v = mz + np.log(np.exp(sub - mz).sum(1, keepdims=True))
                clp[:, mem] = np.where(np.isfinite(mm), v, NEG)
    return lp, clp


def label_ok(lab, V, cls, max_label_len):
    return lab is not None and len(lab) <= max_label_len and all(0 < v < V and cls[v] != 0 for v in lab)


def _lse(*terms):
    out = terms[0]
    for t in terms[1:]:
        out = np.logaddexp(out, t)
    return out


def _shift(v, k):
    """v moved k places to the right (k > 0) or to the left, -inf moving in"""
    out = np.full_like(v, NEG)
    if k > 0:
        out[k:] = v[:-k]
    else:
        out[:k] = v[-k:]
    return out


def _ln_neg(u):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((u < 0) & np.isfinite(u), np.log(np.where(u < 0, -u, 1.0)), NEG)


def _exp(v):
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(v), np.exp(np.where(np.isfinite(v), v, 0.0)), 0.0)


def line(x, length, lab, cls, max_label_len=None, w_ctc=0.0, w_ent=0.0):
    """one line: logits x [T,V], `length` frames, labelling `lab` (list or None).  dict(lnp, H, ratio = N / P, grad [T,V], dH [T,V] =
    the gradient of H alone, dP [T,V] = that of ln P alone)"""
    x = np.asarray(x, dtype=np.float64)
    T, V = x.shape
    length = int(min(max(length, 0), T))
    M = T if max_label_len is None else max_label_len
    zero = np.zeros((T, V))
    out = dict(lnp=NEG, H=0.0, ratio=0.0, grad=zero, dH=zero.copy(), dP=zero.copy(), length=length)
    if not label_ok(lab, V, cls, M):
        return out
    if length == 0:
        if len(lab) == 0:
            out["lnp"] = 0.0
        return out
    L = len(lab)
    S = 2 * L + 1
    ext = np.zeros(S, dtype=np.int64)
    ext[1::2] = lab
    ec = np.asarray(cls)[ext]
    pos = np.arange(S)
    skip = (pos >= 2) & (ext != 0) & (ec != np.roll(ec, 2))               # into s from s - 2
    skip_out = _shift(skip.astype(np.float64), -2) > 0                     # out of s into s + 2
    lp, clp = class_logprobs(x[:length], cls)
    u = clp[:, ext]                                                       # [len, S]
    lnu = _ln_neg(u)
    ninf = np.full(S, NEG)
    a = np.full((length, S), NEG)
    h = np.full((length, S), NEG)
    a[0, :2] = u[0, :2]
    h[0, :2] = np.where(np.isfinite(u[0, :2]), u[0, :2] + lnu[0, :2], NEG)
    for t in range(1, length):
        A = _lse(a[t - 1], _shift(a[t - 1], 1), np.where(skip, _shift(a[t - 1], 2), ninf))
        Hp = _lse(h[t - 1], _shift(h[t - 1], 1), np.where(skip, _shift(h[t - 1], 2), ninf))
        live = np.isfinite(u[t]) & np.isfinite(A)
        a[t] = np.where(live, A + u[t], NEG)
        with np.errstate(invalid="ignore"):
            h[t] = np.where(live, u[t] + np.logaddexp(Hp, A + lnu[t]), NEG)
    ends = np.zeros(S, dtype=bool)
    ends[S - 1] = True
    if S > 1:
        ends[S - 2] = True
    lnp = _lse(*[a[length - 1, s] for s in np.nonzero(ends)[0]])
    lnn = _lse(*[h[length - 1, s] for s in np.nonzero(ends)[0]])
    if not np.isfinite(lnp):
        return out
    ratio = float(np.exp(lnn - lnp))
    out.update(lnp=float(lnp), ratio=ratio, H=max(ratio + float(lnp), 0.0))
    # the backward pair WITHOUT frame t's emission; b / g with it are the recursion's carriers
    bx = np.full((length, S), NEG)
    gx = np.full((length, S), NEG)
    bx[length - 1] = np.where(ends, 0.0, NEG)
    b = np.where(np.isfinite(u[length - 1]), bx[length - 1] + u[length - 1], NEG)
    g = np.where(np.isfinite(b), b + lnu[length - 1], NEG)
    for t in range(length - 2, -1, -1):
        bx[t] = _lse(b, _shift(b, -1), np.where(skip_out, _shift(b, -2), ninf))
        gx[t] = _lse(g, _shift(g, -1), np.where(skip_out, _shift(g, -2), ninf))
        live = np.isfinite(u[t]) & np.isfinite(bx[t])
        b = np.where(live, bx[t] + u[t], NEG)
        with np.errstate(invalid="ignore"):
            g = np.where(live, u[t] + np.logaddexp(gx[t], bx[t] + lnu[t]), NEG)
    reach = np.isfinite(a) & np.isfinite(bx)
    gam = np.where(reach, _exp(a + bx - lnp), 0.0)
    gamn = np.where(reach, _exp(h + bx - lnp) + _exp(a + gx - lnp), 0.0)
    occ = np.zeros((length, V))
    occn = np.zeros((length, V))
    for s in range(S):
        occ[:, ec[s]] += gam[:, s]
        occn[:, ec[s]] += gamn[:, s]
    cl = np.asarray(cls)
    y = _exp(lp)
    share = np.where(np.isfinite(lp), _exp(lp - np.where(np.isfinite(clp), clp, 0.0)), 0.0)
    dP = np.zeros((T, V))
    dH = np.zeros((T, V))
    dP[:length] = share * occ[:, cl] - y
    dH[:length] = share * (occn[:, cl] - ratio * occ[:, cl])
    out.update(dP=dP, dH=dH, grad=w_ctc * dP + w_ent * dH, occ=occ, occn=occn)
    return out


def entropy(logits, lens, labs, canon=None, coeff=None, max_label_len=None):
    """(lnp [B], H [B], grad [T,B,V]) fp64 of logits [T,B,V], labs[b] a label list or None, coeff [B,2] or None (zeros)"""
    x = np.asarray(logits, dtype=np.float64)
    T, B, V = x.shape
    cls = classes_of(V, None if canon is None else np.asarray(canon))
    co = np.zeros((B, 2)) if coeff is None else np.asarray(coeff, dtype=np.float64)
    lnp, H, grad = np.empty(B), np.empty(B), np.zeros((T, B, V))
    for b in range(B):
        r = line(x[:, b], lens[b], labs[b], cls, max_label_len, co[b, 0], co[b, 1])
        lnp[b], H[b], grad[:, b] = r["lnp"], r["H"], r["grad"]
    return lnp, H, grad


def brute_force(x, length, lab, cls):
    """(ln P, H) by enumerating every sequence of `length` CLASSES: a path counts iff it collapses (repeats merge, blanks drop) to the
    classes of `lab`.  (-inf, 0.0) without a path.  Small examples only."""
    x = np.asarray(x, dtype=np.float64)
    _, clp = class_logprobs(x[:length], cls)
    reps = sorted(set(int(c) for c in cls))
    want = [int(cls[v]) for v in lab]
    logs = []
    for frames in itertools.product(reps, repeat=length):
        col, prev = [], 0
        for k in frames:
            if k != 0 and k != prev:
                col.append(k)
            prev = k
        if col == want:
            s = sum(clp[t, k] for t, k in enumerate(frames)) if length else 0.0
            if np.isfinite(s):
                logs.append(s)
    if not logs:
        return NEG, 0.0
    logs = np.asarray(logs)
    top = logs.max()
    P = np.exp(logs - top).sum()
    q = np.exp(logs - top) / P
    lnp = top + np.log(P)
    return float(lnp), float(-(q * (logs - lnp)).sum())


def count_paths(length, lab, cls=None):
    """the number of frame paths of `length` frames that collapse to `lab`, as a Python integer (the lattice recursion over integers)"""
    L = len(lab)
    S = 2 * L + 1
    if length == 0:
        return 1 if L == 0 else 0
    ext = [0] * S
    ext[1::2] = list(lab)
    ec = [ext[s] if cls is None else int(cls[ext[s]]) for s in range(S)]
    row = [0] * S
    row[0] = 1
    if S > 1:
        row[1] = 1
    for _ in range(1, length):
        new = [0] * S
        for s in range(S):
            n = row[s] + (row[s - 1] if s >= 1 else 0)
            if s >= 2 and ext[s] != 0 and ec[s] != ec[s - 2]:
                n += row[s - 2]
            new[s] = n
        row = new
    return row[S - 1] + (row[S - 2] if S > 1 else 0)


def need(lab, cls=None):
    """the fewest frames `lab` fits: its labels plus one blank between neighbours of one class"""
    c = [v if cls is None else int(cls[v]) for v in lab]
    return len(c) + sum(1 for i in range(1, len(c)) if c[i] == c[i - 1])
