"""fp64 numpy restatement of vocr_ctc_edit_scores (vistaocr_amd/csrc/ctc_edit.hip): the CTC forward score of every labelling one
substitution, deletion or insertion away from a hypothesis, from the forward and backward lattices of the hypothesis.  Test helper only;
shares no code with the product.  tests/test_edit_cpu.py holds it to the independent definition, tests.align_ref.align(...).ctc of each
edited labelling.

alpha[t][s], beta[t][s] over the extended sequence (blank 0, S = 2L+1), beta including the emission at t.  For every slot p = 0..L and
every column c at once (arrays [L+1, V]), x is the state of the substituted / inserted class, y the blank behind an inserted one:
    x(0) = lp(0,c) if p = 0 else -inf;  x(t) = lp(t,c) + lse(x(t-1), alpha[t-1][2p], alpha[t-1][2p-1] if p > 0 and c != l(p-1))
    y(0) = -inf;                        y(t) = lp(t,0) + lse(y(t-1), x(t-1))
and every score is a logsumexp over the LAST frame t a path spends in the new state(s), times what follows in beta."""
import numpy as np

from tests import align_ref as ar

NEG = -np.inf


def _lattice(clp, ext, cls):
    """Forward lattice [len, S] of the extended sequence `ext` over the class log-probabilities clp [len, V]."""
    n, S = clp.shape[0], len(ext)
    ext = np.asarray(ext)
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != 0) & (cls[ext[2:]] != cls[ext[:-2]])
    a = np.full((n, S), NEG)
    a[0, 0] = clp[0, 0]
    if S > 1:
        a[0, 1] = clp[0, ext[1]]
    for t in range(1, n):
        prev = a[t - 1]
        tot = prev.copy()
        tot[1:] = np.logaddexp(tot[1:], prev[:-1])
        two = np.full(S, NEG)
        two[2:] = prev[:-2]
        tot = np.logaddexp(tot, np.where(skip, two, NEG))
        a[t] = tot + clp[t, ext]
    return a


class EditScores(object):
    __slots__ = ("ctc", "sub", "dele", "ins")

    def __init__(self, ctc, sub, dele, ins):
        self.ctc, self.sub, self.dele, self.ins = ctc, sub, dele, ins


def edit_scores(logits, length, labels, canon=None):
    """ctc (float), sub [L, V], dele [L], ins [L+1, V] for the first `length` frames of logits [T, V]."""
    x = np.asarray(logits, dtype=np.float64)
    T, V = x.shape
    n = int(min(max(length, 0), T))
    labels = [int(v) for v in labels]
    L = len(labels)
    out = EditScores(NEG, np.full((L, V), NEG), np.full(L, NEG), np.full((L + 1, V), NEG))
    cls = ar.classes_of(V, canon)
    if any(v <= 0 or v >= V or cls[v] == 0 for v in labels):
        return out
    if n == 0:                                       # no frames: only the empty labelling has a score
        out.ctc = 0.0 if L == 0 else NEG
        if L == 1:
            out.dele[0] = 0.0
        return out
    with np.errstate(invalid="ignore", divide="ignore"):
        clp, _ = ar.class_logprobs(x[:n], canon)
        S = 2 * L + 1
        ext = [labels[s >> 1] if s & 1 else 0 for s in range(S)]
        alpha = _lattice(clp, ext, cls)
        beta = _lattice(clp[::-1], ext[::-1], cls)[::-1, ::-1]
        out.ctc = float(np.logaddexp(alpha[n - 1, S - 1], alpha[n - 1, S - 2] if S > 1 else NEG))
        lc = cls[np.array(labels, dtype=np.int64)] if L else np.zeros(0, dtype=np.int64)
        slots = np.arange(L + 1)
        cc = cls[None, :]                                                          # [1, V]
        prev_c = np.concatenate([[-1], lc])[:, None]                               # class of l(p-1), [L+1, 1]
        this_c = np.concatenate([lc, [-1]])[:, None]                               # class of l(p)
        next_c = np.concatenate([lc, [-1, -1]])[1:L + 2, None]                     # class of l(p+1)
        skip_a = (slots[:, None] > 0) & (cc != prev_c)
        skip_b = (slots[:, None] < L - 1) & (cc != next_c)
        ins_x = (slots[:, None] < L) & (cc != this_c)
        skip_d = (slots > 0) & (slots < L - 1) & (prev_c[:, 0] != next_c[:, 0])
        a0 = alpha[:, 2 * slots]                                                   # [n, L+1]
        a1 = np.full((n, L + 1), NEG)
        a1[:, 1:] = alpha[:, 2 * slots[1:] - 1]

        def beta_at(off):                                                          # beta[t][2p + off], -inf beyond the lattice; [n, L+1]
            b = np.full((n, L + 1), NEG)
            ok = 2 * slots + off < S
            b[:, ok] = beta[:, 2 * slots[ok] + off]
            return b

        b1, b2, b3 = beta_at(1), beta_at(2), beta_at(3)
        xs = np.full((n, L + 1, V), NEG)
        ys = np.full((n, L + 1, V), NEG)
        xs[0, 0] = clp[0]
        for t in range(1, n):
            enter = np.logaddexp(a0[t - 1][:, None], np.where(skip_a, a1[t - 1][:, None], NEG))
            xs[t] = clp[t][None, :] + np.logaddexp(xs[t - 1], enter)
            ys[t] = clp[t, 0] + np.logaddexp(ys[t - 1], xs[t - 1])
        # what follows a substituted x (or a label p-1 whose successor was deleted) at frame t: [n, L+1, V] and [n, L+1]
        e_sub = np.full((n, L + 1, V), NEG)
        e_del = np.full((n, L + 1), NEG)
        if n > 1:
            e_sub[:-1] = np.logaddexp(b2[1:][:, :, None], np.where(skip_b[None], b3[1:][:, :, None], NEG))
            e_del[:-1] = np.logaddexp(b2[1:], np.where(skip_d[None], b3[1:], NEG))
        if L > 0:
            e_sub[n - 1, L - 1] = 0.0
            e_del[n - 1, L - 1] = 0.0
        sub = np.logaddexp.reduce(xs + e_sub, axis=0)                              # [L+1, V]
        dele = np.logaddexp.reduce(a1 + e_del, axis=0)                             # [L+1]
        if L > 0:
            dele[0] = np.logaddexp(beta[0, 2], beta[0, 3] if L > 1 else NEG)
        ins = np.full((L + 1, V), NEG)
        if n > 1:
            nxt = b1[1:][:, :, None]
            ins = np.logaddexp.reduce(np.logaddexp(np.where(ins_x[None], xs[:-1] + nxt, NEG), ys[:-1] + nxt), axis=0)
        ins[L] = np.logaddexp(xs[n - 1, L], ys[n - 1, L])
    no_edit = (np.arange(V) == 0) | (cls == 0)
    sub[:, no_edit] = NEG
    ins[:, no_edit] = NEG
    out.sub, out.dele, out.ins = sub[:L], dele[:L], ins
    return out


def edited(labels, kind, p, c=None):
    labels = list(labels)
    if kind == "sub":
        return labels[:p] + [c] + labels[p + 1:]
    if kind == "del":
        return labels[:p] + labels[p + 1:]
    return labels[:p] + [c] + labels[p:]


def direct_scores(logits, length, labels, canon=None):
    """The independent definition: align_ref's forward score of every edited labelling, one by one.  Small cases only."""
    x = np.asarray(logits, dtype=np.float64)
    V = x.shape[1]
    L = len(labels)
    out = EditScores(ar.align(x, length, labels, canon).ctc, np.full((L, V), NEG), np.full(L, NEG), np.full((L + 1, V), NEG))
    cls = ar.classes_of(V, canon)
    if any(v <= 0 or v >= V or cls[v] == 0 for v in labels):
        return out
    for p in range(L):
        out.dele[p] = ar.align(x, length, edited(labels, "del", p), canon).ctc
        for c in range(V):
            out.sub[p, c] = ar.align(x, length, edited(labels, "sub", p, c), canon).ctc
    for q in range(L + 1):
        for c in range(V):
            out.ins[q, c] = ar.align(x, length, edited(labels, "ins", q, c), canon).ctc
    return out


def posteriors(scores, labels, canon, V):
    """fp64 posteriors from raw scores (of the reference or of the kernel) for one labelling: per position p the softmax over
    {each canonical class (the label's own class = keep), delete}, per gap q over {keep, insert each canonical class}.  Returns
    (char [L, V+1] with column V = delete, gap [L+1, V+1] with column V = nothing missing); columns that are no canonical class -inf -> 0."""
    cls = ar.classes_of(V, canon)
    canonical = (cls == np.arange(V)) & (np.arange(V) > 0)
    L = len(labels)
    with np.errstate(invalid="ignore", divide="ignore"):
        ch = np.full((L, V + 1), NEG)
        ch[:, :V] = np.where(canonical[None], np.asarray(scores.sub, dtype=np.float64)[:L], NEG)
        ch[:, V] = np.asarray(scores.dele, dtype=np.float64)[:L]
        gp = np.full((L + 1, V + 1), NEG)
        gp[:, :V] = np.where(canonical[None], np.asarray(scores.ins, dtype=np.float64)[:L + 1], NEG)
        gp[:, V] = float(scores.ctc)
        out = []
        for a in (ch, gp):
            m = np.max(a, axis=1, keepdims=True) if a.shape[0] else np.zeros((0, 1))
            z = np.exp(a - np.where(m == NEG, 0.0, m))
            tot = np.sum(z, axis=1, keepdims=True)
            out.append(np.where(tot > 0, z / np.where(tot > 0, tot, 1.0), 0.0))
    return out[0], out[1]
