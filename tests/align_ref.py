"""fp64 numpy restatement of vocr_ctc_align (vistaocr_amd/csrc/ctc_align.hip) and a brute force over all frame labellings.  Test helper
only; shares no code with the product.

align(): the Viterbi and the forward recursion over the extended sequence (blank 0, S = 2L+1, skip s-2 -> s iff ext[s] is not blank
and its class differs from ext[s-2]'s), the kernel's tie rule (among equal predecessors prefer s, then s-1, then s-2; at the last frame
the final blank over the last label), the spans of the backtrace and the label scores.  It also returns the line's DECISION GAP: the
smallest margin between the chosen and the runner-up predecessor over the cells ON THE BEST PATH, and between the two end states.  If
every fp32 cell value is within eps of the fp64 one, a gap above 2 eps forces the same back pointers along the path, hence the same
spans."""
import itertools

import numpy as np

NEG = -np.inf


def _lse(vals):
    vals = np.asarray(vals, dtype=np.float64)
    m = np.max(vals)
    if m == NEG:
        return NEG
    return float(m + np.log(np.sum(np.exp(vals - m))))


def classes_of(V, canon=None):
    """The sanitised class of every column (the beam searches' rule: an entry that is not a canonical index <= v stands for itself)."""
    cls = np.arange(V)
    if canon is not None:
        canon = np.asarray(canon)
        for v in range(V):
            c = int(canon[v])
            if c < 0 or c > v or int(canon[c]) != c:
                c = v
            cls[v] = c
    return cls


def class_logprobs(logits, canon=None):
    """[T, V] fp64: at every column the log-probability of its class (logsumexp of the members of the row's log-softmax).  A row of -inf
    stays -inf."""
    x = np.asarray(logits, dtype=np.float64)
    T, V = x.shape
    cls = classes_of(V, canon)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.max(x, axis=1, keepdims=True) if T else np.zeros((0, 1))
        dead = m[:, 0] == NEG
        out = x - (m + np.log(np.sum(np.exp(x - np.where(m == NEG, 0.0, m)), axis=1, keepdims=True)))
    out[dead] = NEG
    lp = out.copy()
    for c in np.unique(cls):
        members = np.nonzero(cls == c)[0]
        if len(members) > 1:
            for t in range(T):
                out[t, members] = _lse(lp[t, members])
    return out, cls


def greedy_labels(logits, length):
    """The plain argmax collapse of a line [T, V]: a blank resets, repeats collapse; no threshold, no class merging."""
    idx = np.argmax(np.asarray(logits)[:length], axis=1)
    out, prev = [], 0
    for k in idx:
        k = int(k)
        if k != 0 and k != prev:
            out.append(k)
        prev = k
    return out


class Alignment(object):
    __slots__ = ("viterbi", "ctc", "spans", "label_scores", "gap", "path")

    def __init__(self, viterbi, ctc, spans, label_scores, gap, path):
        self.viterbi, self.ctc, self.spans, self.label_scores, self.gap, self.path = viterbi, ctc, spans, label_scores, gap, path


def _none():
    return Alignment(NEG, NEG, None, None, np.inf, None)


def align(logits, length, labels, canon=None):
    """The alignment of `labels` to the first `length` frames of logits [T, V].  spans / label_scores are [L, 2] arrays (None without an
    alignment), path the extended position of every frame."""
    x = np.asarray(logits, dtype=np.float64)
    T, V = x.shape
    length = int(min(max(length, 0), T))
    labels = [int(v) for v in labels]
    L = len(labels)
    clp, cls = class_logprobs(x[:length], canon) if length > 0 else (np.zeros((0, V)), classes_of(V, canon))
    if any(v <= 0 or v >= V or cls[v] == 0 for v in labels):
        return _none()
    if length == 0:
        return Alignment(0.0, 0.0, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 2)), np.inf, []) if L == 0 else _none()
    S = 2 * L + 1
    ext = [labels[s >> 1] if s & 1 else 0 for s in range(S)]
    skip = [s >= 2 and ext[s] != 0 and cls[ext[s]] != cls[ext[s - 2]] for s in range(S)]
    vm = np.full(S, NEG)
    vs = np.full(S, NEG)
    vm[0] = vs[0] = clp[0, 0]
    if S > 1:
        vm[1] = vs[1] = clp[0, ext[1]]
    back = np.zeros((length, S), dtype=np.int64)
    margin = np.full((length, S), np.inf)
    skip = np.array(skip, dtype=bool)
    ext_a = np.array(ext)

    def preds(v):                                   # [3, S]: the values at s, s-1, s-2 (where the skip is allowed) of the previous frame
        c = np.full((3, S), NEG)
        c[0] = v
        c[1, 1:] = v[:-1]
        c[2, 2:] = v[:-2]
        c[2, ~skip] = NEG
        return c

    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(1, length):
            cand = preds(vm)
            frm = np.zeros(S, dtype=np.int64)
            best = cand[0].copy()
            for k in (1, 2):                        # a predecessor replaces the choice only when strictly greater
                better = cand[k] > best
                frm[better] = k
                best[better] = cand[k][better]
            second = np.sort(cand, axis=0)[1]       # the runner-up of three is their median
            back[t] = frm
            margin[t] = np.where(second == NEG, np.inf, best - second)
            lp = clp[t, ext_a]
            vm = np.where(best == NEG, NEG, best + lp)
            cs = preds(vs)
            m = np.max(cs, axis=0)
            tot = np.where(m == NEG, NEG, m + np.log(np.sum(np.exp(cs - np.where(m == NEG, 0.0, m)), axis=0)))
            vs = np.where(tot == NEG, NEG, tot + lp)
    a, c = vm[S - 1], (vm[S - 2] if S > 1 else NEG)
    s = S - 2 if c > a else S - 1
    vit = max(a, c)
    if vit == NEG:
        return _none()
    ctc = _lse([vs[S - 1], vs[S - 2] if S > 1 else NEG])
    gap = np.inf if min(a, c) == NEG else abs(a - c)
    path = [0] * length
    for t in range(length - 1, -1, -1):
        path[t] = s
        if t > 0:
            gap = min(gap, margin[t, s])
            s -= back[t, s]
    spans = np.full((L, 2), -1, dtype=np.int64)
    for t, s in enumerate(path):
        if s & 1:
            p = s >> 1
            if spans[p, 0] < 0:
                spans[p, 0] = t
            spans[p, 1] = t
    lsc = np.zeros((L, 2))
    for p in range(L):
        seg = clp[spans[p, 0]:spans[p, 1] + 1, labels[p]]
        lsc[p] = (np.max(seg), np.sum(seg))
    return Alignment(float(vit), float(ctc), spans, lsc, float(gap), path)


def path_from_spans(spans, length, L):
    """The frame path (extended positions) that the spans describe, or None if they are not a CTC path of a labelling of length L over
    `length` frames: every label has a span inside the line, spans are in order and disjoint.  Frames outside every span are blanks; a
    blank between equal neighbours is checked by path_is_valid."""
    path = [None] * length
    prev_last = -1
    for p in range(L):
        first, last = int(spans[p][0]), int(spans[p][1])
        if first <= prev_last or last < first or last >= length:
            return None
        for t in range(first, last + 1):
            path[t] = 2 * p + 1
        prev_last = last
    nxt = 0           # blanks: the even position between the neighbouring labels
    for t in range(length):
        if path[t] is None:
            path[t] = nxt
        else:
            nxt = path[t] + 1
    return path


def path_is_valid(path, labels, cls):
    """Monotone, starts in {0, 1}, ends in {2L-1, 2L}, steps of 0 / 1, or 2 onto a label whose class differs from the one two back."""
    L = len(labels)
    S = 2 * L + 1
    if not path:
        return L == 0
    if path[0] not in (0, 1) or path[-1] not in (S - 1, S - 2) or min(path) < 0:
        return False
    for a, b in zip(path[:-1], path[1:]):
        d = b - a
        if d not in (0, 1, 2):
            return False
        if d == 2 and not (b & 1 and cls[labels[b >> 1]] != cls[labels[(b >> 1) - 1]]):
            return False
    return True


def path_score(clp, labels, path):
    return float(sum(clp[t, labels[s >> 1] if s & 1 else 0] for t, s in enumerate(path)))


def brute_force(logits, labels, canon=None):
    """All (number of classes)^T frame labellings of logits [T, V]; those that collapse (repeats merge, blanks drop) to the class sequence
    of `labels`.  Returns (best path score, its spans [L, 2], logsumexp over all of them, the margin between the best and the second
    best path), or (-inf, None, -inf, inf) when there is none.  Only classes with a finite log-probability somewhere are enumerated."""
    x = np.asarray(logits, dtype=np.float64)
    T, V = x.shape
    clp, cls = class_logprobs(x, canon)
    labels = [int(v) for v in labels]
    want = [int(cls[v]) for v in labels]
    alive = [int(c) for c in np.unique(cls) if np.any(clp[:, c] > NEG)]
    if 0 not in alive:
        alive = [0] + alive
    scores, best, best_path = [], NEG, None
    for frames in itertools.product(alive, repeat=T):
        col, prev = [], 0
        for k in frames:
            if k != 0 and k != prev:
                col.append(k)
            prev = k
        if col != want:
            continue
        sc = float(sum(clp[t, k] for t, k in enumerate(frames)))
        if sc == NEG:
            continue
        scores.append(sc)
        if sc > best:
            best, best_path = sc, frames
    if best_path is None:
        return NEG, None, NEG, np.inf
    spans = np.full((len(labels), 2), -1, dtype=np.int64)
    p, prev = -1, 0
    for t, k in enumerate(best_path):
        if k != 0:
            if k != prev:
                p += 1
                spans[p, 0] = t
            spans[p, 1] = t
        prev = k
    srt = sorted(scores, reverse=True)
    margin = srt[0] - srt[1] if len(srt) > 1 else np.inf
    return best, spans, _lse(scores), margin
