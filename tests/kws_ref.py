"""fp64 numpy restatement of vocr_ctc_keyword_scores (vistaocr_amd/csrc/ctc_keyword.hip) and a brute force over all frame labellings.
Test helper only; shares no code with the product.

search(): both recursions over the extended sequence k_1, blank, k_2, .., blank, k_L (S = 2L-1, no outer blank; the skip s-2 -> s iff
position s is a label whose class differs from that of s-2), batched over (line, query):
    entry(t) = 0 if t = 0 else notc_(t-1)(k_1)       ANCHOR_START: sum of ln p_u(blank) over u < t
    exit(t)  = 0 if t = len-1 else notc_(t+1)(k_L)   ANCHOR_END:   sum of ln p_u(blank) over u > t
    a_t(0)   = lp_t(k_1) + lse(a_(t-1)(0), entry(t));  a_t(s) = lp_t(ext_s) + lse(a_(t-1)(s), a_(t-1)(s-1), a_(t-1)(s-2) if allowed)
    ln E     = lse over t of a_t(S-1) + exit(t)
and the same with max, the kernel's tie rule (among equal candidates prefer s, then s-1, then s-2, then the fresh entry, which only
position 0 has; among equal end frames the earliest), every cell carrying the start frame of its best path.  It also returns the
DECISION GAP of the best occurrence: the smallest margin between the chosen and the runner-up candidate over the cells ON THE BEST PATH
(carried forward with the cell like the start frame), and between the best and the runner-up end frame.  If every fp32 cell value is
within eps of the fp64 one, a gap above 2 eps forces the same choices along the path and the same end frame, hence the same span.

notc is the log of the SUM of the other classes' probabilities (a logsumexp over their columns minus the row's), never 1 - p."""
import itertools

import numpy as np

NEG = -np.inf
ANCHOR_START, ANCHOR_END, TRIM_START, TRIM_END = 1, 2, 4, 8


def classes_of(V, canon=None):
    cls = np.arange(V)
    if canon is not None:
        canon = np.asarray(canon)
        for v in range(V):
            c = int(canon[v])
            if c < 0 or c > v or int(canon[c]) != c:
                c = v
            cls[v] = c
    return cls


def _lse_axis(a, axis):
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.max(a, axis=axis, keepdims=True)
        safe = np.where(np.isfinite(m), m, 0.0)
        out = safe + np.log(np.sum(np.exp(a - safe), axis=axis, keepdims=True))
    return np.squeeze(np.where(m == NEG, NEG, out), axis=axis)


def frame_logprobs(logits, canon=None, want=()):
    """logits [..., V] -> (clp [..., V]: at every column ln P(its class); notc {class: [...]}: ln of the summed probability of every
    OTHER class, for the classes of `want`; cls).  A row of -inf gives -inf everywhere."""
    x = np.asarray(logits, dtype=np.float64)
    V = x.shape[-1]
    cls = classes_of(V, canon)
    row = _lse_axis(x, -1)
    with np.errstate(invalid="ignore"):
        lp = np.where(row[..., None] == NEG, NEG, x - np.where(row == NEG, 0.0, row)[..., None])
    clp = lp.copy()
    for c in np.unique(cls):
        members = np.nonzero(cls == c)[0]
        if len(members) > 1:
            clp[..., members] = _lse_axis(lp[..., members], -1)[..., None]
    notc = {}
    for c in set(int(cls[v]) for v in want):
        others = np.nonzero(cls != c)[0]
        with np.errstate(invalid="ignore"):
            notc[c] = np.where(row == NEG, NEG, _lse_axis(x[..., others], -1) - np.where(row == NEG, 0.0, row))
    return clp, notc, cls


def query_ok(q, V, cls, max_len=None, flags=0):
    trims = (1 if flags & TRIM_START else 0) + (1 if flags & TRIM_END else 0)
    return 1 + trims <= len(q) and (max_len is None or len(q) <= max_len) and all(0 < v < V and cls[v] != 0 for v in q)


def search(logits, lens, queries, flags=None, canon=None):
    """logits [T, B, V], lens [B], queries a list of Q label lists, flags a list of Q ints (None: 0).  Returns a dict of [B, Q] arrays:
    log_count, best, span [B, Q, 2], gap."""
    x = np.asarray(logits, dtype=np.float64)
    T, B, V = x.shape
    Q = len(queries)
    flags = [0] * Q if flags is None else [int(f) for f in flags]
    lens = np.clip(np.asarray(lens, dtype=np.int64), 0, T)
    cls0 = classes_of(V, canon)
    ok = np.array([query_ok(q, V, cls0, None, f) for q, f in zip(queries, flags)])
    qs = [list(q) if o else [1] for q, o in zip(queries, ok)]
    flags = [f if o else 0 for f, o in zip(flags, ok)]
    clp, notc, cls = frame_logprobs(x, canon, want=[q[0] for q in qs] + [q[-1] for q in qs])
    Ls = np.array([len(q) for q in qs])
    Ss = 2 * Ls - 1
    SM = int(Ss.max())
    ext = np.zeros((Q, SM), dtype=np.int64)
    inside = np.zeros((Q, SM), dtype=bool)
    skip = np.zeros((Q, SM), dtype=bool)
    restart = np.zeros((Q, SM), dtype=bool)                                      # TRIM_START: the span starts where the path reaches k_2
    mark = np.zeros((Q, SM), dtype=bool)                                         # TRIM_END: ... and ends with the last frame on k_(L-1)
    for i, q in enumerate(qs):
        if flags[i] & TRIM_START:
            restart[i, 2] = True
        if flags[i] & TRIM_END:
            mark[i, Ss[i] - 3] = True
        for s in range(Ss[i]):
            inside[i, s] = True
            if s % 2 == 0:
                ext[i, s] = q[s // 2]
                skip[i, s] = s >= 2 and cls[q[s // 2]] != cls[q[s // 2 - 1]]
    # boundary terms [T, B, Q]
    blank = clp[:, :, 0]
    tt = np.arange(T)[:, None]
    live = tt < lens[None, :]                                                    # [T, B]
    with np.errstate(invalid="ignore"):
        bl = np.where(live, blank, 0.0)
        pre = np.concatenate([np.zeros((1, B)), np.cumsum(bl, axis=0)[:-1]], axis=0)          # sum over u < t
        suf = np.concatenate([np.cumsum(bl[::-1], axis=0)[::-1][1:], np.zeros((1, B))], axis=0)   # sum over u > t (frames >= len add 0)
    EN = np.zeros((T, B, Q))
    EX = np.zeros((T, B, Q))
    last = (tt == lens[None, :] - 1)
    for i, q in enumerate(qs):
        n1, nL = notc[int(cls[q[0]])], notc[int(cls[q[-1]])]
        if flags[i] & ANCHOR_START:
            EN[:, :, i] = pre
        else:
            EN[1:, :, i] = n1[:-1]
        if flags[i] & ANCHOR_END:
            EX[:, :, i] = suf
        else:
            EX[:-1, :, i] = nL[1:]
            EX[:, :, i] = np.where(last, 0.0, EX[:, :, i])
    a = np.full((B, Q, SM), NEG)
    m = np.full((B, Q, SM), NEG)
    ms = np.full((B, Q, SM), -1, dtype=np.int64)
    me = np.full((B, Q, SM), -1, dtype=np.int64)
    mg = np.full((B, Q, SM), np.inf)                                             # the smallest margin along the cell's best path
    acc = np.full((B, Q), NEG)
    fin_all = np.full((T, B, Q), NEG)
    fin_start = np.full((T, B, Q), -1, dtype=np.int64)
    fin_end = np.full((T, B, Q), -1, dtype=np.int64)
    fin_gap = np.full((T, B, Q), np.inf)
    qi = np.arange(Q)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T):
            if not live[t].any():
                break
            lpe = clp[t][:, ext]                                                 # [B, Q, SM]

            def shifted(v, fill, k):
                out = np.full_like(v, fill)
                out[:, :, k:] = v[:, :, :-k] if k < SM else out[:, :, k:]
                return out

            a1, a2 = shifted(a, NEG, 1), np.where(skip[None], shifted(a, NEG, 2), NEG)
            m1, m2 = shifted(m, NEG, 1), np.where(skip[None], shifted(m, NEG, 2), NEG)
            s1, s2 = shifted(ms, -1, 1), shifted(ms, -1, 2)
            g1, g2 = shifted(mg, np.inf, 1), shifted(mg, np.inf, 2)
            e1, e2 = shifted(me, -1, 1), shifted(me, -1, 2)
            a1[:, :, 0], m1[:, :, 0], s1[:, :, 0], g1[:, :, 0] = EN[t], EN[t], t, np.inf      # the fresh entry: position 0's s-1 slot
            best, bs, bg, be = m.copy(), ms.copy(), mg.copy(), me.copy()
            for cm, cs, cg, ce in ((m1, s1, g1, e1), (m2, s2, g2, e2)):          # replaces the choice only when strictly greater
                better = cm > best
                best, bg, be = np.where(better, cm, best), np.where(better, cg, bg), np.where(better, ce, be)
                bs = np.where(better, np.where(restart[None], t, cs), bs)
            be = np.where(mark[None], t, be)
            second = np.sort(np.stack([m, m1, m2]), axis=0)[1]
            margin = np.where(second == NEG, np.inf, best - second)
            a = np.where(inside[None], np.logaddexp(np.logaddexp(a, a1), a2) + lpe, NEG)
            m = np.where(inside[None] & (best > NEG), best + lpe, NEG)
            ms, me, mg = bs, be, np.minimum(bg, margin)
            on = live[t][:, None]
            fa, fm = a[:, qi, Ss - 1] + EX[t], m[:, qi, Ss - 1] + EX[t]
            acc = np.where(on, np.logaddexp(acc, fa), acc)
            fin_all[t] = np.where(on, fm, NEG)
            fin_start[t] = ms[:, qi, Ss - 1]
            fin_end[t] = me[:, qi, Ss - 1]
            fin_gap[t] = mg[:, qi, Ss - 1]
    fin_all = np.where(np.isnan(fin_all), NEG, fin_all)
    e = np.argmax(fin_all, axis=0)                                               # the first maximum: the earliest end frame
    bi, qj = np.meshgrid(np.arange(B), qi, indexing="ij")
    best = fin_all[e, bi, qj]
    srt = np.sort(fin_all, axis=0)
    with np.errstate(invalid="ignore"):
        end_gap = np.where(srt[-2] == NEG, np.inf, best - srt[-2]) if T > 1 else np.full((B, Q), np.inf)
    gap = np.minimum(fin_gap[e, bi, qj], end_gap)
    trim_end = np.array([bool(f & TRIM_END) for f in flags])
    span = np.stack([fin_start[e, bi, qj], np.where(trim_end[None, :], fin_end[e, bi, qj], e)], axis=-1)
    dead = (best == NEG) | ~ok[None, :]
    acc = np.where(np.isnan(acc) | dead, NEG, acc)
    best = np.where(dead, NEG, best)
    span[dead] = -1
    gap = np.where(dead, np.inf, gap)
    return {"log_count": acc, "best": best, "span": span, "gap": gap}


def collapse(frames):
    """The characters of a frame path of class indices: (class, first frame, last frame) of every maximal run of one non-blank class."""
    chars, prev = [], 0
    for t, k in enumerate(frames):
        if k != 0 and k == prev:
            chars[-1][2] = t
        elif k != 0:
            chars.append([k, t, t])
        prev = k
    return chars


def brute_force(logits, query, flags=0, canon=None, whole_word=None):
    """All frame paths of logits [T, V] over the classes.  Returns (ln of the expected number of occurrences of `query` as a contiguous
    substring of the collapsed labelling, the best occurrence's score, its span, the margin to the best score of any other span):
    the score of an occurrence of span [s, e] with the frame labels pi_s .. pi_e is entry(s) + sum of lp_t(pi_t) + exit(e), the frames
    outside the span summed out; the margin is taken over all (span, frame labels) pairs.  Ties: the earliest end frame, then the
    earliest start.  TRIM_START / TRIM_END change the reported span only.  whole_word = the space's class: only occurrences
    bounded on both sides by that class or by the labelling's ends count (flags must be 0), and only the count is returned."""
    x = np.asarray(logits, dtype=np.float64)
    T, V = x.shape
    clp, _, cls = frame_logprobs(x, canon)
    if not query_ok(query, V, cls, None, flags):
        return NEG, NEG, (-1, -1), np.inf
    want = [int(cls[v]) for v in query]
    L = len(want)
    alive = sorted(set(int(c) for c in np.unique(cls)))
    total = []
    spans = {}
    P = np.exp(clp)
    for frames in itertools.product(alive, repeat=T):
        w = float(np.prod([P[t, k] for t, k in enumerate(frames)]))
        if w == 0.0:
            continue
        chars = collapse(frames)
        ks = [c[0] for c in chars]
        for i in range(len(chars) - L + 1):
            if ks[i:i + L] != want:
                continue
            if whole_word is not None:
                if (i > 0 and ks[i - 1] != whole_word) or (i + L < len(ks) and ks[i + L] != whole_word):
                    continue
            else:
                if (flags & ANCHOR_START) and i != 0:
                    continue
                if (flags & ANCHOR_END) and i + L != len(chars):
                    continue
            total.append(w)
            s, e = chars[i][1], chars[i + L - 1][2]
            key = (s, e, chars[min(i + 1, i + L - 1)][1] if flags & TRIM_START else s,
                   chars[max(i + L - 2, i)][2] if flags & TRIM_END else e) + tuple(frames[s:e + 1])
            spans[key] = spans.get(key, 0.0) + w                # the outside summed out: the same number as entry + sum + exit
    if not total:
        return NEG, NEG, (-1, -1), np.inf
    count = float(np.log(np.sum(total)))
    if whole_word is not None:
        return count
    by_span = {}
    for key, w in spans.items():
        if w > by_span.get(key[:2], (0.0, None))[0]:
            by_span[key[:2]] = (w, key[2:4])
    order = sorted(((k, w, rep) for k, (w, rep) in by_span.items()), key=lambda kv: (-kv[1], kv[0][1], kv[0][0]))
    best_w, best_span = order[0][1], order[0][2]             # the span as reported: without the trimmed labels' frames
    margin = np.inf if len(spans) == 1 else float(np.log(best_w) - np.log(sorted(spans.values())[-2]))
    return count, float(np.log(best_w)), best_span, margin
