"""CPU restatement of vocr_ctc_beam_search (vistaocr_amd/csrc/ctc_beam.hip) in fp64 numpy, vectorised over the candidates of a frame,
and the brute-force scorer it is checked against.  Test helper only: the product never imports it.

The restatement follows the kernel's rules exactly: symbol classes by canonical index (log-probability = logsumexp of the members),
stay / extend candidates, merging of an extension into the beam that already holds its prefix (prefixes compared as tuples),
ranking by logsumexp(p_b, p_nb) + alpha * LM + beta * len under the total order (score desc, slot id k*V + c asc), optional pruning,
and + alpha * ln P(</s>) before the final ranking (ties: the rank at the last frame).  It also returns the smallest score gap at
any decision the search took (the K-th against the (K+1)-th candidate of every frame, and neighbouring ranks of the final n-best):
where that gap is large, an fp32 search must take the same decisions.  It tracks the node ids the kernel assigns (a new prefix at
frame t, rank q: t*K + q; a stay keeps its node) and can count, into a `stats` dict, the decisions that fell inside an exact tie,
the merges into a prefix that came back under a new node id, and the largest number of finite candidates of a frame."""
import itertools

import numpy as np

NEG = -np.inf


def lse(a, b):
    m = np.maximum(a, b)
    with np.errstate(invalid="ignore"):
        out = m + np.log(np.exp(a - m) + np.exp(b - m))
    return np.where(m == NEG, NEG, out)


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def classes(canon, V):
    """Sanitised canonical index of every column (the kernel's rule)."""
    if canon is None:
        return np.arange(V)
    canon = np.asarray(canon)
    out = np.arange(V)
    for v in range(V):
        c = int(canon[v])
        if 0 <= c <= v and int(canon[c]) == c:
            out[v] = c
    return out


def class_logprobs(logits, canon=None):
    """[T, V] log-probabilities of the symbol classes (-inf on the non-canonical columns)."""
    lsm = log_softmax(logits)
    V = lsm.shape[1]
    cls = classes(canon, V)
    out = np.full_like(lsm, NEG)
    for c in np.unique(cls):
        mem = lsm[:, cls == c]
        m = mem.max(axis=1, keepdims=True)
        with np.errstate(invalid="ignore"):
            v = (m + np.log(np.exp(mem - m).sum(axis=1, keepdims=True)))[:, 0]
        out[:, c] = np.where(m[:, 0] == NEG, NEG, v)
    return out


def tie_gap(values, v):
    """The distance from the tied value v to the nearest different one of `values`, on either side (inf: there is none)."""
    d = np.abs(values[values != v] - v)
    return float(d.min()) if d.size else np.inf


def beam_search(logits, length, K, nbest=1, canon=None, lm=None, alpha=0.0, beta=0.0, prune=None, exact_ties=False, stats=None):
    """One line: logits [T, V] raw.  lm: an object with logp [S,V], next [S,V], eos [S], start (CharNgramLM) or None.
    Returns (hyps, min_gap): hyps = [(labels, total, acoustic, lm)] best first (at most nbest), min_gap the smallest decision gap.

    exact_ties: a gap of exactly 0.0 (the K-th against the (K+1)-th candidate, or neighbouring final ranks) does not enter min_gap;
    the distance from the tied score to the nearest different candidate score on either side enters instead, and the total order
    (score desc, slot id asc) decides the tie as the kernel does.  This is sound ONLY for logits whose tied candidates come from
    bitwise-duplicated columns: such candidates go through identical operation sequences, so they are equal bit for bit in fp32 as
    they are in fp64, and their slot ids descend from parents that are themselves the same beam or such twins.  On any other input
    an fp64 tie says nothing about fp32, and the default (the tie counts as gap 0: the line is undecided) is the right one.

    stats: a dict that receives, for this line, kth_ties (frames whose cut fell inside an exact tie), final_ties (exact ties between
    neighbouring ranks of the final n-best), remerges (merges into a parent beam whose node id is not the one the child was created
    from: the parent prefix left the beam and came back) and max_live (the largest number of finite candidates in a frame)."""
    logits = np.asarray(logits, dtype=np.float64)
    T, V = logits.shape
    L = int(min(max(length, 0), T))
    lp = class_logprobs(logits[:L], canon) if L else np.zeros((0, V))
    xp = lp.copy()
    if L:
        xp[:, 0] = NEG
        if prune is not None:
            xp[xp < prune] = NEG
    use_lm = lm is not None and alpha != 0.0
    start = lm.start if lm is not None else 0
    pb, pnb, acc = np.array([0.0]), np.array([NEG]), np.array([0.0])
    last, ln, lms = np.array([-1]), np.array([0]), np.array([start])
    pref = [()]
    node, pnode = np.array([-1]), np.array([-1])            # the kernel's pool node of each beam, and that node's parent
    kth_ties = final_ties = remerges = max_live = 0
    min_gap = np.inf
    cols = np.arange(V)
    for t in range(L):
        nb = len(pref)
        where = {p: k for k, p in enumerate(pref)}
        tot = lse(pb, pnb)
        spb = tot + lp[t, 0]
        spnb = np.where(ln > 0, pnb + lp[t, np.maximum(last, 0)], NEG)
        merged = []
        for j in range(nb):
            if ln[j] == 0 or xp[t, last[j]] == NEG:
                continue
            k = where.get(pref[j][:-1])
            if k is None:
                continue
            base = pb[k] if last[j] == last[k] else tot[k]
            spnb[j] = lse(spnb[j], base + xp[t, last[j]])
            merged.append((k, last[j]))
            remerges += int(node[k] != pnode[j])
        base = np.where(cols[None, :] == last[:, None], pb[:, None], tot[:, None])
        ext = base + xp[t][None, :]
        score = ext + beta * (ln[:, None] + 1)
        if use_lm:
            score = score + alpha * (acc[:, None] + lm.logp[lms])
        stay = lse(spb, spnb) + beta * ln + (alpha * acc if use_lm else 0.0)
        score[:, 0] = stay
        for k, c in merged:
            score[k, c] = NEG
        flat = score.ravel()
        ids = np.nonzero(flat > NEG)[0]
        order = ids[np.lexsort((ids, -flat[ids]))]
        max_live = max(max_live, len(order))
        if len(order) > K:
            gap = flat[order[K - 1]] - flat[order[K]]
            if gap == 0.0:
                kth_ties += 1
                if exact_ties:
                    gap = tie_gap(flat[ids], flat[order[K]])
            min_gap = min(min_gap, gap)
        sel = order[:K]
        k, c = sel // V, sel % V
        st = c == 0
        pnode = np.where(st, pnode[k], node[k])
        node = np.where(st, node[k], t * K + np.arange(len(sel)))
        n_pb = np.where(st, spb[k], NEG)
        n_pnb = np.where(st, spnb[k], ext[k, c])
        if lm is not None:
            n_acc = np.where(st, acc[k], acc[k] + lm.logp[lms[k], c])
            n_lms = np.where(st, lms[k], lm.next[lms[k], c])
        else:
            n_acc, n_lms = acc[k], lms[k]
        n_last = np.where(st, last[k], c)
        n_ln = np.where(st, ln[k], ln[k] + 1)
        pref = [pref[kk] if s else pref[kk] + (int(cc),) for kk, cc, s in zip(k, c, st)]
        pb, pnb, acc, last, ln, lms = n_pb, n_pnb, n_acc, n_last, n_ln, n_lms
    ac = lse(pb, pnb)
    lmt = acc + lm.eos[lms] if lm is not None else np.zeros_like(acc)
    total = ac + (alpha * lmt if use_lm else 0.0) + beta * ln
    rank = np.lexsort((np.arange(len(total)), -total))
    for r in range(min(nbest, len(rank) - 1)):
        gap = total[rank[r]] - total[rank[r + 1]]
        if gap == 0.0:
            final_ties += 1
            if exact_ties:
                gap = tie_gap(total, total[rank[r]])
        min_gap = min(min_gap, gap)
    if stats is not None:
        stats.update(kth_ties=kth_ties, final_ties=final_ties, remerges=remerges, max_live=max_live)
    hyps = [(list(pref[i]), float(total[i]), float(ac[i]), float(lmt[i])) for i in rank[:nbest]]
    return hyps, min_gap


def ctc_logprob(lp, labels):
    """ln P_ctc(labels | frames) of class log-probs lp [T, V] (blank 0), fp64 through torch's ctc_loss."""
    import torch
    import torch.nn.functional as F
    T = lp.shape[0]
    lpt = torch.from_numpy(np.ascontiguousarray(lp, dtype=np.float64)).unsqueeze(1)
    tgt = torch.tensor([labels if labels else [1]], dtype=torch.long)
    nll = F.ctc_loss(lpt, tgt, torch.tensor([T]), torch.tensor([len(labels)]), blank=0, reduction="none", zero_infinity=False)
    return -float(nll[0])


def brute_force(logits, classes_used, lm=None, alpha=0.0, beta=0.0, canon=None):
    """Every labelling over `classes_used` of length <= T, scored ln P_ctc + alpha * ln P_lm(y </s>) + beta * |y|, best first
    (ties: shorter, then lexicographic).  Returns [(labels, total, acoustic, lm)] of the finite ones."""
    lp = class_logprobs(logits, canon)
    T = lp.shape[0]
    out = []
    for n in range(T + 1):
        for y in itertools.product(classes_used, repeat=n):
            ac = ctc_logprob(lp, list(y))
            if not np.isfinite(ac):
                continue
            lmv = 0.0
            if lm is not None:
                s = lm.start
                for c in y:
                    lmv += lm.logp[s, c]
                    s = lm.next[s, c]
                lmv += lm.eos[s]
            out.append((list(y), ac + alpha * lmv + beta * n, ac, lmv))
    out.sort(key=lambda h: (-h[1], len(h[0]), h[0]))
    return out
