"""CPU restatement of vocr_ctc_grammar_beam_search (vistaocr_amd/csrc/ctc_beam.hip, the GRAMMAR instantiation) in fp64 numpy for one line.  Test helper
only: the product never imports it.

It is tests/beam_ref.py's beam_search (whose helpers it imports) plus what the grammar adds: every beam carries the state of a
deterministic automaton given as the dense tables of Grammar.dense_tables() (next [S,V], -1: no arc; dist [S], the fewest symbols to
an accepting state, 0 exactly for accepting states); at frame t with rem = L - 1 - t frames left, an extension by class c of a beam
in state s is a candidate only if n = next[s, c] is a state and 0 <= dist[n] <= rem, a stay only if 0 <= dist[s] <= rem; the final
ranking keeps accepting beams only.  A next state outside [0, S) is no arc and a negative distance is "cannot accept", as in the
kernel.  Returns the hypotheses and the smallest decision gap exactly as beam_ref.beam_search does (the K-th against the (K+1)-th
VIABLE candidate of every frame, and neighbouring ranks of the accepted n-best)."""
import numpy as np

from tests.beam_ref import NEG, class_logprobs, classes, lse, tie_gap


def sigma_star(V, canon=None):
    """The dense tables of the one-state automaton that accepts every labelling."""
    cls = classes(canon, V)
    nxt = np.full((1, V), -1, dtype=np.int32)
    nxt[0, [c for c in range(1, V) if cls[c] == c and cls[c] != 0]] = 0
    return nxt, np.zeros(1, dtype=np.int32)


def beam_search(logits, length, tables, K, nbest=1, canon=None, lm=None, alpha=0.0, beta=0.0, prune=None, exact_ties=False):
    """One line: logits [T, V] raw, tables = (next [S,V], dist [S]).  lm as for beam_ref.beam_search.
    Returns (hyps, min_gap): hyps = [(labels, total, acoustic, lm)] best first (at most nbest, accepted only)."""
    nxt_tab, dist_tab = np.asarray(tables[0], dtype=np.int64), np.asarray(tables[1], dtype=np.int64)
    S = dist_tab.shape[0]
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
    last, ln, lms, gst = np.array([-1]), np.array([0]), np.array([start]), np.array([0])
    pref = [()]
    min_gap = np.inf
    cols = np.arange(V)
    for t in range(L):
        nb = len(pref)
        if nb == 0:
            break
        rem = L - 1 - t
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
        base = np.where(cols[None, :] == last[:, None], pb[:, None], tot[:, None])
        ext = base + xp[t][None, :]
        score = ext + beta * (ln[:, None] + 1)
        if use_lm:
            score = score + alpha * (acc[:, None] + lm.logp[lms])
        stay = lse(spb, spnb) + beta * ln + (alpha * acc if use_lm else 0.0)
        # the grammar: the state after each extension, and which candidates the frames left can still complete
        n_all = nxt_tab[gst]                                                   # [nb, V]
        arc = (n_all >= 0) & (n_all < S)
        d_all = np.where(arc, dist_tab[np.where(arc, n_all, 0)], -1)
        score = np.where((d_all >= 0) & (d_all <= rem), score, NEG)
        d_stay = dist_tab[gst]
        score[:, 0] = np.where((d_stay >= 0) & (d_stay <= rem), stay, NEG)
        for k, c in merged:
            score[k, c] = NEG
        flat = score.ravel()
        ids = np.nonzero(flat > NEG)[0]
        order = ids[np.lexsort((ids, -flat[ids]))]
        if len(order) > K:
            gap = flat[order[K - 1]] - flat[order[K]]
            if gap == 0.0 and exact_ties:
                gap = tie_gap(flat[ids], flat[order[K]])
            min_gap = min(min_gap, gap)
        sel = order[:K]
        k, c = sel // V, sel % V
        st = c == 0
        n_pb = np.where(st, spb[k], NEG)
        n_pnb = np.where(st, spnb[k], ext[k, c])
        if lm is not None:
            n_acc = np.where(st, acc[k], acc[k] + lm.logp[lms[k], c])
            n_lms = np.where(st, lms[k], lm.next[lms[k], c])
        else:
            n_acc, n_lms = acc[k], lms[k]
        n_gst = np.where(st, gst[k], n_all[k, c])
        n_last = np.where(st, last[k], c)
        n_ln = np.where(st, ln[k], ln[k] + 1)
        pref = [pref[kk] if s else pref[kk] + (int(cc),) for kk, cc, s in zip(k, c, st)]
        pb, pnb, acc, last, ln, lms, gst = n_pb, n_pnb, n_acc, n_last, n_ln, n_lms, n_gst
    if len(pref) == 0:
        return [], min_gap
    ac = lse(pb, pnb)
    lmt = acc + lm.eos[lms] if lm is not None else np.zeros_like(acc)
    total = ac + (alpha * lmt if use_lm else 0.0) + beta * ln
    keep = np.nonzero(dist_tab[gst] == 0)[0]                                   # the accepting filter
    rank = keep[np.lexsort((keep, -total[keep]))]
    for r in range(min(nbest, len(rank) - 1)):
        gap = total[rank[r]] - total[rank[r + 1]]
        if gap == 0.0 and exact_ties:
            gap = tie_gap(total[keep], total[rank[r]])
        min_gap = min(min_gap, gap)
    hyps = [(list(pref[i]), float(total[i]), float(ac[i]), float(lmt[i])) for i in rank[:nbest]]
    return hyps, min_gap
