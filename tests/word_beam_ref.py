"""CPU restatement of vocr_ctc_word_beam_search (vistaocr_amd/csrc/ctc_word_beam.hip) in fp64 numpy, and the brute-force scorer it is
checked against.  Test helper only: the product never imports it.

The restatement follows the kernel's rules exactly (the CTC side is tests/beam_ref.py's: classes, stay / extend, merging, the total
order (score desc, slot id k*V + c asc), the end-of-line ranking with ties by the rank at the last frame): a beam is outside a word,
inside an open word at a trie node or OOV; it is ranked by logsumexp(p_b, p_nb) + alpha * (LM of its closed tokens + look-ahead) +
beta * closed tokens; letters step the trie, spaces close the open word, singles close it and add their token; candidates whose LM
term is -inf are never taken; at the end the open word is closed and </s> added, and beams whose word cannot close are dropped.  It
reads the resolved tables of WordNgramLM.  It also returns the smallest score gap at any decision the search took, and takes
beam_ref.beam_search's `exact_ties` and `stats` keywords with the same meaning (node ids tracked as the kernel assigns them).

The brute force shares nothing with those tables: every labelling is scored by beam_ref.ctc_logprob, textutils.form_tokenized_words
and a direct recursive ARPA backoff over the parsed n-gram dict."""
import itertools

import numpy as np

from tests import beam_ref as br
from vistaocr_amd.lm import KIND_LETTER, KIND_SINGLE, KIND_SPACE, LN10
from vistaocr_amd.textutils import _DIGITS, _PUNCT, form_tokenized_words

NEG = -np.inf
OUT, OOV = -1, -2


class _Tables(object):
    """Memoised lookups of one WordNgramLM (the restatement asks the same (state, token) many times)."""

    def __init__(self, lm, oov):
        self.lm, self.oov = lm, oov
        self.cache = {}
        self.la_oov = NEG if oov is None else lm.lookup(0, lm.unk)[0] + oov

    def lookup(self, s, w):
        key = (s, w)
        if key not in self.cache:
            self.cache[key] = self.lm.lookup(s, w)
        return self.cache[key]

    def close(self, wn, s):
        t = int(self.lm.trie_tok[wn]) if wn >= 0 else -1
        if t >= 0:
            return self.lookup(s, t)
        if self.oov is None:
            return NEG, s
        lp, ns = self.lookup(s, self.lm.unk)
        return lp + self.oov, ns

    def extend(self, st, c):
        """The state (wn, acc, lms, ntok, la, clp, cst) after class c, or None (not a candidate)."""
        wn, acc, lms, ntok, la, clp, cst = st
        kd = int(self.lm.kind[c])
        if kd == KIND_LETTER:
            nw = OOV
            if wn != OOV:
                nx = int(self.lm.trie_next[max(wn, 0), c])
                if nx > 0:
                    nw = nx
            if nw == OOV:
                if self.oov is None:
                    return None
                if wn == OOV:
                    return (OOV, acc, lms, ntok, self.la_oov, clp, cst)
                ncl, ncs = self.close(OOV, lms)
                return (OOV, acc, lms, ntok, self.la_oov, ncl, ncs)
            ncl, ncs = self.close(nw, lms)
            return (nw, acc, lms, ntok, float(self.lm.trie_la[nw]), ncl, ncs)
        if kd not in (KIND_SPACE, KIND_SINGLE):
            return None
        if wn != OUT:
            if clp == NEG:
                return None
            acc, lms, ntok = acc + clp, cst, ntok + 1
        if kd == KIND_SINGLE:
            lp, lms = self.lookup(lms, int(self.lm.tok[c]))
            acc, ntok = acc + lp, ntok + 1
        return (OUT, acc, lms, ntok, 0.0, 0.0, lms)


def beam_search(logits, length, K, lm, nbest=1, canon=None, alpha=0.0, beta=0.0, oov=None, exact_ties=False, stats=None):
    """One line: logits [T, V] raw, lm a WordNgramLM, oov the oov_penalty (None: closed vocabulary).  Returns (hyps, min_gap):
    hyps = [(labels, total, acoustic, lm)] best first (at most nbest), min_gap the smallest decision gap.

    exact_ties, stats: as in beam_ref.beam_search.  exact_ties is sound ONLY where the tied candidates come from bitwise-duplicated
    columns whose classes the LM also treats alike (the same kind, trie step, look-ahead and close score), so that they go through
    identical operation sequences in fp32 and in fp64."""
    logits = np.asarray(logits, dtype=np.float64)
    T, V = logits.shape
    L = int(min(max(length, 0), T))
    lp = br.class_logprobs(logits[:L], canon) if L else np.zeros((0, V))
    xp = lp.copy()
    if L:
        xp[:, 0] = NEG
    tb = _Tables(lm, oov)
    use_lm = alpha != 0.0
    pb, pnb = np.array([0.0]), np.array([NEG])
    last, ln = np.array([-1]), np.array([0])
    state = [(OUT, 0.0, lm.start, 0, 0.0, 0.0, lm.start)]
    pref = [()]
    node, pnode = [-1], [-1]                                # the kernel's pool node of each beam, and that node's parent
    kth_ties = final_ties = remerges = max_live = 0
    min_gap = np.inf
    for t in range(L):
        nb = len(pref)
        where = {p: k for k, p in enumerate(pref)}
        tot = br.lse(pb, pnb)
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
            spnb[j] = br.lse(spnb[j], base + xp[t, last[j]])
            merged.append((k, last[j]))
            remerges += int(node[k] != pnode[j])
        score = np.full((nb, V), NEG)
        ext_state = {}
        cols = [c for c in range(1, V) if xp[t, c] > NEG]
        for k in range(nb):
            wn, acc, lms, ntok, la = state[k][:5]
            score[k, 0] = br.lse(spb[k], spnb[k]) + (alpha * (acc + la) if use_lm else 0.0) + beta * ntok
            for c in cols:
                e = tb.extend(state[k], c)
                if e is None or not e[1] + e[4] > NEG:
                    continue
                base = pb[k] if c == last[k] else tot[k]
                score[k, c] = base + xp[t, c] + (alpha * (e[1] + e[4]) if use_lm else 0.0) + beta * e[3]
                ext_state[(k, c)] = e
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
                    gap = br.tie_gap(flat[ids], flat[order[K]])
            min_gap = min(min_gap, gap)
        sel = order[:K]
        n_pb, n_pnb, n_last, n_ln, n_state, n_pref, n_node, n_pnode = [], [], [], [], [], [], [], []
        for q, i in enumerate(sel):
            k, c = int(i) // V, int(i) % V
            if c == 0:
                n_pb.append(spb[k]); n_pnb.append(spnb[k]); n_last.append(last[k]); n_ln.append(ln[k])
                n_state.append(state[k]); n_pref.append(pref[k]); n_node.append(node[k]); n_pnode.append(pnode[k])
            else:
                base = pb[k] if c == last[k] else tot[k]
                n_pb.append(NEG); n_pnb.append(base + xp[t, c]); n_last.append(c); n_ln.append(ln[k] + 1)
                n_state.append(ext_state[(k, c)]); n_pref.append(pref[k] + (c,)); n_node.append(t * K + q); n_pnode.append(node[k])
        pb, pnb = np.array(n_pb, dtype=np.float64), np.array(n_pnb, dtype=np.float64)
        last, ln = np.array(n_last, dtype=np.int64), np.array(n_ln, dtype=np.int64)
        state, pref, node, pnode = n_state, n_pref, n_node, n_pnode
    ac = br.lse(pb, pnb)
    total, lmt = np.full(len(pref), NEG), np.full(len(pref), NEG)
    for j, (wn, acc, lms, ntok, la, clp, cst) in enumerate(state):
        if wn != OUT:
            if clp == NEG:
                continue
            acc, lms, ntok = acc + clp, cst, ntok + 1
        lmt[j] = acc + tb.lookup(lms, lm.eos)[0]
        total[j] = ac[j] + (alpha * lmt[j] if use_lm else 0.0) + beta * ntok
    rank = np.lexsort((np.arange(len(total)), -total))
    rank = [r for r in rank if total[r] > NEG]
    for r in range(min(nbest, len(rank) - 1)):
        gap = total[rank[r]] - total[rank[r + 1]]
        if gap == 0.0:
            final_ties += 1
            if exact_ties:
                gap = br.tie_gap(total[total > NEG], total[rank[r]])
        min_gap = min(min_gap, gap)
    if stats is not None:
        stats.update(kth_ties=kth_ties, final_ties=final_ties, remerges=remerges, max_live=max_live)
    hyps = [(list(pref[i]), float(total[i]), float(ac[i]), float(lmt[i])) for i in rank[:nbest]]
    return hyps, min_gap


def direct_logp(grams, hist, w, unk_logp=None):
    """ln P(w | hist) by the ARPA backoff rule over the parsed n-grams ({order: {tuple: (log10 p, log10 bo)}}), hist any tuple; a w
    that is not a 1-gram is <unk> (unk_logp when the LM lists no <unk>)."""
    N = max(grams)
    if (w,) not in grams[1]:
        if ("<unk>",) not in grams[1]:
            return unk_logp
        w = "<unk>"
    h = tuple(hist[-(N - 1):]) if N > 1 else ()
    total = 0.0
    while True:
        if h + (w,) in grams[len(h) + 1]:
            return (total + grams[len(h) + 1][h + (w,)][0]) * LN10
        if h and h in grams[len(h)]:
            total += grams[len(h)][h][1]
        h = h[1:]


def lm_score(grams, tokens, oov=None, unk_logp=None):
    """LM(y) of a token list: every token from its full history after <s>, then </s>.  A letter-word that is not a 1-gram is <unk>
    + oov (None: -inf), a single the LM does not list is <unk>; without <unk> in the LM an <unk> scores unk_logp and the history
    starts again from empty."""
    has_unk = ("<unk>",) in grams[1]
    hist = ("<s>",)
    total = 0.0
    for tok in tokens + ["</s>"]:
        single = tok in _PUNCT or tok in _DIGITS or tok == "</s>"
        if (tok,) in grams[1]:
            total += direct_logp(grams, hist, tok)
            hist = hist + (tok,)
            continue
        if not single:
            if oov is None:
                return NEG
            total += oov
        if has_unk:
            total += direct_logp(grams, hist, "<unk>")
            hist = hist + ("<unk>",)
        else:
            total += unk_logp
            hist = ()
    return total


def brute_force(logits, classes_used, alphabet, grams, alpha=0.0, beta=0.0, oov=None, unk_logp=None, canon=None):
    """Every labelling over `classes_used` of length <= T with a finite LM score, scored ln P_ctc + alpha * LM + beta * n_tokens,
    best first (ties: shorter, then lexicographic).  Returns [(labels, total, acoustic, lm)]."""
    lp = br.class_logprobs(logits, canon)
    T = lp.shape[0]
    out = []
    for n in range(T + 1):
        for y in itertools.product(classes_used, repeat=n):
            ac = br.ctc_logprob(lp, list(y))
            if not np.isfinite(ac):
                continue
            toks = form_tokenized_words([alphabet.idx_to_char[c] for c in y])
            lmv = lm_score(grams, toks, oov, unk_logp)
            if lmv == NEG:
                continue
            out.append((list(y), ac + alpha * lmv + beta * len(toks), ac, lmv))
    out.sort(key=lambda h: (-h[1], len(h[0]), h[0]))
    return out
