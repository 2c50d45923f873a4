"""fp64 numpy restatement of vocr_ctc_grammar_scores (vistaocr_amd/csrc/ctc_grammar.hip) and an independent brute force over all frame
paths.  Test helper only; shares no code with the product.

An automaton is a dict: S (states, 0 the start), src / cls / dst (int arrays, the arcs sorted by (dst, class, src)), accept (int
array [S]).  search() runs both recursions of include/vocr.h - the sum and the max - one frame at a time, vectorised over the cells with
np.logaddexp.reduceat / np.maximum.reduceat: first one value per GROUP of incoming arcs (same destination, same class), then per state
the reduction over its groups, and per arc the reduction over the groups of its source state EXCEPT the one of its own class, through a
list of (arc, group) pairs made once per automaton (so no subtraction anywhere, and not the kernel's prefix / suffix scans either).
brute_force() enumerates all V^T frame paths, collapses each, runs the automaton on the labelling and sums / maximises."""
import itertools

import numpy as np

from tests.align_ref import class_logprobs, classes_of

NEG = -np.inf


def make(S, arcs, accept, V=None, canon=None):
    """An automaton from a list of (src, cls, dst), sorted into the kernel's order."""
    cls = classes_of(V, canon) if V is not None else None
    key = (lambda a: (a[2], int(cls[a[1]]) if cls is not None and 0 <= a[1] < len(cls) else a[1], a[0]))
    arcs = sorted(arcs, key=key)
    acc = np.zeros(S, dtype=np.int32)
    acc[list(accept)] = 1
    return {"S": int(S), "src": np.array([a[0] for a in arcs], dtype=np.int32), "cls": np.array([a[1] for a in arcs], dtype=np.int32),
            "dst": np.array([a[2] for a in arcs], dtype=np.int32), "accept": acc}


def from_grammar(g):
    """The tables of a vistaocr_amd.grammar.Grammar."""
    return {"S": g.n_states, "src": g.arc_src.copy(), "cls": g.arc_cls.copy(), "dst": g.arc_dst.copy(), "accept": g.accept.copy()}


def valid(a, V, cls, max_states, max_arcs):
    """The rules of include/vocr.h."""
    S, E = a["S"], len(a["src"])
    if S < 1 or S > max_states or E > max_arcs:
        return False
    src, c, dst = a["src"], a["cls"], a["dst"]
    if E == 0:
        return True
    if np.any(src < 0) or np.any(src >= S) or np.any(dst < 0) or np.any(dst >= S) or np.any(c <= 0) or np.any(c >= V):
        return False
    k = cls[c]
    if np.any(k == 0):
        return False
    keys = list(zip(dst.tolist(), k.tolist(), src.tolist()))
    return all(keys[i] <= keys[i + 1] for i in range(E - 1))


def max_in_degree(a):
    d = a["dst"][a["dst"] >= 0]                                          # (an invalid automaton may hold anything)
    return int(np.bincount(d, minlength=1).max()) if len(d) else 0


def accepts(a, labels, cls):
    """Whether the automaton accepts a labelling (a set of states is carried: it need not be deterministic)."""
    states = {0}
    k = cls[a["cls"]] if len(a["cls"]) else a["cls"]
    for v in labels:
        c = int(cls[int(v)])
        states = {int(d) for s_, k_, d in zip(a["src"], k, a["dst"]) if int(s_) in states and int(k_) == c}
        if not states:
            return False
    return any(a["accept"][s] for s in states)


class _Plan(object):
    """What the frame loop needs of one automaton."""

    def __init__(self, a, cls):
        self.S, self.E = a["S"], len(a["src"])
        self.src, self.dst = a["src"].astype(np.int64), a["dst"].astype(np.int64)
        self.col = cls[a["cls"]].astype(np.int64) if self.E else np.zeros(0, dtype=np.int64)
        E = self.E
        if E:
            new = np.ones(E, dtype=bool)
            new[1:] = (self.dst[1:] != self.dst[:-1]) | (self.col[1:] != self.col[:-1])
            self.grp_start = np.nonzero(new)[0]                           # the groups: same destination, same class
            gdst, gcol = self.dst[self.grp_start], self.col[self.grp_start]
            snew = np.ones(len(gdst), dtype=bool)
            snew[1:] = gdst[1:] != gdst[:-1]
            self.st_start = np.nonzero(snew)[0]                           # per state with incoming arcs: its first group
            self.st_ids = gdst[self.st_start]
            by_state = {}
            for gi, (d, c) in enumerate(zip(gdst.tolist(), gcol.tolist())):
                by_state.setdefault(d, []).append((gi, c))
            G = len(gdst)
            pairs, off = [], []
            for s_, c in zip(self.src.tolist(), self.col.tolist()):
                off.append(len(pairs))
                pairs.append(G)                                           # a group that is always -inf: no arc is left without a pair
                pairs.extend(gi for gi, gc in by_state.get(s_, ()) if gc != c)
            self.pairs, self.pair_off = np.array(pairs, dtype=np.int64), np.array(off, dtype=np.int64)
        self.fin_w = np.nonzero(a["accept"])[0]
        self.fin_a = np.nonzero(a["accept"][self.dst])[0] if E else np.zeros(0, dtype=np.int64)

    def run(self, clp, op):
        """clp [len, V] class log-probabilities; op np.logaddexp or np.maximum.  The final value."""
        S, E = self.S, self.E
        n = clp.shape[0]
        if n == 0:
            return 0.0 if 0 in self.fin_w else NEG
        W = np.full(S, NEG)
        W[0] = clp[0, 0]
        A = np.where(self.src == 0, clp[0, self.col], NEG) if E else np.zeros(0)
        with np.errstate(invalid="ignore"):
            for t in range(1, n):
                inc = np.full(S, NEG)
                if E:
                    grp = op.reduceat(A, self.grp_start)
                    inc[self.st_ids] = op.reduceat(grp, self.st_start)
                    other = op.reduceat(np.concatenate([grp, [NEG]])[self.pairs], self.pair_off)
                    A = clp[t, self.col] + op(op(A, W[self.src]), other)
                W = clp[t, 0] + op(W, inc)
            fin = np.concatenate([W[self.fin_w], A[self.fin_a] if E else np.zeros(0), [NEG]])
            return float(op.reduce(fin))


def search(logits, lens, automata, canon=None, max_states=None, max_arcs=None):
    """logits [T, B, V]; returns {"logp": [B, G], "best": [B, G]} fp64; an invalid automaton's column is -inf."""
    x = np.asarray(logits, dtype=np.float64)
    T, B, V = x.shape
    cls = classes_of(V, canon)
    ms = max(a["S"] for a in automata) if max_states is None else max_states
    ma = max(len(a["src"]) for a in automata) if max_arcs is None else max_arcs
    logp, best = np.full((B, len(automata)), NEG), np.full((B, len(automata)), NEG)
    plans = [_Plan(a, cls) if valid(a, V, cls, ms, ma) else None for a in automata]
    for b in range(B):
        n = min(max(int(lens[b]), 0), T)
        clp, _ = class_logprobs(x[:n, b], canon)
        for g, p in enumerate(plans):
            if p is not None:
                logp[b, g], best[b, g] = p.run(clp, np.logaddexp), p.run(clp, np.maximum)
    return {"logp": logp, "best": best}


def collapse(path, cls):
    out, prev = [], 0
    for v in path:
        c = int(cls[v])
        if c != 0 and c != prev:
            out.append(c)
        prev = c
    return out


def brute_force(logits, a, canon=None):
    """logits [T, V] of ONE line, a DETERMINISTIC automaton: (ln of the summed probability of all frame paths whose labelling is
    accepted, the largest single path's log-probability), by enumeration.  Independent of search(): the row's log-softmax, a dict of
    transitions, itertools.product."""
    x = np.asarray(logits, dtype=np.float64)
    T, V = x.shape
    cls = classes_of(V, canon)
    kinds = sorted(set(cls.tolist()))                                     # a frame emits a CLASS: its probability is its members' sum
    with np.errstate(divide="ignore"):
        p = np.exp(x - x.max(axis=1, keepdims=True))
        p = p / p.sum(axis=1, keepdims=True)
        lp = np.full((T, V), NEG)
        for c in kinds:
            lp[:, c] = np.log(p[:, cls == c].sum(axis=1))
    step = {}
    for s_, c, d in zip(a["src"].tolist(), a["cls"].tolist(), a["dst"].tolist()):
        assert step.setdefault((s_, int(cls[c])), d) == d, "brute_force needs a deterministic automaton"
    total, top = 0.0, NEG
    for path in itertools.product(kinds, repeat=T):
        s_ = 0
        for c in collapse(path, cls):
            s_ = step.get((s_, c))
            if s_ is None:
                break
        if s_ is None or not a["accept"][s_]:
            continue
        p = float(sum(lp[t, v] for t, v in enumerate(path)))
        total += np.exp(p)
        top = max(top, p)
    return (float(np.log(total)) if total > 0 else NEG), top
