"""fp64 numpy restatement of vocr_ctc_grammar_grad (include/vocr.h): ln P of a line under ITS automaton and the gradient of
sum_b w_b ln P_b with respect to the logits, by alpha and beta over the cells.  Test helper only; shares no code with the product, and
takes only the automaton dicts and the validity rules of tests/grammar_ref.py.

Written from the header's two recursions as an explicit edge list of the product graph, made once per automaton:
    W[s] -> W[s];   A[a] -> A[a];   W[src_a] -> A[a];   A[a] -> W[dst_a];   A[a'] -> A[a] where dst_a' = src_a and the classes differ
alpha_t(c) = lp_t(e(c)) + lse over the edges INTO c of alpha_{t-1}; bhat_t(c) = lp_t(e(c)) + lse over the edges OUT OF c of
bhat_{t+1} (np.logaddexp.reduceat over the edges sorted by head, then by tail: every cell has its self loop, so no group is empty).
No prefix / suffix scans, no mirrored automaton, no groups."""
import numpy as np

from tests import grammar_ref as gr
from tests.align_ref import class_logprobs, classes_of

NEG = -np.inf


class _Graph(object):
    def __init__(self, a, cls):
        S, E = a["S"], len(a["src"])
        self.S, self.E, self.N = S, E, S + E
        src, dst = a["src"].astype(np.int64), a["dst"].astype(np.int64)
        col = cls[a["cls"]].astype(np.int64) if E else np.zeros(0, dtype=np.int64)
        self.emit = np.concatenate([np.zeros(S, dtype=np.int64), col])                 # e(c): the class column a cell emits
        tail = list(range(S + E))                                                     # the self loops
        head = list(range(S + E))
        for i in range(E):
            tail += [int(src[i]), S + i]
            head += [S + i, int(dst[i])]
        out_of = {}
        for i in range(E):
            out_of.setdefault(int(src[i]), []).append(i)
        for i in range(E):                                                            # A[i] -> A[j] for j out of dst_i, other class
            for j in out_of.get(int(dst[i]), ()):
                if col[j] != col[i]:
                    tail.append(S + i)
                    head.append(S + j)
        tail, head = np.array(tail, dtype=np.int64), np.array(head, dtype=np.int64)
        o = np.argsort(head, kind="stable")
        self.in_tail, self.in_start = tail[o], np.searchsorted(head[o], np.arange(self.N))
        o = np.argsort(tail, kind="stable")
        self.out_head, self.out_start = head[o], np.searchsorted(tail[o], np.arange(self.N))
        self.first = np.concatenate([np.arange(S) == 0, src == 0])                    # the cells of frame 0
        acc = a["accept"] != 0
        self.last = np.concatenate([acc, acc[dst] if E else np.zeros(0, dtype=bool)])  # the cells of the last frame

    def line(self, clp):
        """clp [n, V] class log-probabilities.  (ln P, occ [n, V]: the class occupancies, zeros when ln P = -inf)."""
        n, V = clp.shape
        if n == 0:
            return (0.0 if self.last[0] else NEG), np.zeros((0, V))
        e = self.emit
        with np.errstate(invalid="ignore"):
            alpha = np.full((n, self.N), NEG)
            alpha[0] = np.where(self.first, clp[0, e], NEG)
            for t in range(1, n):
                alpha[t] = clp[t, e] + np.logaddexp.reduceat(alpha[t - 1][self.in_tail], self.in_start)
            bhat = np.full((n, self.N), NEG)
            bhat[n - 1] = np.where(self.last, clp[n - 1, e], NEG)
            for t in range(n - 2, -1, -1):
                bhat[t] = clp[t, e] + np.logaddexp.reduceat(bhat[t + 1][self.out_head], self.out_start)
            fin = alpha[n - 1][self.last]
            lnp = float(np.logaddexp.reduce(fin)) if fin.size else NEG
            occ = np.zeros((n, V))
            if lnp != NEG:
                for t in range(n):
                    z = alpha[t] + bhat[t] - clp[t, e] - lnp
                    z = np.where((alpha[t] == NEG) | (bhat[t] == NEG), 0.0, np.exp(np.where(np.isnan(z), NEG, z)))
                    np.add.at(occ[t], e, z)
        return lnp, occ


def run(logits, lens, automata, which, canon=None, weights=None, max_states=None, max_arcs=None):
    """logits [T, B, V]; which [B].  {"logp": [B] fp64, "grad": [T, B, V] fp64 (weights None: weight 1 per line), "occ": [T, B, V]}.
    A line whose automaton is invalid, whose which is outside [0, G) or whose ln P is -inf: -inf and zero rows."""
    x = np.asarray(logits, dtype=np.float64)
    T, B, V = x.shape
    cls = classes_of(V, canon)
    ms = max(a["S"] for a in automata) if max_states is None else max_states
    ma = max(len(a["src"]) for a in automata) if max_arcs is None else max_arcs
    graphs = [_Graph(a, cls) if gr.valid(a, V, cls, ms, ma) else None for a in automata]
    w = np.ones(B) if weights is None else np.asarray(weights, dtype=np.float64)
    logp, grad, occs = np.full(B, NEG), np.zeros((T, B, V)), np.zeros((T, B, V))
    for b in range(B):
        k = int(which[b])
        if k < 0 or k >= len(automata) or graphs[k] is None:
            continue
        n = min(max(int(lens[b]), 0), T)
        clp, _ = class_logprobs(x[:n, b], canon)
        logp[b], occ = graphs[k].line(clp)
        if logp[b] == NEG or n == 0:
            continue
        occs[:n, b] = occ
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            xs = x[:n, b]
            m = xs.max(axis=1, keepdims=True)
            p = np.exp(xs - np.where(m == NEG, 0.0, m))
            p = p / p.sum(axis=1, keepdims=True)                                      # p_t(v)
            P = np.exp(clp)                                                           # P_t(class(v)) at every column
            ratio = np.where(P > 0, occ[:, cls] / np.where(P > 0, P, 1.0), 0.0)
            grad[:n, b] = w[b] * np.where(p > 0, p * (ratio - 1.0), 0.0)
    return {"logp": logp, "grad": grad, "occ": occs}
