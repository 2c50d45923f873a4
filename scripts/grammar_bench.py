"""Time vocr_ctc_grammar_scores on configs[1]'s logits shape (T = 294, B = 32, V = 96), peaky and dense inputs of tests/beam_data.py,
for three sets of grammars: (a) 10 `contains` grammars (.*keyword.*), (b) one date regex, (c) a 500-word trie.  Device time per call
of ops.ctc_grammar_scores, scores only and with best paths, and, for scale, the same recursion written in batched torch on the same
GPU: all lines and all automata of a set at once (the automata concatenated into one table), segmented logsumexp / max through
scatter_reduce, a Python loop over T, no back pointers.  That implementation lives here, not in the product; its log-probabilities are
compared with the kernel's.  For (a) also KeywordSpotter.search on the same keywords (the expected count, a different and cheaper
question).  A timed window is HIP events around enough back-to-back calls for about 50 ms, with every argument on the device already.
Output: profiles/r14_grammar_bench.txt.

    python scripts/grammar_bench.py [--repeats 10] [--out profiles/r14_grammar_bench.txt]"""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, B, V = 294, 32, 96
NEG = float("-inf")
KEYWORDS = ["the", "and", "pay", "sum", "date", "total", "invoice", "pounds", "bearer", "number"]


def _windows(fn, warmup, repeats, window_ms=50.0):
    """`repeats` timed windows of HIP events around n back-to-back calls of fn (n chosen so that a window lasts about window_ms);
    ms per call of every window."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    n = max(1, int(round(window_ms / max(e0.elapsed_time(e1), 1e-3))))
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / n)
    return ms


def _stats(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def inputs(kind):
    from tests import beam_data as bd
    rng = np.random.default_rng(7)
    return bd.peaky_logits(rng, T, B, V, p_char=0.35) if kind == "peaky" else bd.dense_logits(rng, T, B, V)


def grammar_sets(al):
    from vistaocr_amd.grammar import Grammar
    rng = np.random.default_rng(9)
    letters = list("abcdefghijklmnopqrstuvwxyz")
    words = set()
    while len(words) < 500:
        words.add("".join(rng.choice(letters, int(rng.integers(3, 10)))))
    return [("10 contains", [Grammar.contains(al, k) for k in KEYWORDS]),
            ("date regex", [Grammar.from_regex(al, "\\d{1,2}/\\d{1,2}/\\d{4}")]),
            ("500-word trie", [Grammar.from_words(al, sorted(words))])]


class TorchGrammar(object):
    """The recursion of include/vocr.h for a set of automata, concatenated into one table, on [B, cells] tensors."""

    def __init__(self, grammars, dev):
        s_off = np.cumsum([0] + [g.n_states for g in grammars])
        src = np.concatenate([g.arc_src + s_off[i] for i, g in enumerate(grammars)])
        dst = np.concatenate([g.arc_dst + s_off[i] for i, g in enumerate(grammars)])
        col = np.concatenate([g.arc_cls for g in grammars])
        self.S, self.E, self.G = int(s_off[-1]), len(src), len(grammars)
        new = np.ones(self.E, dtype=bool)
        new[1:] = (dst[1:] != dst[:-1]) | (col[1:] != col[:-1])
        grp_of = np.cumsum(new) - 1                                       # the group (destination, class) of every arc
        ngrp = int(grp_of[-1]) + 1
        gdst, gcol = dst[new], col[new]
        by_state = {}
        for gi, d in enumerate(gdst.tolist()):
            by_state.setdefault(d, []).append(gi)
        pa, pg = [], []                                                   # (arc, group into its source of another class)
        for a, (s, c) in enumerate(zip(src.tolist(), col.tolist())):
            for gi in by_state.get(s, ()):
                if gcol[gi] != c:
                    pa.append(a)
                    pg.append(gi)
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.long, device=dev)
        self.src, self.dst, self.col, self.grp_of, self.ngrp = t(src), t(dst), t(col), t(grp_of), ngrp
        self.gdst, self.pa, self.pg = t(gdst), t(pa), t(pg)
        self.start = t(s_off[:-1])
        accept = np.concatenate([g.accept for g in grammars]).astype(bool)
        owner_s = np.concatenate([np.full(g.n_states, i) for i, g in enumerate(grammars)])
        owner_a = np.concatenate([np.full(g.n_arcs, i) for i, g in enumerate(grammars)])
        self.fin_w, self.fin_a = t(np.nonzero(accept)[0]), t(np.nonzero(accept[dst])[0])
        self.fin_owner = t(np.concatenate([owner_s[accept], owner_a[accept[dst]]]))
        self.pairs = len(pa)

    @staticmethod
    def seg(vals, index, n, use_max):
        """Segmented logsumexp (or max) of vals [B, P] by index [P] into [B, n]; an empty segment is -inf."""
        idx = index[None, :].expand(vals.shape[0], -1)
        m = torch.full((vals.shape[0], n), NEG, device=vals.device).scatter_reduce(1, idx, vals, "amax", include_self=True)
        if use_max:
            return m
        ms = m.masked_fill(m == NEG, 0.0)
        s = torch.zeros_like(m).scatter_add(1, idx, torch.exp(vals - ms.gather(1, idx)))
        return ms + torch.log(s)

    def run(self, lp, use_max):
        """lp [T, B, V] log-softmax (full-length lines); [B, G]."""
        op = torch.maximum if use_max else torch.logaddexp
        nb = lp.shape[1]
        W = torch.full((nb, self.S), NEG, device=lp.device)
        W[:, self.start] = lp[0][:, :1]
        first = (self.src[:, None] == self.start[None, :]).any(dim=1)
        A = lp[0][:, self.col].masked_fill(~first[None, :], NEG)
        for t in range(1, lp.shape[0]):
            grp = self.seg(A, self.grp_of, self.ngrp, use_max)
            inc = self.seg(grp, self.gdst, self.S, use_max)
            other = self.seg(grp[:, self.pg], self.pa, self.E, use_max)
            A = lp[t][:, self.col] + op(op(A, W[:, self.src]), other)
            W = lp[t][:, :1] + op(W, inc)
        fin = torch.cat([W[:, self.fin_w], A[:, self.fin_a]], dim=1)
        return self.seg(fin, self.fin_owner, self.G, use_max)


def class_logprobs(xd, canon):
    """[T, B, V] log-softmax with, at every class's canonical column, the logsumexp over the class's members."""
    lp = torch.log_softmax(xd, dim=2)
    canon = np.asarray(canon)
    for c in np.unique(canon):
        members = np.nonzero(canon == c)[0]
        if len(members) > 1:
            lp[:, :, int(c)] = torch.logsumexp(lp[:, :, torch.as_tensor(members, device=xd.device)], dim=2)
    return lp


def clocks():
    """The device's clocks as the management tool prints them (read only), or a note that it could not be asked."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30)
        keep = [l.strip() for l in r.stdout.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l)]
        return "; ".join(keep) if keep else "rocm-smi printed no clocks"
    except Exception as e:                                                # noqa: BLE001
        return "clocks not read (%s)" % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10, help="timed windows per measurement")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-repeats", type=int, default=3, help="timed calls of the torch composition (each is hundreds of launches)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_grammar_bench.txt"))
    args = ap.parse_args()
    from __graft_entry__ import build
    build()
    import vistaocr_amd as va
    from vistaocr_amd import ops
    from vistaocr_amd.grammar import pack_grammars
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    al = va.english_alphabet()
    assert len(al) == V
    say("device: %s; clocks before: %s" % (torch.cuda.get_device_name(0), clocks()))
    say("vocr_ctc_grammar_scores, T=%d B=%d V=%d, every line of full length" % (T, B, V))
    say("a timed window: HIP events around n back-to-back calls of ops.ctc_grammar_scores, n chosen for a window of about 50 ms, ms per "
        "call = window / n; %d windows after %d warm-up calls; median / min / max.  Logits, lens and the packed automata are device "
        "tensors: a call is the wrapper's checks, its output allocations and the launches (class log-probabilities, plan, sum sweep, and "
        "with best paths the max sweep), no host-to-device copy and no synchronise inside a window." % (args.repeats, args.warmup))
    say("torch: the same recursion on [B, cells] tensors with scatter_reduce, all automata of a set at once, a Python loop over T; one "
        "warm-up call, then the median of %d single calls between HIP events.  torch sum: ln P only; torch sum+max: both recursions, "
        "without back pointers or labels." % args.torch_repeats)
    fmt = "%-6s %-14s %6s %6s %5s | %8s %8s %8s | %8s %8s %8s | %10s %7s %12s %7s | %8s"
    say(fmt % ("input", "grammars", "states", "arcs", "maxD", "scores", "min", "max", "+best", "min", "max", "torch sum", "ratio",
               "torch sum+max", "ratio", "|diff|"))
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    canon = torch.as_tensor(al.canonical_indices(), dtype=torch.int32).cuda()
    sets = grammar_sets(al)
    kws = {}
    for kind in ("peaky", "dense"):
        x = inputs(kind)
        xd = torch.from_numpy(x).cuda()
        lp = class_logprobs(xd, al.canonical_indices())
        for name, grammars in sets:
            gp = pack_grammars(grammars, "cuda")
            s_only = _stats(_windows(lambda: ops.ctc_grammar_scores(xd, lens, gp, canon, False), args.warmup, args.repeats))
            w_best = _stats(_windows(lambda: ops.ctc_grammar_scores(xd, lens, gp, canon, True), args.warmup, args.repeats))
            tg = TorchGrammar(grammars, "cuda")
            t_sum = _stats(_windows(lambda: tg.run(lp, False), 1, args.torch_repeats, window_ms=0.0))[0]
            t_both = _stats(_windows(lambda: (tg.run(lp, False), tg.run(lp, True)), 1, args.torch_repeats, window_ms=0.0))[0]
            mine = ops.ctc_grammar_scores(xd, lens, gp, canon, False)[0]
            ref = tg.run(lp, False)
            fin = torch.isfinite(ref) & torch.isfinite(mine)
            same_inf = bool((torch.isfinite(ref) == torch.isfinite(mine)).all())
            diff = float((ref[fin] - mine[fin]).abs().max()) if bool(fin.any()) else 0.0
            say(fmt % (kind, name, sum(g.n_states for g in grammars), sum(g.n_arcs for g in grammars), max(g.max_in_degree for g in grammars),
                       "%.3f" % s_only[0], "%.3f" % s_only[1], "%.3f" % s_only[2], "%.3f" % w_best[0], "%.3f" % w_best[1], "%.3f" % w_best[2],
                       "%.1f" % t_sum, "%.1fx" % (t_sum / s_only[0]), "%.1f" % t_both, "%.1fx" % (t_both / w_best[0]),
                       "%.2g%s" % (diff, "" if same_inf else " inf!")))
        sp = va.KeywordSpotter(al)
        kws[kind] = _stats(_windows(lambda: sp.search(xd, lens, KEYWORDS), args.warmup, args.repeats))
    say("")
    for kind in ("peaky", "dense"):
        say("%s: KeywordSpotter.search on the same 10 keywords (expected counts and best spans, not the probability; the whole call: the "
            "queries packed on the host and copied to the device, the kernels, one device-to-host copy of the results, which the grammar "
            "columns above do not include): %.3f ms per call (min %.3f, max %.3f)" % ((kind,) + kws[kind]))
    say("")
    say("scores / +best: ms per call of ops.ctc_grammar_scores without / with best paths (median, min, max of the windows).  states, arcs: "
        "the sum over the set's automata; maxD: the largest in-degree.  ratio: torch / kernel, both medians.  |diff|: the largest "
        "difference of the two ln P (fp32 both).")
    say("clocks after: %s" % clocks())
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
