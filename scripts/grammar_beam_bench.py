"""Time vocr_ctc_grammar_beam_search on configs[1]'s logits shape (T = 294, B = 32, V = 96) with peaky, floored (peaky with every -inf
lifted to 25 below the frame's maximum) and dense logits for K in {1, 4, 16, 64}, without an LM and with the synthetic character
6-gram of scripts/beam_bench.py:
  - under the one-state automaton that accepts everything, against vocr_ctc_beam_search on the same inputs: the ratio is the cost of
    the extra table loads and the state;
  - under a date regex, a 500-word trie and a 20 000-word trie (the last far beyond the sweep kernels' 8192 cells);
  - against the workaround it replaces: BeamDecoder at nbest = K plus a filter on the host (Grammar.accepts over the list), with the
    share of lines on which that finds any accepted string.
HIP events around the device work, wall clock around the workaround (it ends on the host); warm-up, median of repeats.
Output: profiles/r18_grammar_beam_bench.txt.

    python scripts/grammar_beam_bench.py [--repeats 20] [--out profiles/r18_grammar_beam_bench.txt]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vistaocr_amd as va                                    # noqa: E402
from vistaocr_amd import ops                                 # noqa: E402
from vistaocr_amd.grammar import Grammar, pack_dense_grammars  # noqa: E402
from tests import beam_data as bd                            # noqa: E402

T, B, V = 294, 32, 96
KS = (1, 4, 16, 64)


def _time(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def _wall(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def _words(n, seed):
    rng = np.random.default_rng(seed)
    abc = "abcdefghijklmnopqrstuvwxyz"
    out = set()
    while len(out) < n:
        out.add("".join(abc[i] for i in rng.integers(0, 26, size=rng.integers(3, 11))))
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_grammar_beam_bench.txt"))
    args = ap.parse_args()
    from __graft_entry__ import build
    build()
    al = va.english_alphabet()
    canon = np.array(al.canonical_indices())
    cls = np.nonzero(canon == np.arange(V))[0][1:]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    # peaky: one or two finite classes per frame, everything else -inf (most languages have no labelling of finite score at all);
    # floored: the same with every -inf lifted to 25 below the frame's maximum, what a trained model's output looks like; dense: N(0, 3)
    peaky = bd.peaky_logits(np.random.default_rng(7), T, B, V, classes=cls)
    floored = np.where(np.isinf(peaky), peaky.max(axis=2, keepdims=True) - 25.0, peaky).astype(np.float32)
    inputs = (("peaky", torch.from_numpy(peaky).cuda()), ("floored", torch.from_numpy(floored).cuda()),
              ("dense", torch.from_numpy(bd.dense_logits(np.random.default_rng(8), T, B, V)).cuda()))
    tmp = tempfile.mkdtemp()
    path = bd.write_char_arpa(os.path.join(tmp, "char6.arpa"), [al.idx_to_char[c] for c in range(1, 40)], order=6, lines=600, seed=1)
    lm = va.CharNgramLM.from_arpa(path, al)
    lmd = lm.to("cuda")
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda()
    lens_l = [T] * B
    lms = (("none", None, None, 0.0, 0.0), ("6-gram", lm, lmd, 0.8, 1.0))

    grammars = []
    for name, make in (("Sigma*", lambda: Grammar.from_regex(al, ".*")), ("date regex", lambda: Grammar.from_regex(al, r"\d{4}-\d\d-\d\d")),
                       ("500-word trie", lambda: Grammar.from_words(al, _words(500, 1))),
                       ("20000-word trie", lambda: Grammar.from_words(al, _words(20000, 2)))):
        t0 = time.time()
        g = make()
        packed = pack_dense_grammars([g], "cuda")
        say("%-16s %6d states %7d arcs, dense tables %8.2f MiB, built and packed in %.2f s on the host"
            % (name, g.n_states, g.n_arcs, g.n_states * (V + 1) * 4 / 2.0 ** 20, time.time() - t0))
        grammars.append((name, g, packed))

    say("")
    say("T=%d B=%d V=%d, nbest=1, no pruning; median of %d after %d warm-up (ms per batch, HIP events)" % (T, B, V, args.repeats, args.warmup))
    say("1. the automaton that accepts everything against vocr_ctc_beam_search (the same inputs, the same results)")
    say("%-4s %-8s %-7s %12s %14s %8s" % ("K", "LM", "logits", "beam_search", "grammar_beam", "ratio"))
    sigma = grammars[0][2]
    for K in KS:
        for lname, _, lmx, a, bb in lms:
            for iname, lg in inputs:
                r0 = _time(lambda: ops.ctc_beam_search(lg, lens_l, cd, K, 1, lmx, a, bb), args.warmup, args.repeats)
                r1 = _time(lambda: ops.ctc_grammar_beam_search(lg, lens_l, sigma, None, cd, K, 1, lmx, a, bb), args.warmup, args.repeats)
                w, g = ops.ctc_beam_search(lg, lens_l, cd, K, 1, lmx, a, bb), ops.ctc_grammar_beam_search(lg, lens_l, sigma, None, cd, K, 1, lmx, a, bb)
                assert torch.equal(w[0], g[0]) and torch.equal(w[1], g[1])
                say("%-4d %-8s %-7s %12.3f %14.3f %7.2fx" % (K, lname, iname, r0[0], r1[0], r1[0] / r0[0]))

    say("")
    say("2. grammars; 'lines' = lines with an accepted hypothesis")
    say("%-16s %-4s %-8s %-7s %10s %10s %10s %7s" % ("grammar", "K", "LM", "logits", "median", "min", "max", "lines"))
    for gname, g, packed in grammars[1:]:
        for K in KS:
            for lname, _, lmx, a, bb in lms:
                for iname, lg in inputs:
                    r = _time(lambda: ops.ctc_grammar_beam_search(lg, lens_l, packed, None, cd, K, 1, lmx, a, bb), args.warmup, args.repeats)
                    sc = ops.ctc_grammar_beam_search(lg, lens_l, packed, None, cd, K, 1, lmx, a, bb)[2]
                    say("%-16s %-4d %-8s %-7s %10.3f %10.3f %10.3f %4d/%d" % ((gname, K, lname, iname) + r +
                                                                               (int(torch.isfinite(sc[:, 0, 0]).sum()), B)))

    say("")
    say("3. the workaround: BeamDecoder at nbest = K, then Grammar.accepts over the list on the host (wall clock, ms per batch, the "
        "copy and the filter included); 'lines' = lines whose K-best holds any accepted string")
    say("%-16s %-4s %-8s %-7s %10s %10s %10s %7s" % ("grammar", "K", "LM", "logits", "median", "min", "max", "lines"))
    for gname, g, _ in grammars[1:]:
        for K in KS:
            for lname, lmh, _, a, bb in lms:
                dec = va.BeamDecoder(al, beam=K, nbest=K, lm=lmh, lm_weight=a, insertion_bonus=bb)
                for iname, lg in inputs:
                    found = [0]

                    def run():
                        lists = dec.decode_nbest(lg, lens_l)
                        found[0] = sum(1 for lst in lists if any(g.accepts(y) for y, _ in lst))

                    r = _wall(run, 1, max(args.repeats // 4, 3))
                    say("%-16s %-4d %-8s %-7s %10.3f %10.3f %10.3f %4d/%d" % ((gname, K, lname, iname) + r + (found[0], B)))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
