"""Time the weighted grammar entries on configs[1]'s logits shape (T = 294, B = 32, V = 96), on peaky logits and on the dense logits of
the untrained configs[1] model, and hold the UNWEIGHTED entries to the parent commit's library:

  twins    each weighted entry against its unweighted twin on the same automaton (random weights in [-2, 2]): a date regex, a 500-word
           trie and 10 `contains` grammars - scores only, scores with best paths, the gradient (line b against grammar b mod G), and
           the beam search at K = 16;
  boost    Grammar.boost of 50 phrases with the synthetic 6-gram under GrammarBeamDecoder's kernel against vocr_ctc_beam_search with
           the same 6-gram, K = 16;
  ngram    Grammar.from_ngram of a digit-alphabet trigram (V = 11) as a score and as a gradient;
  parent   (--parent <libvocr.so of the parent commit>): the calls of `twins` that go to the three UNWEIGHTED entries, made on the C
           entries with tensors this script owns (workspaces included) on both libraries in this process, windows of --window calls alternating for
           --rounds rounds.  Per call and library the median of the round medians and the parent's own max - min over its rounds; the
           new median must not exceed the parent's median plus that spread (exit 1 otherwise).

No target is set for the weighted entries: the ratios are reported as they come.  A timed window is HIP events around enough
back-to-back calls for about 50 ms (scripts/risk_bench.py's _windows).  Output: profiles/r19_wgrammar_bench.txt.

    python scripts/wgrammar_bench.py [--repeats 7] [--parent scripts/_cut/libvocr.so] [--out profiles/r19_wgrammar_bench.txt]"""
import argparse
import ctypes
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from risk_bench import B, T, V, _logits, _windows  # noqa: E402

DATE = r"\d\d/\d\d/\d\d\d\d"
UNWEIGHTED = ("vocr_ctc_grammar_scores", "vocr_ctc_grammar_grad", "vocr_ctc_grammar_beam_search")


def _reweighted(g, rng):
    """the same automaton with random weights in [-2, 2] on every arc and accepting state"""
    from vistaocr_amd.grammar import Grammar
    trans, acc = g.dfa()
    tw = [{c: float(rng.uniform(-2, 2)) for c in row} for row in trans]
    return Grammar(g.alphabet, trans, acc, name="weighted " + g.name, arc_w=tw, final_w=[float(rng.uniform(-2, 2)) for _ in acc],
                   as_given=True)


def _grammar_sets(al, rng):
    from vistaocr_amd.grammar import Grammar
    abc = "abcdefghijklmnopqrstuvwxyz"
    words = sorted({"".join(abc[i] for i in rng.integers(0, 26, size=rng.integers(3, 9))) for _ in range(520)})[:500]
    keys = ["the", "and", "ing", "tion", "date", "name", "total", "no", "page", "of"]
    return {"date regex": [Grammar.from_regex(al, DATE)], "500-word trie": [Grammar.from_words(al, words)],
            "10 contains": [Grammar.contains(al, k) for k in keys]}


def _legs(x, lens, canon, sets, rng):
    """name -> (unweighted fn, weighted fn)"""
    from vistaocr_amd import ops
    from vistaocr_amd.grammar import pack_dense_grammars, pack_grammars
    legs = {}
    for name, gs in sets.items():
        ws = [_reweighted(g, rng) for g in gs]
        pu, pw = pack_grammars(gs, "cuda"), pack_grammars(ws, "cuda")
        du, dw = pack_dense_grammars(gs, "cuda"), pack_dense_grammars(ws, "cuda")
        which = torch.arange(B, dtype=torch.int32, device="cuda") % len(gs)
        wl = which.tolist()
        ones = torch.ones(B, device="cuda")
        legs[name + ", scores"] = tuple((lambda p=p: ops.ctc_grammar_scores(x, lens, p, canon, False)) for p in (pu, pw))
        legs[name + ", best paths"] = tuple((lambda p=p: ops.ctc_grammar_scores(x, lens, p, canon, True)) for p in (pu, pw))
        legs[name + ", gradient"] = tuple((lambda p=p: ops.ctc_grammar_grad(x, lens_dev(lens), p, which, canon, ones)) for p in (pu, pw))
        legs[name + ", beam K=16"] = tuple((lambda d=d: ops.ctc_grammar_beam_search(x, lens, d, wl, canon, 16, 1)) for d in (du, dw))
    return legs


def lens_dev(lens):
    return torch.tensor(lens, dtype=torch.int32, device="cuda")


def _lm6(al):
    import vistaocr_amd as va
    from tests import beam_data as bd
    with tempfile.TemporaryDirectory() as d:
        path = bd.write_char_arpa(os.path.join(d, "en6.arpa"), [al.idx_to_char[c] for c in range(1, len(al))], order=6, seed=11)
        return va.CharNgramLM.from_arpa(path, al)


def _unweighted_calls(x, lens, canon, sets):
    """label -> (C entry, its argument list) of the twins' unweighted calls, written out argument by argument, and the list of every
    tensor behind a pointer in them - inputs, tables, outputs and a workspace of the size the entry's query answers, allocated here:
    the caller keeps that list alive while the calls are replayed."""
    from vistaocr_amd import _lib, ops
    from vistaocr_amd.grammar import pack_dense_grammars, pack_grammars
    lib, p, st = _lib.load(), ops._p, ops._stream()
    owned = [x, canon]
    ld = lens_dev(lens)
    owned.append(ld)

    def new(*shape, dtype=torch.float32):
        t = torch.zeros(*shape, dtype=dtype, device="cuda")
        owned.append(t)
        return t

    def space(nbytes):
        assert nbytes > 0
        return new((nbytes + 3) // 4), nbytes

    calls = {}
    i32 = torch.int32
    for name, gs in sets.items():
        G = len(gs)
        gp, dp = pack_grammars(gs, "cuda"), pack_dense_grammars(gs, "cuda")
        owned.extend(v for v in list(gp.values()) + list(dp.values()) if torch.is_tensor(v))
        ms, ma = gp["max_states"], gp["max_arcs"]
        tabs = (p(gp["state_off"]), p(gp["arc_off"]), G, p(gp["src"]), p(gp["cls"]), p(gp["dst"]), p(gp["accept"]), ms, ma)
        which = (torch.arange(B, dtype=i32, device="cuda") % G).contiguous()
        owned.append(which)
        for best in (0, 1):
            ws, nb = space(lib.vocr_ctc_grammar_workspace_bytes(T, B, V, G, ms, ma, best))
            outs = (p(new(B, G)),) + ((p(new(B, G)), p(new(B, G, T, dtype=i32)), p(new(B, G, dtype=i32))) if best else (None, None, None))
            calls[name + (", best paths" if best else ", scores")] = ("vocr_ctc_grammar_scores", (p(x), p(ld), T, B, V, p(canon)) + tabs + outs +
                                                                    (T, p(ws), nb, st))
        ws, nb = space(lib.vocr_ctc_grammar_grad_workspace_bytes(T, B, V, G, ms, ma, 1))
        ones = new(B) + 1.0
        owned.append(ones)
        calls[name + ", gradient"] = ("vocr_ctc_grammar_grad", (p(x), p(ld), T, B, V, p(canon)) + tabs +
                                      (p(which), p(ones), p(new(B)), p(new(T, B, V)), p(ws), nb, st))
        ws, nb = space(lib.vocr_ctc_grammar_beam_workspace_bytes(T, B, V, 16, 1))
        calls[name + ", beam K=16"] = ("vocr_ctc_grammar_beam_search", (p(x), p(ld), T, B, V, p(canon), 16, 1, p(dp["state_off"]), p(dp["next"]),
                                                                       p(dp["dist"]), G, p(which), None, None, None, 0, 0, 0.0, 0.0,
                                                                       float("-inf"), p(new(B, 1, T, dtype=i32)), p(new(B, 1, dtype=i32)),
                                                                       p(new(B, 1, 3)), p(ws), nb, st))
    torch.cuda.synchronize()
    return calls, owned


def _replay(records, parent_path, window, rounds, out):
    """the unweighted calls on the parent's library and on the in-tree one, alternating; every pointer in them is to a tensor that
    _unweighted_calls' list keeps alive"""
    from vistaocr_amd import _lib
    new = _lib.load()
    old = ctypes.CDLL(parent_path)
    for name in UNWEIGHTED:
        fn = getattr(old, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    bad = 0
    for label, (name, args) in records.items():
        fns = {"parent": getattr(old, name), "new": getattr(new, name)}
        meds = {"parent": [], "new": []}
        for fn in fns.values():
            for _ in range(20):
                assert fn(*args) == 0
        torch.cuda.synchronize()
        for _ in range(rounds):
            for who in ("parent", "new"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(window):
                    fns[who](*args)
                e1.record()
                e1.synchronize()
                meds[who].append(e0.elapsed_time(e1) / window)
        p, n = float(np.median(meds["parent"])), float(np.median(meds["new"]))
        spread = max(meds["parent"]) - min(meds["parent"])
        ok = n <= p + spread
        bad += not ok
        out("  %-34s parent %8.4f ms (spread %.4f)   new %8.4f ms   %s" % (label, p, spread, n, "within" if ok else "OUTSIDE"))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kinds", default="peaky,dense")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_wgrammar_bench.txt"))
    a = ap.parse_args()
    import vistaocr_amd as va
    from vistaocr_amd import _lib, ops
    from vistaocr_amd.grammar import Grammar, pack_dense_grammars, pack_grammars
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    al = va.english_alphabet()
    canon = torch.as_tensor(al.canonical_indices(), dtype=torch.int32).cuda()
    lens = [T] * B
    out("weighted grammars: T = %d, B = %d, V = %d; ms per call, median [min, max] of %d windows" % (T, B, V, a.repeats))
    bad = 0
    for kind in a.kinds.split(","):
        x = _logits(kind)[0]
        rng = np.random.default_rng(19)
        sets = _grammar_sets(al, rng)
        legs = _legs(x, lens, canon, sets, rng)
        out("\n%s logits - each weighted entry against its unweighted twin" % kind)
        for name, (fu, fw) in legs.items():
            u, w = _windows(fu, 3, a.repeats), _windows(fw, 3, a.repeats)
            out("  %-28s unweighted %8.3f [%.3f, %.3f]   weighted %8.3f [%.3f, %.3f]   x %.3f" % (name, *u, *w, w[0] / u[0]))
        lm = _lm6(al)
        words = sorted({"".join("abcdefghijklmnopqrstuvwxyz"[i] for i in rng.integers(0, 26, size=rng.integers(4, 10))) for _ in range(60)})[:50]
        hot = pack_dense_grammars([Grammar.boost(al, words, 3.0)], "cuda")
        lmd = lm.to("cuda")
        u = _windows(lambda: ops.ctc_beam_search(x, lens, canon, 16, 1, lmd, 0.8, 0.6), 3, a.repeats)
        w = _windows(lambda: ops.ctc_grammar_beam_search(x, lens, hot, None, canon, 16, 1, lmd, 0.8, 0.6, None, 1.0), 3, a.repeats)
        out("  %-28s BeamDecoder + 6-gram %8.3f [%.3f, %.3f]   boost of 50 phrases + 6-gram %8.3f [%.3f, %.3f]   x %.3f"
            % ("boost, beam K=16", *u, *w, w[0] / u[0]))
        if a.parent:
            out("\n%s logits - the unweighted entries, the parent commit's library against this one (windows of %d calls, %d rounds)"
                % (kind, a.window, a.rounds))
            calls, owned = _unweighted_calls(x, lens, canon, sets)
            bad += _replay(calls, a.parent, a.window, a.rounds, out)
            del owned
    # a digit-alphabet trigram as an automaton: V = 11
    from tests import beam_data as bd
    dal = va.Alphabet(["<ctc-blank>"] + ["u%04x" % (0x30 + d) for d in range(10)], left_to_right=True)
    with tempfile.TemporaryDirectory() as d:
        lm3 = va.CharNgramLM.from_arpa(bd.write_char_arpa(os.path.join(d, "d3.arpa"), [dal.idx_to_char[c] for c in range(1, 11)], order=3,
                                                          seed=3), dal)
    g = Grammar.from_ngram(lm3)
    xd = torch.from_numpy(bd.dense_logits(np.random.default_rng(5), T, B, 11)).float().cuda()
    p = pack_grammars([g], "cuda")
    zero = torch.zeros(B, dtype=torch.int32, device="cuda")
    ones = torch.ones(B, device="cuda")
    s = _windows(lambda: ops.ctc_grammar_scores(xd, lens, p, None, False), 3, a.repeats)
    gr = _windows(lambda: ops.ctc_grammar_grad(xd, lens_dev(lens), p, zero, None, ones), 3, a.repeats)
    out("\nfrom_ngram of a digit trigram (%d states + %d arcs), dense logits of V = 11: ln sum_l P(l|x) P_LM(l) %8.3f [%.3f, %.3f] ms, with "
        "the gradient %8.3f [%.3f, %.3f] ms" % (g.n_states, g.n_arcs, *s, *gr))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    _lib.load()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
