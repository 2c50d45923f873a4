"""GPU: vocr_ctc_grammar_scores (vistaocr_amd/csrc/ctc_grammar.hip) through ops.ctc_grammar_scores, GrammarMatcher and
KeywordSpotter.probability, against the fp64 restatement of tests/grammar_ref.py (itself checked against a brute force over all frame
paths in tests/test_grammar_cpu.py).

EVERY entry of out_logp and out_best is compared: -inf exactly where the reference has -inf, never NaN or +inf, finite entries within
    bound = 4 * 2^-24 * ((T + 2) * max(|score|, 1) + T * (D + 2) + (S + E))
of fp64 - a linear worst case for fp32 over the T additions of a path (tests/test_align_gpu.py's eps_line), one lse of at most D + 2
terms per frame (D the automaton's largest in-degree) and the final lse over at most S + E cells; the factor 4 is the allowance the
neighbouring suites give the device's exp / log.  Derived, not measured.  Best paths are checked WITHOUT a tie carve-out, so no pair is
left out: (i) out_best within the bound of the reference's maximum, (ii) the returned labelling is accepted by the automaton, (iii)
ops.ctc_align on that labelling gives a Viterbi score within the bound of out_best.

Each test prints the largest difference and the largest fraction of the bound used (profiles/ctc_grammar_errors.txt keeps a run's
output)."""
import numpy as np
import pytest
import torch

import vistaocr_amd as va
from tests import align_ref as ar
from tests import beam_data as bd
from tests import grammar_ref as gr
from vistaocr_amd import ops
from vistaocr_amd.grammar import Grammar, GrammarMatcher

pytestmark = pytest.mark.gpu

NEG = -np.inf


def bound(T, score, D, N):
    return 4.0 * 2.0 ** -24 * ((T + 2) * np.maximum(np.abs(score), 1.0) + T * (D + 2) + N)


def _pack(automata):
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    cat = lambda k: i32(np.concatenate([np.asarray(a[k], dtype=np.int32) for a in automata]))
    return {"state_off": i32(np.cumsum([0] + [a["S"] for a in automata])), "arc_off": i32(np.cumsum([0] + [len(a["src"]) for a in automata])),
            "src": cat("src"), "cls": cat("cls"), "dst": cat("dst"), "accept": cat("accept"),
            "max_states": max(a["S"] for a in automata), "max_arcs": max(len(a["src"]) for a in automata)}


def _run(x, lens, automata, canon=None, want_best=True, max_states=None, max_arcs=None):
    """Host (logp [B,G], best [B,G], labels [B,G,T], label_lens [B,G]) and the device tensors."""
    gp = _pack(automata)
    if max_states is not None:
        gp["max_states"], gp["max_arcs"] = max_states, max_arcs
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda() if canon is not None else None
    out = ops.ctc_grammar_scores(xd, lens, gp, cd, want_best)
    torch.cuda.synchronize()
    return [None if o is None else o.cpu().numpy() for o in out], (xd, cd, out)


def _check(name, x, lens, automata, canon=None, max_states=None, max_arcs=None, need_finite=1):
    """Both scores of every (line, automaton) against the reference, and the best paths by (ii) and (iii).  Returns (got, ref)."""
    T, B, V = x.shape
    cls = ar.classes_of(V, canon)
    (logp, best, labels, ln), (xd, cd, dev) = _run(x, lens, automata, canon, True, max_states, max_arcs)
    ref = gr.search(x, lens, automata, canon, max_states, max_arcs)
    D = np.array([gr.max_in_degree(a) for a in automata])[None, :]
    Tb = np.clip(np.asarray([int(v) for v in lens]), 0, T)[:, None]      # a line's own frame count
    N = np.array([a["S"] + len(a["src"]) for a in automata])[None, :]
    worst, frac, finite = 0.0, 0.0, 0
    for what, g, r in (("logp", logp, ref["logp"]), ("best", best, ref["best"])):
        assert not np.isnan(g).any() and not np.any(g == np.inf), (name, what)
        assert np.array_equal(g == NEG, r == NEG), (name, what, np.argwhere((g == NEG) != (r == NEG))[:5].tolist())
        fin = r != NEG
        finite += int(fin.sum())
        if fin.any():
            d = np.abs(g.astype(np.float64) - np.where(fin, r, 0.0))[fin]
            bnd = np.broadcast_to(bound(Tb, np.where(fin, r, 0.0), D, N), r.shape)[fin]
            worst, frac = max(worst, float(d.max())), max(frac, float((d / bnd).max()))
    dead = ref["best"] == NEG
    assert np.all(ln[dead] == -1) and np.all(ln[~dead] >= 0), name
    for b, g in np.argwhere(~dead):
        assert gr.accepts(automata[g], labels[b, g, :ln[b, g]], cls), (name, int(b), int(g), labels[b, g, :ln[b, g]].tolist())
        assert np.all(labels[b, g, ln[b, g]:] == 0)
    vit = ops.ctc_align(xd, lens, dev[2], dev[3], cd)[0][..., 0].cpu().numpy()
    afrac = 0.0
    if (~dead).any():
        d = np.abs(vit.astype(np.float64)[~dead] - best.astype(np.float64)[~dead])
        afrac = float((d / np.broadcast_to(bound(Tb, np.where(dead, 0.0, ref["best"]), D, N), dead.shape)[~dead]).max())
    print("%s: %d pairs, %d finite scores, largest |fp32 - fp64| %.3g, largest fraction of the bound %.3f; %d best paths accepted, "
          "aligned Viterbi score within %.3f of the bound" % (name, dead.size, finite, worst, frac, int((~dead).sum()), afrac))
    assert frac <= 1.0, (name, worst, frac)
    assert afrac <= 1.0, (name, afrac)
    assert finite >= need_finite, (name, finite)
    return (logp, best, labels, ln), ref


def _sigma_star(V, cls=None):
    kinds = sorted({int(c) for c in (cls if cls is not None else np.arange(V))[1:] if c != 0})
    return gr.make(1, [(0, c, 0) for c in kinds], [0])


def _string(labels):
    return gr.make(len(labels) + 1, [(i, c, i + 1) for i, c in enumerate(labels)], [len(labels)])


def _random_dfa(rng, V, S, p, cls=None):
    cls = np.arange(V) if cls is None else cls
    kinds = sorted({int(c) for c in cls[1:] if c != 0})
    arcs = [(s, c, int(rng.integers(0, S))) for s in range(S) for c in kinds if rng.random() < p]
    return gr.make(S, arcs, [s for s in range(S) if rng.random() < 0.4] or [S - 1], V=V)


def _tree(V, N):
    """A deterministic two-level tree of exactly N = S + E cells (the leaves and the inner states accept; an odd cell is one unreachable
    state): in-degree 1 everywhere."""
    n, extra = divmod(N - (2 * V - 1), 2)
    assert 0 <= n <= (V - 1) ** 2
    arcs = [(0, c, c) for c in range(1, V)]
    for i in range(n):
        arcs.append((1 + i // (V - 1), 1 + i % (V - 1), V + i))
    a = gr.make(V + n + extra, arcs, range(1, V + n), V=V)
    assert a["S"] + len(a["src"]) == N
    return a


def _hub(rng, V, D, cells=None, sinks=0):
    """A deterministic automaton with one state of in-degree exactly D: a two-level tree whose D leaves all lead into the hub, on classes
    drawn at random (so its incoming arcs form groups of several arcs per class); the hub has a self loop (an incoming arc of the class it
    leaves on: the exclusion), arcs to an accepting state and one back.  `cells`: further leaves until S + E is `cells` or one below it;
    the first 64 * `sinks` of them lead, 64 each, into accepting states of their own (in-degree exactly 64), the rest are dead ends."""
    n = max(D - 1, 1) if cells is None else (cells - (2 * V + D + 4) - 65 * sinks) // 2
    assert max(D - 1, 1) + 64 * sinks <= n <= (V - 1) ** 2
    arcs = [(0, c, c) for c in range(1, V)]
    leaves = [V + i for i in range(n)]
    for i in range(n):
        arcs.append((1 + i // (V - 1), 1 + i % (V - 1), leaves[i]))
    hub, fin = V + n, V + n + 1
    arcs += [(s, int(rng.integers(1, V)), hub) for s in leaves[:D - 1]]
    arcs += [(hub, 1, hub)] if D > 1 else []
    arcs += [(hub, 2, fin), (hub, 3, fin), (fin, 1, fin)] + ([(fin, 2, hub)] if D == 1 else [])
    rest = leaves[max(D - 1, 0):]
    for j in range(sinks):
        arcs += [(s, int(rng.integers(1, V)), fin + 1 + j) for s in rest[64 * j:64 * j + 64]]
    a = gr.make(fin + 1 + sinks, arcs, [fin, 1] + [fin + 1 + j for j in range(sinks)], V=V)
    if D > 1:
        assert np.bincount(a["dst"])[hub] == D, (np.bincount(a["dst"])[hub], D)
    return a


@pytest.mark.parametrize("T", [1, 2, 3, 17])
def test_small_shapes(T):
    """lens of 0, 1 and < T in one batch; Sigma*, a string with a doubled letter, a state with two incoming arcs of one class (and an arc
    leaving it on that class: the exclusion), a non-accepting and an accepting start; dense lines."""
    V = 7
    rng = np.random.default_rng(T)
    x = bd.dense_logits(rng, T, 4, V, sigma=2.0)
    lens = [T, 0, 1, max(T - 1, 1)]
    twin = gr.make(4, [(0, 1, 1), (0, 2, 2), (1, 3, 3), (2, 3, 3), (3, 3, 0), (3, 1, 3), (3, 4, 1)], [3], V=V)
    automata = [_sigma_star(V), _string([1, 1, 2]), twin, _random_dfa(rng, V, 5, 0.6), gr.make(2, [(0, 1, 1)], [0, 1], V=V)]
    _check("T = %d" % T, x, lens, automata, need_finite=8)


def test_alphabet_sizes_and_classes():
    """V = 2 (one symbol); V = 256 with canon = NULL (a state of 255 incoming arcs) and with a two-member class."""
    rng = np.random.default_rng(11)
    x = bd.dense_logits(rng, 9, 3, 2, sigma=1.0)
    _check("V = 2", x, [9, 4, 1], [_sigma_star(2), _string([1]), _string([1, 1])], need_finite=12)
    V = 256
    x = bd.dense_logits(rng, 6, 2, V, sigma=2.0)
    _check("V = 256, canon NULL", x, [6, 5], [_sigma_star(V), _random_dfa(rng, V, 4, 0.5), _string([255, 255, 1])], need_finite=10)
    canon = np.arange(V)
    canon[200], canon[9] = 7, 3                                          # {7, 200} and {3, 9} are one class each
    cls = ar.classes_of(V, canon)
    automata = [_sigma_star(V, cls), _random_dfa(rng, V, 4, 0.5, cls), gr.make(3, [(0, 200, 1), (1, 3, 2)], [2], V=V, canon=canon)]
    (logp, best, labels, ln), _ = _check("V = 256, two-member classes", x, [6, 5], automata, canon=canon, need_finite=10)
    assert labels[0, 2, :2].tolist() == [7, 3]                            # the labelling comes back as canonical columns


def test_minus_infinity_logits():
    """Peaky lines (all but two columns of a frame -inf), a frame that is all -inf, a line whose blank is impossible everywhere."""
    T, V = 17, 9
    rng = np.random.default_rng(21)
    x = np.concatenate([bd.peaky_logits(rng, T, 3, V, p_char=0.6, p_alt=1.0, cost=(1.0, 4.0)), bd.dense_logits(rng, T, 2, V, 2.0)], axis=1)
    x[5, 3, :] = NEG
    x[:, 4, 0] = NEG
    greedy = ar.greedy_labels(x[:, 0], T)
    automata = [_sigma_star(V), _string(greedy), _string(greedy[:2]), _random_dfa(rng, V, 6, 0.7), _random_dfa(rng, V, 3, 0.9)]
    (logp, _, _, _), ref = _check("-inf logits", x, [T, T, 12, T, T], automata, need_finite=12)
    assert np.all(logp[3] == NEG) and np.isfinite(logp[0, 1])


def test_in_degrees_across_the_lane_wave_seam():
    """Hubs of in-degree 1, 63, 64, 65 and 300 in ONE call (very different sizes, results at the caller's index): a state with fewer than
    64 incoming arcs is scanned by a lane, one with more by its wave, 64 arcs at a time."""
    T, V = 8, 20
    rng = np.random.default_rng(31)
    x = bd.dense_logits(rng, T, 3, V, sigma=1.5)
    automata = [_hub(rng, V, D) for D in (64, 1, 300, 63, 65)]
    assert [gr.max_in_degree(a) for a in automata] == [64, 3, 300, 63, 65]
    got, ref = _check("in-degrees 64, 1, 300, 63, 65", x, [T, T - 1, 5], automata, need_finite=24)
    again, _ = _run(x, [T, T - 1, 5], automata[::-1])                      # the reversed list: the reversed columns, bit for bit
    assert all(np.array_equal(g, a[:, ::-1]) for g, a in zip(got, again))


@pytest.mark.parametrize("N,D,sinks", [(2100, 65, 3), (2100, 300, 3), (5000, 130, 20), (8192, 65, 20), (8192, 700, 20)])
def test_wave_scanned_states_in_large_automata(N, D, sinks):
    """A hub of 64 or more incoming arcs inside an automaton of more than 2048 cells: the workgroup has 1024 threads, so the wave-scanned
    states (the hub and 3 or 20 states of in-degree 64: fewer and more than the waves) are dealt over 16 waves; at 8192 cells the plan no longer fits the LDS beside the rows and is read from global memory (at 2100
    and 5000 it is staged)."""
    V, T = 96, 7
    rng = np.random.default_rng(N + D)
    x = bd.dense_logits(rng, T, 2, V, sigma=1.0)
    a = _hub(rng, V, D, cells=N, sinks=sinks)
    assert N - 1 <= a["S"] + len(a["src"]) <= N and gr.max_in_degree(a) == D
    _check("S + E = %d with a hub of in-degree %d" % (a["S"] + len(a["src"]), D), x, [T, 5], [a, _hub(rng, V, 64)], need_finite=8)


@pytest.mark.parametrize("N", [255, 256, 257, 2047, 2048, 2049, 8191, 8192])
def test_cell_counts_around_a_workgroup_pass(N):
    """S + E just below, at and above one pass of 256 threads, around the size from which a workgroup has 1024 threads, and at the
    supported maximum."""
    V = 16 if N < 1000 else 96
    T = 5
    rng = np.random.default_rng(N)
    x = bd.dense_logits(rng, T, 2, V, sigma=1.0)
    _check("S + E = %d" % N, x, [T, 3], [_tree(V, N)], need_finite=4)


BREAKS = ["no state", "too many states", "too many arcs", "src out of range", "dst out of range", "cls 0", "cls V", "blank's class", "order"]


@pytest.mark.parametrize("kind", BREAKS)
def test_an_invalid_automaton_poisons_only_its_own_column(kind):
    T, V = 6, 8
    rng = np.random.default_rng(41)
    x = bd.dense_logits(rng, T, 3, V, sigma=1.5)
    canon = np.arange(V)
    canon[6] = 0                                                          # column 6 is in the blank's class
    good = [_string([1, 2]), _random_dfa(rng, 6, 4, 0.6)]
    ms, ma = max(a["S"] for a in good), max(len(a["src"]) for a in good)
    arcs = [(0, 1, 1), (1, 2, 2), (2, 3, 0)]
    bad = gr.make(3, arcs, [2])
    if kind == "no state":
        bad = {"S": 0, "src": np.zeros(0, np.int32), "cls": np.zeros(0, np.int32), "dst": np.zeros(0, np.int32), "accept": np.zeros(0, np.int32)}
    elif kind == "too many states":
        bad = _string([1] * ms)
    elif kind == "too many arcs":
        bad = gr.make(ms, [(s, c, (s + 1) % ms) for s in range(ms) for c in (1, 2, 3, 4, 5, 7)][:ma + 1], [1])
        assert len(bad["src"]) == ma + 1 and bad["S"] <= ms
    elif kind == "src out of range":
        bad["src"][1] = 3
    elif kind == "dst out of range":
        bad["dst"][2] = -1
    elif kind == "cls 0":
        bad["cls"][0] = 0
    elif kind == "cls V":
        bad["cls"][0] = V
    elif kind == "blank's class":
        bad["cls"][0] = 6
    elif kind == "order":
        bad = dict(bad, src=bad["src"][::-1].copy(), cls=bad["cls"][::-1].copy(), dst=bad["dst"][::-1].copy())
    automata = [good[0], bad, good[1]]
    (logp, best, labels, ln), ref = _check(kind, x, [T, 4, 0], automata, canon=canon, max_states=ms, max_arcs=ma, need_finite=4)
    assert np.all(logp[:, 1] == NEG) and np.all(best[:, 1] == NEG) and np.all(ln[:, 1] == -1)
    assert np.all(np.isfinite(logp[:2, 0]))


def test_scores_only_and_repeat_give_the_same_bits():
    T, V = 17, 12
    rng = np.random.default_rng(51)
    x = bd.dense_logits(rng, T, 3, V, sigma=2.0)
    automata = [_hub(rng, V, 70), _sigma_star(V), _tree(V, 101), _random_dfa(rng, V, 9, 0.5)]
    a, _ = _run(x, [T, 9, 2], automata)
    b, _ = _run(x, [T, 9, 2], automata)
    c, _ = _run(x, [T, 9, 2], automata, want_best=False)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert c[1] is None and c[2] is None and c[3] is None and np.array_equal(a[0].view(np.int32), c[0].view(np.int32))


def _planted(rng, al, T, texts, peaky):
    """[T, B, V] lines that spell `texts` (one frame per character, two blanks between): dense N(0, 1) logits with the planted path
    raised by 14 (peaky) or by 3 (dense: every reading keeps a real share)."""
    V = len(al)
    x = rng.normal(0, 1, (T, len(texts), V)).astype(np.float32)
    for b, text in enumerate(texts):
        path = [0, 0]
        for ch in text:
            path += [al.char_to_idx["u%04x" % ord(ch)], 0, 0]
        path = (path + [0] * T)[:T]
        x[np.arange(T), b, path] += 14.0 if peaky else 3.0
    return x


WORDS = None


def _words(rng):
    global WORDS
    if WORDS is None:
        letters = "abcdefghijklmnopqrstuvwxyz"
        WORDS = sorted({"".join(rng.choice(list(letters), int(rng.integers(3, 9)))) for _ in range(199)} | {"invoice"})
    return WORDS


@pytest.mark.parametrize("kind", ["peaky", "dense"])
def test_configs1_shape(kind):
    """T = 294, B = 4, V = 96; contains "the", a date, a 200-word trie and Sigma* on lines that spell a sentence with "the", a date, a
    word of the trie and noise."""
    al = va.english_alphabet()
    T, V = 294, len(al)
    assert V == 96
    rng = np.random.default_rng(61)
    words = _words(np.random.default_rng(62))
    grammars = [Grammar.contains(al, "the"), Grammar.from_regex(al, "\\d{1,2}/\\d{1,2}/\\d{4}"), Grammar.from_words(al, words),
                Grammar.from_regex(al, ".*")]
    x = _planted(rng, al, T, ["pay the sum of 12 pounds to the bearer", "3/11/2024", "invoice", ""], kind == "peaky")
    canon = al.canonical_indices()
    automata = [gr.from_grammar(g) for g in grammars]
    (logp, best, labels, ln), ref = _check("configs[1] shape, %s" % kind, x, [T, 60, 40, T], automata, canon=canon, need_finite=10)
    if kind == "peaky":
        assert logp[0, 0] > -0.2 and logp[1, 1] > -0.2 and logp[2, 2] > -0.2
        hits = GrammarMatcher(al).match(torch.from_numpy(x).cuda(), [T, 60, 40, T], grammars)
        assert hits.best_text[1][1] == "3/11/2024" and hits.best_text[2][2] == "invoice" and "the" in hits.best_text[0][0]
        assert np.array_equal(hits.logp, logp) and np.array_equal(hits.best_logp, best)


def test_identities():
    """Sigma*: ln P = 0 and best = the sum of the frames' maxima; a single string: both of ops.ctc_align's scores and its labels; a
    language and its complement sum to 1; a trie sums its words' CTC scores."""
    al = va.english_alphabet()
    T, V = 40, len(al)
    rng = np.random.default_rng(71)
    x = _planted(rng, al, T, ["cat", "a cart", "dog"], False)
    lens = [T, 30, 12]
    canon = al.canonical_indices()
    xd, cd = torch.from_numpy(x).cuda(), torch.as_tensor(canon, dtype=torch.int32).cuda()
    words = ["cat", "cart", "dog", "do", "tree"]
    trie, single = Grammar.from_words(al, words), Grammar.from_words(al, ["cart"])
    trans, accept = trie.dfa()
    kinds = sorted({c for c in canon[1:] if c != 0})
    sink = len(trans)
    comp = Grammar.from_dfa(al, [{c: row.get(c, sink) for c in kinds} for row in trans] + [{c: sink for c in kinds}],
                            [not a for a in accept] + [True])
    star = Grammar.from_regex(al, ".*")
    grammars = [star, single, trie, comp]
    automata = [gr.from_grammar(g) for g in grammars]
    (logp, best, labels, ln), ref = _check("identities", x, lens, automata, canon=canon, need_finite=24)
    D = [g.max_in_degree for g in grammars]
    N = [g.n_states + g.n_arcs for g in grammars]
    lab = np.zeros((3, len(words), 8), dtype=np.int32)
    wl = np.zeros((3, len(words)), dtype=np.int32)
    for i, w in enumerate(words):
        lab[:, i, :len(w)] = [al.char_to_idx["u%04x" % ord(ch)] for ch in w]
        wl[:, i] = len(w)
    sc = ops.ctc_align(xd, lens, torch.from_numpy(lab).cuda(), torch.from_numpy(wl).cuda(), cd)[0].cpu().numpy().astype(np.float64)
    for b in range(3):
        n = lens[b]
        clp, _ = ar.class_logprobs(x[:n, b].astype(np.float64), canon)
        top = float(clp.max(axis=1).sum())
        assert abs(logp[b, 0]) <= bound(T, 0.0, D[0], N[0]) and abs(best[b, 0] - top) <= bound(T, top, D[0], N[0])
        assert abs(logp[b, 1] - sc[b, 1, 1]) <= bound(T, sc[b, 1, 1], D[1], N[1])
        assert abs(best[b, 1] - sc[b, 1, 0]) <= bound(T, sc[b, 1, 0], D[1], N[1])
        assert labels[b, 1, :ln[b, 1]].tolist() == lab[b, 1, :4].tolist()
        p, q = np.exp(float(logp[b, 2])), np.exp(float(logp[b, 3]))
        tol = p * bound(T, logp[b, 2], D[2], N[2]) + q * bound(T, logp[b, 3], D[3], N[3])
        assert abs(p + q - 1.0) <= 1.5 * tol, (b, p, q, tol)             # e^x - 1 <= 1.5 x for the small x of a bound
        total = float(np.exp(sc[b, :, 1]).sum())
        tol = p * bound(T, logp[b, 2], D[2], N[2]) + float((np.exp(sc[b, :, 1]) * 4.0 * (T + 2) * 2.0 ** -24 * np.maximum(np.abs(sc[b, :, 1]), 1.0)).sum())
        assert abs(p - total) <= 1.5 * tol, (b, p, total, tol)
    print("identities: Sigma*, single string against ctc_align, complement, trie sum: within the bound")


def test_keyword_probability():
    """KeywordSpotter.probability <= min(1, expected count) everywhere; equal to the expected count for a keyword of pairwise distinct
    characters on lines of at most 2L - 1 frames, where two occurrences cannot fit; the whole-word variant against the reference built
    from the same grammar."""
    al = va.english_alphabet()
    canon = al.canonical_indices()
    rng = np.random.default_rng(81)
    T = 30
    x = _planted(rng, al, T, ["the cat", "at the", "other", "ttt"], False)
    lens = [T, 20, 25, 9]
    xd = torch.from_numpy(x).cuda()
    kws = ["the", "t", "at", "tt", "he"]
    for whole in (False, True):
        sp = va.KeywordSpotter(al, whole_word=whole)
        prob = sp.probability(xd, lens, kws)
        count = sp.search(xd, lens, kws).expected_count
        ref = gr.search(x, lens, [gr.from_grammar(Grammar.contains(al, k, whole_word=whole)) for k in kws], canon)
        grams = [Grammar.contains(al, k, whole_word=whole) for k in kws]
        b_p = np.stack([[bound(T, ref["logp"][b, q], g.max_in_degree, g.n_states + g.n_arcs) for q, g in enumerate(grams)] for b in range(4)])
        b_c = 4.0 * (T + 2) * 2.0 ** -24 * np.maximum(np.abs(np.log(count)), 1.0)       # the keyword search's own bound
        assert np.all(np.abs(np.log(prob) - ref["logp"]) <= b_p), whole
        assert np.all(prob <= np.minimum(1.0, count * (1 + 1.5 * b_c)) * (1 + 1.5 * b_p)), (whole, prob, count)
        print("keyword probability (whole_word=%s): largest P / min(1, E) = %.6f" % (whole, float((prob / np.minimum(1.0, count)).max())))
    T = 5                                                                 # L = 3: two occurrences need six frames
    x = _planted(rng, al, T, ["", "", ""], False)
    x[[0, 1, 2], 0, [al.char_to_idx["u0074"], al.char_to_idx["u0068"], al.char_to_idx["u0065"]]] += 4.0
    lens = [5, 4, 3]
    xd = torch.from_numpy(x).cuda()
    sp = va.KeywordSpotter(al)
    prob, hits = sp.probability(xd, lens, ["the"]), sp.search(xd, lens, ["the"])
    g = Grammar.contains(al, "the")
    tol = bound(T, np.log(prob), g.max_in_degree, g.n_states + g.n_arcs) + 4.0 * (T + 2) * 2.0 ** -24 * np.maximum(np.abs(hits.log_count), 1.0)
    assert np.all(np.abs(np.log(prob) - hits.log_count) <= tol), (prob, hits.expected_count)
    print("keyword probability = expected count at T <= 2L - 1: largest |ln P - ln E| %.3g" % float(np.abs(np.log(prob) - hits.log_count).max()))
