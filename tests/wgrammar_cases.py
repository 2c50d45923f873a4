"""Pinned inputs and bars of the weighted grammars' tests (tests/test_wgrammar_cpu.py, tests/test_wgrammar_gpu.py,
tests/test_wgrammar_guarded_gpu.py) and their fp64 references (tests/wgrammar_ref.py).  Test helper only.  References are computed once
per process and shared; the CPU test holds them to brute force, to central differences and to their floors of decided lines, the GPU
tests compare the kernels with the same objects.

THE SWEEP SCORES' BOUND.  tests/test_grammar_gpu.py derives, for the unweighted sweep,
    4 * 2^-24 * ((T + 2) * max(|score|, 1) + T * (D + 2) + N):
a linear worst case for fp32 over the T additions of a path (each a rounding of a value no larger than the score), one lse of at most
D + 2 terms per frame and the final lse over N cells, times the allowance of 4 for the device's exp / log.  A weight adds ONE more
addition - one more rounding - per frame to a path (an arc is entered at most once per frame), and the final weight one at the end; and
the values that are rounded are no longer bounded by |score| alone but by |score| plus the weight the path has accumulated, at most
W = T * max |w_a| + max |f_s|.  So
    bound = 4 * 2^-24 * ((2 T + 3) * (max(|score|, 1) + W) + T * (D + 2) + N).
Derived, not measured.

GRADIENTS AND BEAM SCORES follow the project's rule: 4 x the largest error measured on the MI355X against fp64, rounded up to one
digit (RECORDED, profiles/ctc_wgrammar_errors.txt), never above the beam suites' ceiling of 1e-3.  One cap does not depend on the code
under test: on each family the weighted entry's error stays within 10 x what the existing unweighted entry shows on the same logits
and automaton (tests/test_wgrammar_gpu.py measures both in the same test)."""
import collections
import functools
import math
import os
import tempfile

import numpy as np

import vistaocr_amd as va
from tests import beam_cases as bc
from tests import beam_data as bd
from tests import grammar_beam_cases as gc
from tests import grammar_ref as gr
from tests import wgrammar_ref as wr
from vistaocr_amd.grammar import Grammar

NEG = -np.inf
TAU = bc.TAU
CEILING = bc.CEILING
U = 2.0 ** -24


def bound(T, score, D, N, W):
    return 4.0 * U * ((2 * T + 3) * (np.maximum(np.abs(score), 1.0) + W) + T * (D + 2) + N)


def one_digit_up(x):
    """x rounded up to one significant digit"""
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


# family: the largest (score error, gradient error) of vocr_ctc_grammar_grad_weighted against fp64 on the MI355X, in the units of
# tests/test_grammar_grad_gpu.py (|ln Z - ref| / max(|ref|, 1); per line max |g - ref| / the line's largest |ref|):
# profiles/ctc_wgrammar_errors.txt
GRAD_RECORDED = {
    "tiny": (7.7e-08, 6.6e-07),
    "degree": (1.3e-07, 2.4e-06),
    "threads": (4.3e-08, 3.5e-06),
    "stage": (1.1e-07, 6.7e-06),
    "max": (2.8e-08, 3.7e-06),
    "slack": (6.1e-07, 4.9e-06),
    "surface": (1.6e-07, 5.2e-06),
}

# group: the largest |score - fp64| of (total, acoustic, lm, grammar) of vocr_ctc_grammar_beam_search_weighted on the MI355X
# (profiles/ctc_wgrammar_errors.txt).  A 0 is a column that is exact there: no LM, or weights that are multiples of 1/8.
BEAM_RECORDED = {
    "ngram": (3.85e-06, 2.82e-06, 0.00e+00, 2.50e-06),
    "brute": (3.36e-07, 3.36e-07, 0.00e+00, 0.00e+00),
    "dense": (6.29e-06, 7.05e-06, 0.00e+00, 2.98e-08),
    "dense_lm": (5.39e-06, 4.37e-06, 2.37e-06, 0.00e+00),
    "boost": (4.04e-07, 4.04e-07, 7.46e-07, 2.98e-08),
    "trie": (1.22e-05, 1.13e-05, 1.89e-06, 0.00e+00),
    "guarded": (1.06e-05, 8.88e-06, 2.22e-06, 0.00e+00),
}


def bars(recorded):
    """4 x the recorded maxima, rounded up to one digit, never above the ceiling"""
    return tuple(min(one_digit_up(4.0 * r), CEILING) for r in recorded)


def letters(V):
    return gc.letters(V)


def random_weights(rng, a, lo=-2.0, hi=2.0):
    """tests/grammar_ref.py's automaton with weights drawn from [lo, hi], stored as the float32 values the kernel gets"""
    w = rng.uniform(lo, hi, len(a["src"])).astype(np.float32).astype(np.float64)
    fw = rng.uniform(lo, hi, a["S"]).astype(np.float32).astype(np.float64)
    return wr.weighted(a, w, fw)


# ---- the tiny case: V = 4 columns of which 2 and 3 are one class, T = 5; a self loop (1 -2-> 1, and 2 -3-> 2 through the merged
# column), an arc into the start state (1 -1-> 0), a non-deterministic pair (0 -1-> 1 and 0 -1-> 2), an accepting start
TINY_CANON = [0, 1, 2, 2]
TINY_LENS = [5, 0, 1, 5]


@functools.lru_cache(maxsize=None)
def tiny_automaton():
    a = gr.make(3, [(0, 1, 1), (0, 1, 2), (1, 2, 1), (1, 1, 0), (2, 3, 2), (2, 1, 1), (0, 2, 2)], [0, 2], V=4, canon=TINY_CANON)
    return random_weights(np.random.default_rng(501), a)


@functools.lru_cache(maxsize=None)
def tiny_logits():
    return np.random.default_rng(502).normal(0, 2, size=(5, 4, 4)).astype(np.float32).astype(np.float64)


# ---- the sweeps' seams.  The host plan (plan_for in csrc/ctc_grammar.hip): 256 threads up to 2048 cells, 1024 beyond; the plan is
# staged in LDS while rows + plan fit 147 KiB, and the weights behind it while they fit too.
LDS_DYN_MAX = 160 * 1024 - 13 * 1024


def _align16(n):
    return (n + 15) & ~15


def staging(max_states, max_arcs):
    """0: nothing staged, 1: the plan, 3: the plan and the weights - the host plan's rule restated"""
    lds = (4 * (max_states + max_arcs) + 2 * 256) * 4
    plan = _align16(16 * max_arcs + 8 * max_states + 4 * (max_arcs // 64 + 2))
    if lds + plan > LDS_DYN_MAX:
        return 0
    return 3 if max_arcs > 0 and lds + plan + _align16(4 * max_arcs) <= LDS_DYN_MAX else 1


TREE_V = 96


def tree(N):
    from tests.test_grammar_gpu import _tree
    return _tree(TREE_V, N)


def tree_sizes(N):
    n, extra = divmod(N - (2 * TREE_V - 1), 2)
    return TREE_V + n + extra, TREE_V - 1 + n


@functools.lru_cache(maxsize=None)
def stage_seams():
    """(the largest tree whose plan AND weights are staged, the largest whose plan is): N with staging 3 / 1 and N + 1 without"""
    last = {}
    for N in range(2100, 8193):
        last[staging(*tree_sizes(N))] = N
    assert staging(*tree_sizes(last[3] + 1)) == 1 and staging(*tree_sizes(last[1] + 1)) == 0
    return last[3], last[1]


Sweep = collections.namedtuple("Sweep", "family x lens automata canon max_states max_arcs")


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    """name -> Sweep.  T = 12; the lens hold a full line, a shorter one and (where B = 3) a very short one."""
    from tests.test_grammar_gpu import _hub
    T = 12
    if name.startswith("degree"):
        D = int(name[6:])
        rng = np.random.default_rng(600 + D)
        a = random_weights(rng, _hub(rng, 20, D))
        assert gr.max_in_degree(a) == D
        return Sweep("degree", bd.dense_logits(rng, T, 3, 20, sigma=1.5), [12, 11, 5], [a], None, None, None)
    if name.startswith("cells"):
        N = int(name[5:])
        rng = np.random.default_rng(700 + N)
        a = random_weights(rng, tree(N))
        s3, s1 = stage_seams()
        family = "threads" if N in (2048, 2049) else "max" if N == 8192 else "stage"
        assert family != "stage" or N in (s3, s3 + 1, s1, s1 + 1), (N, s3, s1)
        return Sweep(family, bd.dense_logits(rng, T, 2, TREE_V, sigma=1.0), [12, 7], [a], None, None, None)
    assert name == "slack"
    rng = np.random.default_rng(800)
    V = 9
    canon = [0, 1, 1, 3, 4, 4, 4, 7, 8]
    from tests.test_grammar_gpu import _random_dfa
    from tests.align_ref import classes_of
    cls = classes_of(V, canon)
    automata = [random_weights(rng, _random_dfa(rng, V, S, 0.7, cls)) for S in (5, 2, 9)]
    ms, ma = max(a["S"] for a in automata) + 7, max(len(a["src"]) for a in automata) + 13
    return Sweep("slack", bd.dense_logits(rng, T, 4, V, sigma=2.0), [12, 12, 3, 9], automata, canon, ms, ma)


def sweep_names():
    s3, s1 = stage_seams()
    return (["degree%d" % D for D in (63, 64, 65, 130)] + ["cells%d" % N for N in (2048, 2049, s3, s3 + 1, s1, s1 + 1, 8192)] + ["slack"])


# ---- the beam search
def unit_weights(rng, n, lo=-2.0, hi=2.0):
    """n weights that are multiples of 1/8: every sum of them is exact in float32 and float64"""
    return (rng.integers(int(lo * 8), int(hi * 8) + 1, size=n) / 8.0).tolist()


@functools.lru_cache(maxsize=None)
def field_ngram():
    """gc.field_lm()'s trigram as a weighted automaton"""
    return Grammar.from_ngram(gc.field_lm())


@functools.lru_cache(maxsize=None)
def lm6():
    """a character 6-gram over the English alphabet"""
    al, _ = bc.english()
    with tempfile.TemporaryDirectory() as d:
        units = [al.idx_to_char[c] for c in range(1, len(al))]
        path = bd.write_char_arpa(os.path.join(d, "en6.arpa"), units, order=6, seed=11)
        return va.CharNgramLM.from_arpa(path, al)


@functools.lru_cache(maxsize=None)
def field_words():
    """a weighted lexicon over the field alphabet: 40 words of digits, '-' and 'a', weights in eighths"""
    rng = np.random.default_rng(901)
    abc = "0123456789-a"
    words = sorted({"".join(abc[i] for i in rng.integers(0, 12, size=rng.integers(1, 6))) for _ in range(40)})
    return Grammar.from_words(gc.field_alphabet(), words, unit_weights(rng, len(words), -3.0, 0.0)), words


@functools.lru_cache(maxsize=None)
def field_boost():
    return Grammar.boost(gc.field_alphabet(), ["12", "2-2", "a", "1"], [1.5, 2.0, -0.75, 0.25])


@functools.lru_cache(maxsize=None)
def tiny_boost():
    """over blank + 3 letters: overlapping phrases, a phrase inside a phrase, a repeated symbol"""
    return Grammar.boost(letters(4), ["ab", "ba", "aba", "aa", "c"], [1.0, -0.5, 0.75, 1.25, 0.125])


@functools.lru_cache(maxsize=None)
def big_weighted_trie():
    """gc.big_trie()'s 3000 words with weights: beyond the sweep kernels' 8192 cells"""
    al, _ = bc.english()
    _, words = gc.big_trie()
    g = Grammar.from_words(al, words, unit_weights(np.random.default_rng(902), len(words), -4.0, 0.0))
    assert g.n_states + g.n_arcs > 8192
    return g


BOOST_PHRASE = "qvx"


@functools.lru_cache(maxsize=None)
def boost_line():
    """[T = 12, 1, V] English logits that read `qzx` with `qvx` a close second (z over v by 1.0 at its frames), and the boost of
    `qvx` by 3"""
    al, canon = bc.english()
    V = len(canon)
    x = np.random.default_rng(903).normal(0, 0.3, size=(12, 1, V))
    ix = lambda ch: al.char_to_idx["u%04x" % ord(ch)]
    for t, ch in ((1, "q"), (2, "q"), (5, "z"), (6, "z"), (9, "x"), (10, "x")):
        x[t, 0, ix(ch)] += 9.0
    for t in (5, 6):
        x[t, 0, ix("v")] += 8.5
    for t in (0, 3, 4, 7, 8, 11):
        x[t, 0, 0] += 9.0
    return x.astype(np.float32).astype(np.float64), Grammar.boost(al, [BOOST_PHRASE, "zebra"], 3.0)


Beam = collections.namedtuple("Beam", "group x lens K nbest grammars which canon gw lm alpha beta")


@functools.lru_cache(maxsize=None)
def beam_case(name):
    if name.startswith("ngram_K"):                                  # from_ngram under the weighted search, no LM; T = 12, B = 8
        K = int(name[7:])
        seed = {4: 1004, 16: 1053, 128: 1276}[K]                    # seeds whose eight lines the restatement decides by more than TAU
        x = bd.dense_logits(np.random.default_rng(seed), 12, 8, 13)
        return Beam("ngram", x, [12] * 8, K, min(K, 4), [field_ngram()], None, None, 0.8, None, 0.0, 0.6)
    if name == "brute":                                             # T = 4, V = 4: 121 prefixes at most, the beam of 128 holds them all
        x = np.random.default_rng(1100).normal(0, 2, size=(4, 4, 4)).astype(np.float32).astype(np.float64)
        return Beam("brute", x, [4, 4, 3, 1], 128, 8, [tiny_boost()], None, None, 1.0, None, 0.0, 0.0)
    if name in ("dense", "dense_lm"):
        with_lm = name == "dense_lm"
        x = bd.dense_logits(np.random.default_rng(1200 + with_lm), 12, 8, 13)
        lm, alpha, beta = (gc.field_lm(), 0.8, 0.6) if with_lm else (None, 0.0, 0.3)
        return Beam(name, x, [12, 12, 12, 12, 9, 12, 12, 5], 16, 4, [field_words()[0], field_boost(), gc.field_grammar()],
                    [0, 1, 1, 0, 1, 2, 1, 0], None, 0.7, lm, alpha, beta)
    if name in ("boost", "boost_lm"):
        x, g = boost_line()
        _, canon = bc.english()
        lm, alpha = (lm6(), 0.5) if name == "boost_lm" else (None, 0.0)
        return Beam("boost", x, [12], 16, 2, [g], None, canon, 1.0, lm, alpha, 0.0)
    assert name == "trie"
    al, canon = bc.english()
    x = bd.dense_logits(np.random.default_rng(1300), 12, 4, len(canon))
    return Beam("trie", x, [12] * 4, 16, 4, [big_weighted_trie()], None, canon, 1.0, bc.char_lm5(), 0.8, 0.6)


# ---- the guarded suite's beam cases (tests/test_wgrammar_guarded_gpu.py).  name: (seed, T, K, nbest, lens, which, with LM); a which
# outside [0, 3) gives its line no hypothesis
GUARDED_BEAM = {"K16": (71, 12, 16, 16, [12, 1, 0, 19, 12, 12, 9, 12], [0, 1, 2, 1, 5, 2, 0, 1], True),
                "K128": (72, 8, 128, 1, [8, 0, 9, 5, 8, 8, 3, 8], [1, 1, 0, 2, 2, 0, 1, -1], False)}


@functools.lru_cache(maxsize=None)
def guarded_beam_case(name):
    seed, T, K, nbest, lens, which, with_lm = GUARDED_BEAM[name]
    grammars = [field_words()[0], field_boost(), gc.field_grammar()]
    x = bd.dense_logits(np.random.default_rng(seed), T, len(lens), 13)
    lm, alpha, beta, gw = (gc.field_lm(), 0.8, 0.6, 0.7) if with_lm else (None, 0.0, 0.3, 1.25)
    return Beam("guarded", x, lens, K, nbest, grammars, which, None, gw, lm, alpha, beta)


@functools.lru_cache(maxsize=None)
def guarded_beam_reference(name):
    """the in-range lines by the restatement; a line whose which lies outside [0, 3) has no hypothesis and nothing to decide"""
    c = guarded_beam_case(name)
    ref = beam_references(c._replace(which=[k if 0 <= k < 3 else 0 for k in c.which]))
    return [r if 0 <= k < 3 else Ref([], np.inf) for r, k in zip(ref, c.which)]


BEAM_NAMES = ["ngram_K4", "ngram_K16", "ngram_K128", "brute", "dense", "dense_lm", "boost", "boost_lm", "trie"]
Ref = collections.namedtuple("Ref", "hyps gap")


def beam_references(c, gw=None):
    """tests/wgrammar_ref.py's search of every line of a case (gw: another grammar weight than the case's)"""
    gw = c.gw if gw is None else gw
    tabs = [(g.dense_tables(), tuple(t.astype(np.float64) for t in g.dense_weights())) for g in c.grammars]
    out = []
    for b in range(c.x.shape[1]):
        w = 0 if c.which is None else c.which[b]
        hyps, gap = wr.beam_search(c.x[:, b], c.lens[b], tabs[w][0], tabs[w][1], c.K, nbest=c.nbest, canon=c.canon, grammar_weight=gw,
                                   lm=c.lm, alpha=c.alpha, beta=c.beta)
        out.append(Ref(hyps, gap))
    return out


@functools.lru_cache(maxsize=None)
def beam_reference(name):
    return beam_references(beam_case(name))


def decided(ref):
    """gc.decided's sense: the lines on which no rank of the restatement lies within TAU of its neighbour"""
    return [b for b, r in enumerate(ref) if r.gap >= TAU]


def beam_compare(name, c, ref, lab, ln, sc, og):
    """The kernel's output against the restatement: on the decided lines labels, lengths and rank order exactly, the four scores
    (total, acoustic, lm, grammar) within the group's bars; on EVERY line every returned labelling is accepted and out_grammar is
    weight_of of it.  At most 1/8 of the lines may be undecided.  Prints the line of profiles/ctc_wgrammar_errors.txt before it
    asserts; returns the errors."""
    lines = decided(ref)
    B = lab.shape[0]
    err, wrong = np.zeros(4), []
    for b in range(B):
        filled = np.isfinite(sc[b, :, 0])
        assert not filled[1:][~filled[:-1]].any(), (name, b)
        assert (ln[b, ~filled] == 0).all() and (sc[b, ~filled, 0] == NEG).all() and not lab[b, ~filled].any(), (name, b)
        assert (og[b, ~filled] == 0).all(), (name, b)
        g = c.grammars[0 if c.which is None else c.which[b]]
        got = [(lab[b, q, :ln[b, q]].tolist(), list(sc[b, q]) + [og[b, q]]) for q in range(lab.shape[1]) if filled[q]]
        for y, s in got:
            w = g.weight_of(y)
            assert w is not None, (name, b, y)
            assert abs(s[3] - w) <= 4 * U * (len(y) + 1) * max(abs(w), 4.0), (name, b, y, s[3], w)       # a sum of len + 1 floats
        if b not in lines:
            continue
        if [y for y, _ in got] != [h[0] for h in ref[b].hyps]:
            wrong.append(b)
            continue
        for (_, s), h in zip(got, ref[b].hyps):
            err = np.maximum(err, np.abs(np.asarray(s, dtype=np.float64) - np.asarray(h[1:])))
    bar = bars(BEAM_RECORDED[c.group])
    print("wgrammar-beam-errors %-12s group %-8s K %3d V %3d T %2d B %d  compared %d/%d  max |score - fp64|: total %.2e acoustic %.2e lm "
          "%.2e grammar %.2e" % (name, c.group, c.K, c.x.shape[2], c.x.shape[0], B, len(lines), B, *err))
    assert not wrong, "%s: lines %s differ from the restatement" % (name, wrong)
    assert 8 * (B - len(lines)) <= B, "%s: %d of %d lines are undecided" % (name, B - len(lines), B)
    assert (err <= np.asarray(bar)).all(), (name, err, bar)
    return err
