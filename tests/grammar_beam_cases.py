"""Pinned inputs of the grammar-constrained beam search's tests (tests/test_grammar_beam_cpu.py, tests/test_grammar_beam_gpu.py,
tests/test_grammar_beam_guarded_gpu.py) and their fp64 references (tests/grammar_beam_ref.py).  Test helper only.  The references are
computed once per process and shared; the CPU test holds their floors of compared lines with the restatement alone, the GPU tests
compare the kernel with the same objects.

Score bars.  Labels, lengths and rank order have no tolerance on a line whose restatement gap is at least TAU (tests/beam_cases.py's
2e-4).  The three scores are held to fp64 at 4 times the largest |score - fp64| recorded per group on the MI355X
(profiles/ctc_grammar_beam_errors.txt), the margin of the other beam suites, never above their ceiling of 1e-3."""
import collections
import functools
import os
import tempfile

import numpy as np

import vistaocr_amd as va
from tests import beam_cases as bc
from tests import beam_data as bd
from tests import grammar_beam_ref as gbr
from vistaocr_amd.grammar import Grammar

TAU = bc.TAU
Case = collections.namedtuple("Case", "group x lens K nbest grammars which canon lm alpha beta")
Ref = bc.Ref

# group: the largest |score - fp64| of (total, acoustic, lm) over the compared hypotheses of the group's cases, recorded on the MI355X
# (profiles/ctc_grammar_beam_errors.txt).  Without an LM the LM score is 0 on both sides.
RECORDED = {
    "brute": (2.51e-06, 2.51e-06, 0.0),
    "dense": (1.97e-05, 1.97e-05, 0.0),
    "dense_lm": (2.60e-05, 2.36e-05, 2.12e-06),
    "which": (9.85e-06, 9.85e-06, 0.0),
    "trie_lm": (1.50e-05, 1.39e-05, 4.04e-06),
    "corners": (4.09e-06, 3.77e-06, 0.0),
    "guarded": (8.80e-06, 8.80e-06, 2.99e-06),
}


def bars(group):
    return tuple(min(4.0 * r, bc.CEILING) for r in RECORDED[group])


def letters(V, first=0x61):
    return bc._letters_alphabet(V, first)


# ---- the brute-force case: V = 4, T = 6, `1 (2|3)* 1`
@functools.lru_cache(maxsize=None)
def tiny_grammar():
    return Grammar.from_regex(letters(4), "a[bc]*a")


def tiny_logits(seed):
    return np.random.default_rng(1000 + seed).normal(0, 2, size=(6, 4)).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def tiny_brute(seed):
    """Every labelling of the line the grammar accepts, best first, from beam_ref.brute_force: [(labels, total, acoustic, lm)]."""
    g = tiny_grammar()
    return [h for h in bc.br.brute_force(tiny_logits(seed), [1, 2, 3]) if g.accepts(h[0])]


# ---- the dense case: N(0, 3), T = 24, V = 13, B = 32, `digit digit - digit digit`
@functools.lru_cache(maxsize=None)
def field_alphabet():
    """blank, the ten digits, '-' and one letter: V = 13"""
    return va.Alphabet(["<ctc-blank>"] + ["u%04x" % (0x30 + d) for d in range(10)] + ["u002d", "u0061"], left_to_right=True)


@functools.lru_cache(maxsize=None)
def field_grammar():
    return Grammar.from_regex(field_alphabet(), r"\d\d-\d\d")


@functools.lru_cache(maxsize=None)
def field_lm():
    al = field_alphabet()
    with tempfile.TemporaryDirectory() as d:
        path = bd.write_char_arpa(os.path.join(d, "field3.arpa"), [al.idx_to_char[c] for c in range(1, 13)], order=3, seed=5)
        return va.CharNgramLM.from_arpa(path, al)


DENSE_K = (1, 5, 16, 128)
DENSE = ["dense_K%d%s" % (K, s) for K in DENSE_K for s in ("", "_lm")]


def _dense(K, with_lm):
    x = bd.dense_logits(np.random.default_rng(4100 + K + (7 if with_lm else 0)), 24, 32, 13)
    lm, alpha, beta = (field_lm(), 0.8, 0.6) if with_lm else (None, 0.0, 0.0)
    return Case("dense_lm" if with_lm else "dense", x, [24] * 32, K, min(K, 4), [field_grammar()], None, None, lm, alpha, beta)


# ---- a trie beyond the sweep kernels' 8192 cells: about 3000 random words over the English letters, with the character 5-gram
@functools.lru_cache(maxsize=None)
def big_trie():
    al, _ = bc.english()
    rng = np.random.default_rng(77)
    abc = "abcdefghijklmnopqrstuvwxyz"
    words = sorted({"".join(abc[i] for i in rng.integers(0, 26, size=rng.integers(3, 9))) for _ in range(3000)})
    return Grammar.from_words(al, words), words


TRIE = ["trie_K16_lm"]


def _trie():
    al, canon = bc.english()
    x = bd.dense_logits(np.random.default_rng(4300), 16, 16, len(canon))
    return Case("trie_lm", x, [16] * 16, 16, 4, [big_trie()[0]], None, canon, bc.char_lm5(), 0.8, 0.6)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in TRIE:
        return _trie()
    K = int(name.split("_")[1][1:])
    return _dense(K, name.endswith("_lm"))


def references(c, tables=None):
    """The restatement of every line of a case; tables: per grammar (next, dist), the grammars' own by default."""
    tables = [g.dense_tables() for g in c.grammars] if tables is None else tables
    out = []
    for b in range(c.x.shape[1]):
        w = 0 if c.which is None else c.which[b]
        if not 0 <= w < len(tables):
            out.append(Ref([], np.inf, {}))
            continue
        hyps, gap = gbr.beam_search(c.x[:, b], c.lens[b], tables[w], c.K, nbest=c.nbest, canon=c.canon, lm=c.lm, alpha=c.alpha,
                                    beta=c.beta)
        out.append(Ref(hyps, gap, {}))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    return references(case(name))


def decided(ref):
    return [b for b, r in enumerate(ref) if r.gap >= TAU]


def compare(name, c, ref, lab, ln, sc, floor=None):
    """The kernel's output against the restatement: on the decided lines labels, lengths and rank order exactly (a line without a
    hypothesis must have none on both sides), the three scores within the group's bars; every returned labelling is accepted by its
    line's grammar on EVERY line.  Prints the line of profiles/ctc_grammar_beam_errors.txt before it asserts; returns the errors."""
    lines = decided(ref)
    err = np.zeros(3)
    wrong = []
    for b in range(lab.shape[0]):
        got = [(list(lab[b, q, :ln[b, q]]), sc[b, q]) for q in range(lab.shape[1]) if np.isfinite(sc[b, q, 0])]
        filled = np.isfinite(sc[b, :, 0])
        assert not filled[1:][~filled[:-1]].any(), (name, b)                   # best first: no filled rank behind an unfilled one
        assert (ln[b, ~filled] == 0).all() and (sc[b, ~filled, 0] == -np.inf).all() and not lab[b, ~filled].any(), (name, b)
        w = 0 if c.which is None else c.which[b]
        for y, _ in got:
            assert 0 <= w < len(c.grammars) and c.grammars[w].accepts(y), (name, b, y)
        if b not in lines:
            continue
        want = ref[b].hyps
        if [g[0] for g in got] != [h[0] for h in want]:
            wrong.append(b)
            continue
        for g, h in zip(got, want):
            err = np.maximum(err, np.abs(np.asarray(g[1], dtype=np.float64) - np.asarray(h[1:])))
    bar = bars(c.group)
    T, B, V = c.x.shape
    print("%-22s %-9s K %3d V %3d T %3d B %2d  compared %2d/%-2d  max |score - fp64|: total %.2e acoustic %.2e lm %.2e  bars %.1e %.1e "
          "%.1e" % (name, c.group, c.K, V, T, B, len(lines), B, err[0], err[1], err[2], *bar))
    assert not wrong, "%s: lines %s differ from the restatement" % (name, wrong)
    floor = (3 * B + 3) // 4 if floor is None else floor
    assert len(lines) >= floor, "%s: only %d of %d lines are decided by more than %g" % (name, len(lines), B, TAU)
    assert (err <= np.asarray(bar)).all(), (name, err, bar)
    return err
