"""Pinned inputs of the fp64 seam tests of the two CTC beam searches (tests/test_beam_fp64_gpu.py, tests/test_word_beam_fp64_gpu.py)
and their references.  Test helper only.

Every case is a batch of lines with the search's settings and a floor: the number of lines whose decisions the fp64 restatement
(tests/beam_ref.py, tests/word_beam_ref.py) took by at least TAU, which the CPU tests hold to at least half of the batch with the
restatement alone.  The regimes are the ones the peaky inputs of the older tests never reach: dense logits (every one of the K*V
candidate slots finite, the radix select cuts thousands of live scores), bitwise-duplicated columns (the cut and the final ranks
fall inside exact ties), prefixes that leave the beam and come back under a new node id while their child stays (pinned by seed,
and one built by hand), every intermediate beam of a line (lens = 1..T, nbest = K), and the largest launch (K = 128, V = 256).  The
references are computed once per process and shared: the CPU tests check the counters that pin the inputs, the GPU tests compare the
kernels with the same objects.

Score bars.  Labels, lengths and rank order have no tolerance.  The three scores keep the older tests' absolute 1e-3 as a ceiling (it
was set for T = 294); for the short lines here each group's bar is 4 times the largest |score - fp64| recorded on the MI355X
(profiles/beam_fp64_errors.txt; the factor covers the spread between seeds), so a regression of the fp32 arithmetic shows."""
import collections
import functools
import itertools
import os
import tempfile

import numpy as np

import vistaocr_amd as va
from tests import beam_data as bd
from tests import beam_ref as br
from tests import word_beam_data as wd
from tests import word_beam_ref as wr
from vistaocr_amd.alphabet import Alphabet

TAU = 2e-4          # a line is compared only where every decision of the fp64 restatement won by at least this much
CEILING = 1e-3      # the older tests' score bar

Case = collections.namedtuple("Case", "group x lens K nbest canon lm alpha beta prune oov exact_ties floor dense")
Ref = collections.namedtuple("Ref", "hyps gap stats")

# group: the largest |score - fp64| of (total, acoustic, lm) over the compared lines of the group's cases, recorded on the MI355X
# (profiles/beam_fp64_errors.txt).  Without an LM the LM score is 0 on both sides.
RECORDED = {
    "dense": (8.83e-06, 8.83e-06, 0.0),
    "dense_lm": (2.52e-05, 1.14e-05, 2.78e-05),
    "variants": (2.71e-05, 8.99e-06, 2.57e-05),
    "big": (2.16e-06, 2.16e-06, 0.0),
    "intermediate": (4.95e-06, 4.95e-06, 0.0),
    "ties": (5.07e-06, 5.07e-06, 0.0),
    "comeback": (1.11e-06, 1.11e-06, 0.0),
    "word_closed": (1.44e-05, 1.20e-05, 9.93e-06),
    "word_oov": (1.07e-05, 1.01e-05, 2.19e-06),
    "word_big": (2.11e-06, 2.39e-06, 1.27e-07),
    "word_ties": (2.87e-06, 1.90e-06, 1.23e-06),
}


def bars(group):
    """The group's score bars: 4 x its recorded maxima, never above the older tests' 1e-3."""
    return tuple(min(4.0 * r, CEILING) for r in RECORDED[group])


def _case(group, x, K, nbest, lens=None, canon=None, lm=None, alpha=0.0, beta=0.0, prune=None, oov=None, exact_ties=False,
          floor=None, dense=True):
    B = x.shape[1]
    lens = [x.shape[0]] * B if lens is None else list(lens)
    return Case(group, x, lens, K, nbest, canon, lm, alpha, beta, prune, oov, exact_ties, (B + 1) // 2 if floor is None else floor,
                dense)


@functools.lru_cache(maxsize=None)
def english():
    al = va.english_alphabet()
    return al, np.array(al.canonical_indices())


@functools.lru_cache(maxsize=None)
def arabic():
    al = va.arabic_alphabet()
    return al, np.array(al.canonical_indices())


@functools.lru_cache(maxsize=None)
def char_lm5():
    """The character 5-gram of tests/test_beam_gpu.py's lm5 fixture."""
    al = english()[0]
    with tempfile.TemporaryDirectory() as d:
        path = bd.write_char_arpa(os.path.join(d, "char5.arpa"), [al.idx_to_char[c] for c in range(1, 40)], order=5, seed=3)
        return va.CharNgramLM.from_arpa(path, al)


# ---------------------------------------------------------------------------------------------------------------- character search

V12_PAIRS = [(9, 5), (7, 3)]                # tie inputs: column 9 = column 5, column 7 = column 3
ENGLISH_PAIRS = [(40, 20), (55, 33)]        # two duplicated letter columns of the English alphabet (different classes)

# come-back cases: V = 4, T = 10, sigma = 2.5, rng seed 1000 + s; found by counting `remerges` over 300 seeds per K (about 2 % of
# them have one), all decided by > 8e-3
COMEBACK = {3: [6, 90, 228, 261], 4: [6, 90, 140, 228], 5: [6, 90, 107, 140, 173, 261], 6: [6, 83, 107, 173, 208, 291]}

# The hand-built come-back, as probabilities (columns: blank, a, b, c), K = 5.  After frame 1 the beam is b, ab, "", c, cb and "a"
# (.045) is cut below cb (.075) while its child "ab" stays.  Frame 2 re-creates "a" from "" (.0495, rank 4: node 2*5 + 4) next to
# the staying "ab", whose node still names the "a" of frame 0 as its parent.  Frame 3 extends "a" by b: the merge into "ab" has to
# find the parent by walking the two node chains, the node ids differ.
HAND_PROBS = [[.6, .3, 0, .1], [.15, 0, .75, .1], [.35, .55, 0, .1], [.05, 0, .9, .05]]
HAND_K = 5
HAND_KEPT = [{(), (1,), (3,)}, {(2,), (1, 2), (), (3,), (3, 2)}, {(2, 1), (2,), (1, 2, 1), (1, 2), (1,)}]


def _dense_english(seed, T, B, K, nbest=None, with_lm=False, group=None, **kw):
    al, canon = english()
    x = bd.dense_logits(np.random.default_rng(seed), T, B, len(al))
    lm = char_lm5() if with_lm else None
    return _case(group or ("dense_lm" if with_lm else "dense"), x, K, min(K, 4) if nbest is None else nbest, canon=canon, lm=lm,
                 alpha=0.8 if with_lm else 0.0, beta=1.0 if with_lm else 0.0, **kw)


def _intermediate(seed, T, K):
    al, canon = english()
    line = bd.dense_logits(np.random.default_rng(seed), T, 1, len(al))
    return _case("intermediate", np.repeat(line, T, axis=1), K, K, lens=range(1, T + 1), canon=canon, dense=False)


def _ties_v12(K):
    x = bd.tie_logits(np.random.default_rng(70 + K), 20, 16, 12, 2.0, V12_PAIRS)
    return _case("ties", x, K, min(K, 8), exact_ties=True, dense=False)


def _ties_english():
    al, canon = english()
    assert all(canon[c] == c for pair in ENGLISH_PAIRS for c in pair)
    x = bd.tie_logits(np.random.default_rng(81), 20, 16, len(al), 3.0, ENGLISH_PAIRS)
    return _case("ties", x, 16, 8, canon=canon, exact_ties=True)


def _comeback(K):
    x = np.stack([np.random.default_rng(1000 + s).normal(0, 2.5, size=(10, 4)).astype(np.float32) for s in COMEBACK[K]], axis=1)
    return _case("comeback", x, K, K, floor=x.shape[1], dense=False)


def hand_logits():
    with np.errstate(divide="ignore"):
        return np.log(np.array(HAND_PROBS))[:, None, :].astype(np.float32)


def _ragged():
    T = 24
    return _dense_english(23, T, 12, 16, with_lm=True, group="variants", lens=[0, 1, T, T + 9, 2, 3, 7, 13, 23, 5, T, 18], dense=False)


def _arabic():
    al, canon = arabic()
    return _case("variants", bd.dense_logits(np.random.default_rng(51), 24, 16, len(al)), 16, 4, canon=canon)


CHAR_CASES = {}
for _K in (1, 5, 16, 64, 100, 128):
    _T = 24 if _K <= 16 else 12             # at T = 24 the restatement decides 10 - 16 of 32 lines at K = 100 / 128: too close
    CHAR_CASES["K%d" % _K] = functools.partial(_dense_english, 100 + _K, _T, 32, _K)
    CHAR_CASES["K%d_lm" % _K] = functools.partial(_dense_english, 100 + _K, _T, 32, _K, with_lm=True)
CHAR_CASES.update({
    "K16_nbest16_lm": functools.partial(_dense_english, 31, 24, 32, 16, nbest=16, with_lm=True, group="variants"),
    # pruning thins the candidates by design (at most 96 / 448 live at -3 / -6): these two are not held to the density floor
    "K16_prune3_lm": functools.partial(_dense_english, 41, 24, 32, 16, with_lm=True, group="variants", prune=-3.0, dense=False),
    "K16_prune6_lm": functools.partial(_dense_english, 41, 24, 32, 16, with_lm=True, group="variants", prune=-6.0, dense=False),
    "arabic_K16": _arabic,
    "ragged_K16_lm": _ragged,
    "B1_K16": functools.partial(_dense_english, 25, 24, 1, 16, group="variants"),
    "B65_K16": functools.partial(_dense_english, 26, 12, 65, 16, group="variants"),
    "big_K128_V256": lambda: _case("big", bd.dense_logits(np.random.default_rng(61), 10, 16, 256), 128, 4),
    "inter_K16": functools.partial(_intermediate, 90, 24, 16),
    "inter_K5": functools.partial(_intermediate, 91, 24, 5),
    "tie_english_K16": _ties_english,
})
for _K in (4, 7, 16, 64):
    CHAR_CASES["tie_K%d" % _K] = functools.partial(_ties_v12, _K)
for _K in sorted(COMEBACK):
    CHAR_CASES["comeback_K%d" % _K] = functools.partial(_comeback, _K)

CHAR_DENSE = ["K%d%s" % (K, s) for K in (1, 5, 16, 64, 100, 128) for s in ("", "_lm")]
CHAR_VARIANTS = ["K16_nbest16_lm", "K16_prune3_lm", "K16_prune6_lm", "arabic_K16", "ragged_K16_lm", "B1_K16", "B65_K16"]
CHAR_TIES = ["tie_K4", "tie_K7", "tie_K16", "tie_K64", "tie_english_K16"]
CHAR_COMEBACK = ["comeback_K%d" % K for K in sorted(COMEBACK)]
CHAR_INTERMEDIATE = ["inter_K16", "inter_K5"]


@functools.lru_cache(maxsize=None)
def char_case(name):
    return CHAR_CASES[name]()


@functools.lru_cache(maxsize=None)
def char_reference(name):
    """The fp64 restatement of every line of the case: [Ref(hyps, gap, stats)]."""
    c = char_case(name)
    out = []
    for b in range(c.x.shape[1]):
        stats = {}
        hyps, gap = br.beam_search(c.x[:, b], c.lens[b], c.K, nbest=c.nbest, canon=c.canon, lm=c.lm, alpha=c.alpha, beta=c.beta,
                                   prune=c.prune, exact_ties=c.exact_ties, stats=stats)
        out.append(Ref(hyps, gap, stats))
    return out


def kept_path_scores(lp, kept):
    """Brute force over the V^T alignments of class log-probs lp [T, V] that a beam search with the beams kept[t] after frame t
    (t < T - 1) can still see: the alignments whose collapsed prefix is in kept[t] after every such frame.  Returns
    {labelling: ln of the summed probability}: the acoustic score the search must hold for every prefix after the last frame."""
    T, V = lp.shape
    out = {}
    for path in itertools.product(range(V), repeat=T):
        pref, prev, ok = (), 0, True
        for t, c in enumerate(path):
            if c != 0 and c != prev:
                pref = pref + (c,)
            prev = c
            if t < T - 1 and pref not in kept[t]:
                ok = False
                break
        p = sum(lp[t, c] for t, c in enumerate(path))
        if ok and np.isfinite(p):
            out[pref] = np.logaddexp(out.get(pref, -np.inf), p)
    return out


# --------------------------------------------------------------------------------------------------------------------- word search

@functools.lru_cache(maxsize=None)
def word_lm400():
    """The 400-word Zipf lexicon and word 3-gram of tests/test_word_beam_gpu.py's corpus fixture."""
    al = english()[0]
    rng = np.random.default_rng(1)
    words, wts = wd.make_lexicon(rng, 400)
    sents = wd.make_sentences(rng, words, wts, 1532, max_words=6)
    with tempfile.TemporaryDirectory() as d:
        path = wd.write_word_arpa(os.path.join(d, "word3.arpa"), words, wts, sents[:1500], seed=2)
        return va.WordNgramLM.from_arpa(path, al)


def _letters_alphabet(V, first=0x61):
    return Alphabet(["<ctc-blank>"] + ["u%04x" % (first + i) for i in range(V - 1)], left_to_right=True)


@functools.lru_cache(maxsize=None)
def tiny_word_lm(kind):
    """tests/test_word_beam_cpu.py's ARPA3 (lexicon a, b, ab, ba, cab; the single '.') over one of three alphabets:
    'v256': its 7 symbols followed by 249 more letters, the largest V; 'de': its 7 symbols and the letters d, e, which start no
    lexicon word; an int V: blank and V - 1 letters from 'a' on (the equivalence tests, where only the letter kinds matter)."""
    from tests.test_word_beam_cpu import ALPHA, ARPA3
    base = [ALPHA.idx_to_char[c] for c in range(len(ALPHA))]
    if kind == "v256":
        al = Alphabet(base + ["u%04x" % (0x100 + i) for i in range(256 - len(base))], left_to_right=True)
    elif kind == "de":
        al = Alphabet(base + ["u0064", "u0065"], left_to_right=True)
    else:
        al = _letters_alphabet(int(kind))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "w3.arpa")
        with open(path, "w") as fh:
            fh.write(ARPA3)
        return va.WordNgramLM.from_arpa(path, al)


def _dense_word(seed, T, B, K, oov):
    al, canon = english()
    x = bd.dense_logits(np.random.default_rng(seed), T, B, len(al))
    # a closed vocabulary thins the candidates by design (a letter that leaves the trie is none): only the open cases are held to
    # the density floor
    return _case("word_oov" if oov is not None else "word_closed", x, K, min(K, 4), canon=canon, lm=word_lm400(), alpha=0.8, beta=1.0,
                 oov=oov, dense=oov is not None)


def _big_word():
    x = bd.dense_logits(np.random.default_rng(63), 8, 6, 256)
    return _case("word_big", x, 128, 4, lm=tiny_word_lm("v256"), alpha=0.8, beta=1.0, oov=-3.0)


def _tie_word():
    """Columns 7 and 8 (d, e) bitwise equal: both leave the trie at once, so the two OOV beams share look-ahead and close score."""
    x = bd.tie_logits(np.random.default_rng(77), 12, 16, 9, 2.0, [(8, 7)])
    return _case("word_ties", x, 6, 6, lm=tiny_word_lm("de"), alpha=0.8, beta=1.0, oov=-2.5, exact_ties=True, dense=False)


WORD_SIZES = {5: (24, 16), 16: (24, 16), 64: (12, 12), 128: (8, 12)}       # K: (T, B), cut so a case's restatement takes seconds
WORD_CASES = {"w_big_K128_V256": _big_word, "w_tie_lm_K6": _tie_word}
for _K, (_T, _B) in WORD_SIZES.items():
    WORD_CASES["w_K%d_closed" % _K] = functools.partial(_dense_word, 300 + _K, _T, _B, _K, None)
    WORD_CASES["w_K%d_oov" % _K] = functools.partial(_dense_word, 300 + _K, _T, _B, _K, -3.0)
WORD_DENSE = ["w_K%d_%s" % (K, s) for K in WORD_SIZES for s in ("closed", "oov")]


@functools.lru_cache(maxsize=None)
def word_case(name):
    return WORD_CASES[name]()


@functools.lru_cache(maxsize=None)
def word_reference(name):
    c = word_case(name)
    out = []
    for b in range(c.x.shape[1]):
        stats = {}
        hyps, gap = wr.beam_search(c.x[:, b], c.lens[b], c.K, c.lm, nbest=c.nbest, canon=c.canon, alpha=c.alpha, beta=c.beta,
                                   oov=c.oov, exact_ties=c.exact_ties, stats=stats)
        out.append(Ref(hyps, gap, stats))
    return out


# ------------------------------------------------------------------------------------------------------------------------ comparing

def decided(case, ref):
    """The lines of the case that are compared: every decision of the restatement won by at least TAU."""
    return [b for b, r in enumerate(ref) if r.gap >= TAU]


def total(case, ref, key):
    """A counter of the restatement summed over the decided lines."""
    return sum(ref[b].stats[key] for b in decided(case, ref))


def check_pinned(name, case, ref):
    """What pins the case, from the restatement alone: the floor of compared lines, and for a dense case at least K*V/2 finite
    candidates in some frame of every compared line, so the input cannot silently turn sparse."""
    lines = decided(case, ref)
    assert len(lines) >= case.floor >= (case.x.shape[1] + 1) // 2, (name, len(lines), case.floor)
    if case.dense:
        for b in lines:
            assert ref[b].stats["max_live"] >= case.K * case.x.shape[2] / 2, (name, b, ref[b].stats)


def compare(name, case, ref, lab, ln, sc):
    """The kernel's output (labels [B, nbest, T], lengths [B, nbest], scores [B, nbest, 3]) against the restatement on the decided
    lines: labels, lengths and rank order exactly (an empty rank list must be empty on both sides), the three scores within the
    group's bars.  Asserts the floor, prints the line of profiles/beam_fp64_errors.txt, returns (compared, max errors)."""
    lines = decided(case, ref)
    err = np.zeros(3)
    for b in lines:
        got = [(list(lab[b, q, :ln[b, q]]), sc[b, q]) for q in range(lab.shape[1]) if np.isfinite(sc[b, q, 0])]
        want = ref[b].hyps
        assert [g[0] for g in got] == [w[0] for w in want], (name, b, case.K)
        for g, w in zip(got, want):
            err = np.maximum(err, np.abs(np.asarray(g[1], dtype=np.float64) - np.asarray(w[1:])))
    bar = bars(case.group)
    T, B, V = case.x.shape
    print("%-18s %-13s K %3d V %3d T %3d B %2d  compared %2d/%-2d (floor %2d)  max |score - fp64|: total %.2e acoustic %.2e lm %.2e"
          "  bars %.1e %.1e %.1e" % (name, case.group, case.K, V, T, B, len(lines), B, case.floor, err[0], err[1], err[2], *bar))
    assert len(lines) >= case.floor, "%s: only %d of %d lines are decided by more than %g" % (name, len(lines), B, TAU)
    assert (err <= np.asarray(bar)).all(), (name, err, bar)
    return len(lines), err
