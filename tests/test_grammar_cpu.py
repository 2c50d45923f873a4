"""CPU: tests/grammar_ref.py (the fp64 reference of the CTC grammar search) against its brute force over all frame paths, the grammar
compiler of vistaocr_amd/grammar.py against Python's re and plain set / substring tests, and the parts of
vocr_ctc_grammar_workspace_bytes / vocr_ctc_grammar_scores that need no device."""
import ctypes
import itertools
import re

import numpy as np
import pytest

import vistaocr_amd as va
from tests import grammar_ref as gr
from vistaocr_amd.grammar import Grammar

NEG = -np.inf


def _alphabet():
    """Letters, digits and space."""
    chars = [va.alphabet.BLANK] + ["u%04x" % ord(c) for c in "abcdefghijklmnopqrstuvwxyz0123456789 "]
    return va.Alphabet(chars, left_to_right=True)


def _random_dfa(rng, V):
    """A random PARTIAL deterministic automaton over classes 1 .. V-1: some states unreachable, the start accepting or not."""
    S = int(rng.integers(1, 6))
    arcs = []
    for s in range(S):
        for c in range(1, V):
            if rng.random() < 0.55:
                arcs.append((s, c, int(rng.integers(0, S))))
    accept = [s for s in range(S) if rng.random() < 0.5]
    return gr.make(S, arcs, accept)


@pytest.mark.parametrize("i", range(60))
def test_reference_against_brute_force(i):
    """Random partial automata, V <= 4, T <= 6; every third one gets a non-accepting start, every fifth accepts nothing but the empty
    labelling."""
    rng = np.random.default_rng(1000 + i)
    V, T = int(rng.integers(2, 5)), int(rng.integers(1, 7))
    a = _random_dfa(rng, V)
    if i % 3 == 0:
        a["accept"][0] = 0
    if i % 5 == 0:
        a["accept"][:] = 0
        a["accept"][0] = 1
        keep = a["dst"] != 0                                             # no way back to the start: only the empty labelling is accepted
        a = dict(a, src=a["src"][keep], cls=a["cls"][keep], dst=a["dst"][keep])
    x = rng.normal(0, 2, (T, 1, V))
    got = gr.search(x, [T], [a])
    want = gr.brute_force(x[:, 0], a)
    for g, w in ((got["logp"][0, 0], want[0]), (got["best"][0, 0], want[1])):
        assert (g == NEG) == (w == NEG), (g, w)
        if w != NEG:
            assert abs(g - w) <= 1e-12 * max(1.0, abs(w)), (g, w)


def test_reference_classes_and_empty_line():
    """A two-member class (columns 1 and 3) against the brute force; lens = 0: ln P = best = 0 iff the start accepts."""
    rng = np.random.default_rng(5)
    canon = [0, 1, 2, 1]
    a = gr.make(3, [(0, 1, 1), (1, 2, 2), (2, 3, 0), (1, 1, 1)], [0, 2], V=4, canon=canon)
    x = rng.normal(0, 2, (5, 1, 4))
    got, want = gr.search(x, [5], [a], canon), gr.brute_force(x[:, 0], a, canon)
    assert abs(got["logp"][0, 0] - want[0]) <= 1e-12 and abs(got["best"][0, 0] - want[1]) <= 1e-12
    got = gr.search(x, [0], [a, dict(a, accept=np.array([0, 1, 0], dtype=np.int32))], canon)
    assert got["logp"].tolist() == [[0.0, NEG]] and got["best"].tolist() == [[0.0, NEG]]


PATTERNS = ["abc", "a|b", "ab|cd|", "(a|b)*", "a*b+c?", "(ab)+", "a.c", ".*", ".+b", "[abc]d", "[a-c]+", "[^a]b", "[^a-c ]*", "\\d\\d", "\\d+a?",
            "a{2}", "a{1,3}b", "(ab){0,2}", "a{2,}", "(a|bc)*d", "a\\.?b", "[a\\d]+", "(a(b|c)*)?d", "a b", "((a))", "(a|b)(c|d)", "[ab-c]*",
            "\\d{1,2}/?\\d{1,2}"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_regex_compiler_against_re(pattern):
    """Acceptance equals re.fullmatch on every string up to length 4 over {a, b, c, 1} and on 300 random strings over the alphabet."""
    al = _alphabet()
    if "/" in pattern or "\\." in pattern:                                # symbols outside the alphabet are refused by name
        with pytest.raises(ValueError, match="not in the alphabet"):
            Grammar.from_regex(al, pattern)
        pattern = pattern.replace("/", "d").replace("\\.", "d")
    g = Grammar.from_regex(al, pattern)
    rx = re.compile(pattern)
    strings = ["".join(p) for n in range(5) for p in itertools.product("abc1", repeat=n)]
    rng = np.random.default_rng(len(pattern))
    every = "abcdefghijklmnopqrstuvwxyz0123456789 "
    strings += ["".join(rng.choice(list(every), int(rng.integers(0, 8)))) for _ in range(300)]
    wrong = [s for s in strings if g.accepts(s) != (rx.fullmatch(s) is not None)]
    assert not wrong, (pattern, wrong[:5])


def test_regex_errors():
    al = _alphabet()
    for bad in ["(a", "a)", "*a", "a{2", "a{3,1}", "[a", "a\\", "\\w"]:
        with pytest.raises(ValueError):
            Grammar.from_regex(al, bad)


def test_words_and_contains():
    al = _alphabet()
    words = ["cat", "car", "cart", "dog", "do", "a", "abab"]
    g = Grammar.from_words(al, words)
    probes = words + ["", "ca", "carts", "d", "og", "ab", "aba", "ababa"]
    assert all(g.accepts(w) == (w in words) for w in probes)
    assert g.accepts([al.char_to_idx["u0061"]]) and g.max_in_degree >= 1
    strings = ["".join(p) for n in range(7) for p in itertools.product("ab ", repeat=n)]
    for kw in ("aba", "ab", "a", "aa", "abab"):
        c = Grammar.contains(al, kw)
        assert all(c.accepts(s) == (kw in s) for s in strings), kw
        w = Grammar.contains(al, kw, whole_word=True)
        assert all(w.accepts(s) == (kw in s.split(" ")) for s in strings), kw
    assert Grammar.contains(al, "aba").n_states == 4                      # the minimal automaton of .*aba.*: one state per matched prefix


def test_minimisation_and_arc_order():
    al = _alphabet()
    g = Grammar.from_regex(al, "(a|b)*")
    assert g.n_states == 1 and g.n_arcs == 2 and g.max_in_degree == 2
    assert Grammar.from_regex(al, "a|a|aa*").n_states == 2                # a+: two states
    assert Grammar.from_regex(al, "[^a-z0-9 ]").n_arcs == 0               # the empty language: the start alone, accepting nothing
    for g in (Grammar.from_regex(al, "(ab|cd)*e?\\d{2}"), Grammar.from_words(al, ["one", "two", "three", "tone"]), Grammar.contains(al, "abc")):
        keys = list(zip(g.arc_dst.tolist(), g.arc_cls.tolist(), g.arc_src.tolist()))
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        assert gr.valid(gr.from_grammar(g), len(al), np.arange(len(al)), g.n_states, g.n_arcs)
        assert g.arc_src.dtype == np.int32 and g.accept.shape == (g.n_states,)


def test_from_dfa_and_complement():
    al = _alphabet()
    g = Grammar.from_regex(al, "ab*")
    trans, accept = g.dfa()
    classes = sorted({c for c in al.canonical_indices()[1:]})
    sink = len(trans)                                                     # complete it with a sink, flip the flags
    full = [{c: row.get(c, sink) for c in classes} for row in trans] + [{c: sink for c in classes}]
    comp = Grammar.from_dfa(al, full, [not a for a in accept] + [True])
    for s in ["", "a", "ab", "abb", "b", "ba", "abc", "zzz"]:
        assert comp.accepts(s) != g.accepts(s), s
    with pytest.raises(ValueError):
        Grammar.from_dfa(al, [{"a": 3}], [True])
    with pytest.raises(ValueError):
        Grammar.from_dfa(al, [{"?": 0}], [True])
    assert Grammar.from_dfa(al, [{"a": 1, "b": 2}, {}, {}], [False, True, True]).n_states == 2      # the two accepting leaves merge


def test_two_member_classes_share_an_arc():
    """The English alphabet lists u002d twice (73 and 91): one class, one arc, and either index is accepted."""
    al = va.english_alphabet()
    canon = al.canonical_indices()
    twins = [k for k in range(len(canon)) if canon[k] != k]
    assert twins
    k = twins[0]
    g = Grammar.from_regex(al, "a-b")
    assert g.n_arcs == 3 and canon[k] in g.arc_cls.tolist() and k not in g.arc_cls.tolist()
    a, b = al.char_to_idx["u0061"], al.char_to_idx["u0062"]
    assert g.accepts([a, k, b]) and g.accepts([a, canon[k], b]) and not g.accepts([a, b])
    d = Grammar.from_dfa(al, [{canon[k]: 1, k: 1}, {}], [False, True])
    assert d.n_arcs == 1
    with pytest.raises(ValueError, match="not deterministic"):
        Grammar.from_dfa(al, [{canon[k]: 1, k: 0}, {}], [False, True])


def test_matcher_splits_a_call_at_the_kernels_limits():
    """GrammarMatcher cuts the list into calls the kernel takes (cells: the largest state count plus the largest arc count; with best
    paths the 2 GiB of back pointers) and names a grammar that fits no call."""
    from vistaocr_amd.grammar import group_grammars
    al = _alphabet()
    gs = [Grammar.contains(al, "the"), Grammar.from_regex(al, ".*"), Grammar.from_words(al, ["cat", "dog"])]
    cells = max(g.n_states for g in gs) + max(g.n_arcs for g in gs)
    assert group_grammars(gs, 294, 32, True) == [gs] and group_grammars(gs, 294, 1 << 20, False) == [gs]
    lines = (1 << 31) // (294 * 4 * 2 * cells)                            # two grammars' back pointers fit, three do not
    assert group_grammars(gs, 294, lines, True) == [gs[:2], gs[2:]]
    with pytest.raises(ValueError, match="contains 'the' has 4 states"):
        group_grammars(gs, 294, 1 << 22, True)
    rng = np.random.default_rng(3)
    letters, every = list("abcdefghijklmnopqrstuvwxyz"), "abcdefghijklmnopqrstuvwxyz0123456789 "
    words = sorted({"".join(rng.choice(letters, 8)) for _ in range(1500)})
    many = Grammar.from_words(al, words[:850])                            # the states come from this one, the arcs from the next
    wide = Grammar.from_dfa(al, [{c: int(rng.integers(0, 130)) for c in every} for _ in range(130)], [int(v) for v in rng.integers(0, 2, 130)])
    assert many.n_states + wide.n_arcs > 8192 >= max(many.n_states + many.n_arcs, wide.n_states + wide.n_arcs)
    assert group_grammars([many, wide], 8, 1, False) == [[many], [wide]]
    huge = Grammar.from_words(al, words)
    assert huge.n_states + huge.n_arcs > 8192
    with pytest.raises(ValueError, match="more than the kernel's 8192 cells"):
        group_grammars([many, huge], 8, 1, False)


def test_shape_answers_without_a_device():
    from vistaocr_amd import _lib, build
    build.build()
    lib = _lib.load()
    ws = lib.vocr_ctc_grammar_workspace_bytes
    assert ws(294, 32, 96, 4, 100, 800, 0) > 0 and ws(294, 4, 96, 4, 4000, 4192, 1) > ws(294, 4, 96, 4, 4000, 4192, 0) > 0
    assert ws(1, 1, 2, 1, 1, 0, 1) > 0
    bad = [(294, 32, 1, 4, 100, 800, 0), (294, 32, 257, 4, 100, 800, 0), (294, 32, 96, 0, 100, 800, 0), (294, 32, 96, 4, 0, 800, 0),
           (294, 32, 96, 4, 100, -1, 0), (294, 32, 96, 4, 4000, 4193, 0), (294, 32, 96, 1 << 18, 100, 800, 0), (0, 32, 96, 4, 100, 800, 0),
           (294, 32, 96, 64, 4000, 4192, 1)]                               # the last: 2.3 GiB of back pointers
    one = ctypes.c_void_p(16)
    for t, b, v, g, ms, ma, wb in bad:
        assert ws(t, b, v, g, ms, ma, wb) == 0, (t, b, v, g, ms, ma, wb)
        best = one if wb else None
        rc = lib.vocr_ctc_grammar_scores(one, one, t, b, v, None, one, one, g, one, one, one, one, ms, ma, one, best, best, best, max(t, 1), one,
                                         1 << 40, None)
        assert rc == -1 and b"vocr_ctc_grammar_scores" in lib.vocr_last_error(), (t, b, v, g, ms, ma, wb)
    assert ws(294, 32, 96, 64, 4000, 4192, 0) > 0                         # ... which a scores-only call does not need
    call = lambda *a: lib.vocr_ctc_grammar_scores(*a)
    ok = (8, 2, 50, None, one, one, 3, one, one, one, one, 10, 20)
    big = 1 << 30
    assert call(None, one, *ok, one, one, one, one, 8, one, big, None) == -1 and b"null pointer" in lib.vocr_last_error()
    assert call(one, one, *ok, None, one, one, one, 8, one, big, None) == -1                      # no out_logp
    assert call(one, one, *ok, one, one, None, one, 8, one, big, None) == -1 and b"all NULL or all given" in lib.vocr_last_error()
    assert call(one, one, *ok, one, None, None, one, 8, one, big, None) == -1 and b"all NULL or all given" in lib.vocr_last_error()
    assert call(one, one, *ok, one, one, one, one, 7, one, big, None) == -1 and b"label_stride" in lib.vocr_last_error()
    assert call(one, one, *ok, one, one, one, one, 8, one, 16, None) == -1 and b"workspace too small" in lib.vocr_last_error()
    assert call(one, one, *ok, one, None, None, None, 0, ctypes.c_void_p(8), big, None) == -1 and b"16-byte aligned" in lib.vocr_last_error()
