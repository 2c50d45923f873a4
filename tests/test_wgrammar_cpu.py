"""CPU: the weighted grammars' host side.  tests/wgrammar_ref.py's restatements against an independent brute force over all frame paths
and against central differences; Grammar.weight_of of boost / from_words / from_ngram exhaustively over every string of up to 5 of 3
symbols; the weighted minimisation; the validation of weights; the weighted entries' workspace queries and host argument checks (no
launch); and the floors of decided lines that tests/test_wgrammar_gpu.py relies on."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import grammar_beam_cases as gc
from tests import wgrammar_cases as wc
from tests import wgrammar_ref as wr
from tests.align_ref import classes_of
from vistaocr_amd.grammar import Grammar, pack_dense_grammars, pack_grammars

NEG = -np.inf


# ------------------------------------------------------------------------------------------------ the restatements
def test_sweep_equals_brute_force():
    """V = 4 (two columns one class), T <= 5, the tiny automaton: non-deterministic, a self loop, an arc into the start."""
    a, x = wc.tiny_automaton(), wc.tiny_logits()
    for b, n in enumerate(wc.TINY_LENS):
        ref = wr.search(x[:, b:b + 1], [n], [a], wc.TINY_CANON)
        lnz, top, _ = wr.brute_force(x[:n, b], a, wc.TINY_CANON)
        assert np.isfinite(lnz) and abs(ref["logp"][0, 0] - lnz) < 1e-12 and abs(ref["best"][0, 0] - top) < 1e-12, (b, ref, lnz, top)
    ref = wr.search(x[:, :1], [0], [a], wc.TINY_CANON)                       # no frame: the start state's final weight
    assert ref["logp"][0, 0] == ref["best"][0, 0] == a["fw"][0]


def test_zero_weights_are_the_unweighted_recursion():
    from tests import grammar_ref as gr
    a, x = wc.tiny_automaton(), wc.tiny_logits()
    z = wr.weighted(a, np.zeros(len(a["src"])), np.zeros(a["S"]))
    got, want = wr.search(x, wc.TINY_LENS, [z], wc.TINY_CANON), gr.search(x, wc.TINY_LENS, [a], wc.TINY_CANON)
    assert np.allclose(got["logp"], want["logp"], atol=1e-12) and np.allclose(got["best"], want["best"], atol=1e-12)


def test_gradient_equals_central_differences():
    a, x = wc.tiny_automaton(), wc.tiny_logits()
    for b, n in ((0, 5), (3, 4), (2, 1)):
        lnz, g = wr.gradient(x[:, b], n, a, wc.TINY_CANON)
        assert abs(lnz - wr.search(x[:, b:b + 1], [n], [a], wc.TINY_CANON)["logp"][0, 0]) < 1e-12
        assert np.abs(g[:n].sum(axis=1)).max() < 1e-12 and not g[n:].any()          # every weight counted once: the rows sum to 0
        h = 1e-6
        for t, v in itertools.product(range(n), range(4)):
            xp, xm = x[:, b].copy(), x[:, b].copy()
            xp[t, v] += h
            xm[t, v] -= h
            d = (wr.gradient(xp, n, a, wc.TINY_CANON)[0] - wr.gradient(xm, n, a, wc.TINY_CANON)[0]) / (2 * h)
            assert abs(d - g[t, v]) < 1e-8, (b, t, v, d, g[t, v])


def test_beam_restatement_equals_brute_force_when_the_beam_holds_everything():
    c = wc.beam_case("brute")
    g = c.grammars[0]
    a = wr.from_grammar(g)
    cls = classes_of(4)
    ref = wc.beam_reference("brute")
    for b, n in enumerate(c.lens):
        _, _, labs = wr.brute_force(c.x[:n, b], a)
        want = sorted(((lp + wm, list(lab)) for lab, (lp, _, wm) in labs.items()), key=lambda h: -h[0])
        got = ref[b].hyps
        assert len(got) == min(c.nbest, len(want))
        for h, (tot, lab) in zip(got, want):
            assert h[0] == lab and abs(h[1] - tot) < 1e-11 and abs(h[4] - g.weight_of(lab)) < 1e-12, (b, h, tot, lab)
            assert abs(wr.path_weights(a, lab, cls)[1] - h[4]) < 1e-6


# ------------------------------------------------------------------------------------------------ weight_of, exhaustively
def _strings(n_sym=3, upto=5):
    for L in range(upto + 1):
        for s in itertools.product(range(1, n_sym + 1), repeat=L):
            yield list(s)


def _occurrences(s, p):
    return sum(1 for i in range(len(s) - len(p) + 1) if s[i:i + len(p)] == p)


def test_boost_weighs_every_string_by_its_occurrences():
    al = wc.letters(4)
    phrases = [[1, 2], [2, 1], [1, 2, 1], [1, 1], [3]]                       # overlapping, one inside another, a repeated symbol
    bonus = [1.0, -0.5, 0.75, 1.25, 0.125]
    g = Grammar.boost(al, phrases, bonus)
    assert g.weighted and all(g.accept) and (g.dense_tables()[1] == 0).all()
    for s in _strings():
        want = sum(b * _occurrences(s, p) for p, b in zip(phrases, bonus))
        assert abs(g.weight_of(s) - want) < 1e-12, (s, g.weight_of(s), want)
    one = Grammar.boost(al, ["ab"], 2.0)                                    # a float: the same bonus for every phrase
    assert one.weight_of("abab") == 4.0 and one.weight_of("ba") == 0.0
    nxt, _ = one.dense_tables()
    logw, fin = one.dense_weights()
    s = int(nxt[0, 1])
    assert logw[0, 1] == 1.0 and fin[s] == -1.0                             # half the phrase: half the bonus, paid back at the end
    with pytest.raises(ValueError):
        Grammar.boost(al, ["ab"], [1.0, 2.0])
    with pytest.raises(ValueError):
        Grammar.boost(al, ["ab"], float("nan"))
    with pytest.raises(ValueError):
        Grammar.boost(al, [""], 1.0)


def test_from_words_gives_every_word_its_weight():
    al = wc.letters(4)
    words = [[1], [1, 2], [1, 2, 3], [2, 2], [3, 1, 1, 2, 3], [2]]
    w = [-0.5, -2.25, 0.75, -1.0, -3.5, 0.0]
    g = Grammar.from_words(al, words, w)
    assert g.weighted
    for s in _strings():
        want = w[words.index(s)] if s in words else None
        assert g.weight_of(s) == want and g.accepts(s) == (want is not None), (s, g.weight_of(s), want)
    nxt, _ = g.dense_tables()
    logw, _ = g.dense_weights()
    assert logw[0, 1] == 0.75 and logw[0, 3] == -3.5 and logw[0, 2] == 0.0   # the look-ahead: the best word below each child
    assert Grammar.from_words(al, words).weight_of([1, 2]) == 0.0 and not Grammar.from_words(al, words).weighted
    with pytest.raises(ValueError):
        Grammar.from_words(al, words, w[:-1])
    with pytest.raises(ValueError):
        Grammar.from_words(al, words, [float("inf")] + w[1:])


def test_from_ngram_scores_as_the_lm_does():
    lm = gc.field_lm()
    al = gc.field_alphabet()
    g = Grammar.from_ngram(lm)
    assert g.weighted and all(g.accept) and g.alphabet is al
    f32 = lambda v: float(np.float32(v))
    for s in _strings(3, 5):
        st, want = lm.start, 0.0
        for c in s:
            want += f32(lm.logp[st, c])
            st = int(lm.next[st, c])
        want += f32(lm.eos[st])
        assert abs(g.weight_of(s) - want) < 1e-12, (s, g.weight_of(s), want)
    half = Grammar.from_ngram(lm, scale=0.5)
    assert abs(half.weight_of([1, 2]) - 0.5 * g.weight_of([1, 2])) < 1e-6
    d = Grammar.from_ngram(lm, dense_only=True)
    assert d.arc_src is None and np.array_equal(d.dense_weights()[0], g.dense_weights()[0])
    with pytest.raises(ValueError, match="dense tables alone"):
        pack_grammars([d], "cpu")
    big = wc.lm6()
    with pytest.raises(ValueError, match=r"\d+ states \+ \d+ arcs"):
        Grammar.from_ngram(big)
    assert Grammar.from_ngram(big, dense_only=True).n_states > 1


# ------------------------------------------------------------------------------------------------ minimisation, validation, packing
def test_weighted_minimisation_keeps_language_and_weights():
    al = wc.letters(4)
    # states 1 and 2 are equivalent with equal weights (merged); 3 and 4 have the same language but different weights (kept apart)
    trans = [{1: 1, 2: 2, 3: 3}, {1: 5, 2: 4}, {1: 5, 2: 4}, {2: 5}, {2: 5}, {}, {1: 5}]
    tw = [{1: 0.5, 2: 0.5, 3: 1.0}, {1: -1.0, 2: 0.0}, {1: -1.0, 2: 0.0}, {2: 0.25}, {2: 0.75}, {}, {1: 9.0}]
    acc = [False, False, False, False, False, True, False]                  # state 6 is unreachable
    fw = [0.0, 0.0, 0.0, 0.0, 0.0, 0.125, 0.0]

    def walk(s):
        st, w = 0, 0.0
        for c in s:
            if c not in trans[st]:
                return None
            w += tw[st][c]
            st = trans[st][c]
        return w + fw[st] if acc[st] else None

    g = Grammar(al, trans, acc, arc_w=tw, final_w=fw)
    assert g.n_states == 5                                                  # 0, {1, 2}, 3, 4, 5
    for s in _strings():
        assert g.weight_of(s) == walk(s), (s, g.weight_of(s), walk(s))
    r = Grammar.from_dfa(al, [{"a": 1}, {}], [False, True], arc_weights=[{"a": 1.5}, {}], final_weights=[7.0, -0.5])
    assert r.weight_of("a") == 1.0 and r.final_logw.tolist() == [0.0, -0.5]   # a final weight is read for accepting states only
    assert Grammar.from_regex(al, "ab*").weight_of("abb") == 0.0 and Grammar.from_regex(al, "ab*").weight_of("b") is None


def test_weights_are_validated():
    al = wc.letters(4)
    t, a = [{"a": 1}, {"b": 1}], [False, True]
    ok = dict(arc_weights=[{"a": 0.5}, {"b": -0.5}], final_weights=[0.0, 1.0])
    assert Grammar.from_dfa(al, t, a, **ok).weight_of("abb") == 0.5
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            Grammar.from_dfa(al, t, a, arc_weights=[{"a": bad}, {"b": 0.0}], final_weights=[0.0, 1.0])
        with pytest.raises(ValueError, match="finite"):
            Grammar.from_dfa(al, t, a, arc_weights=ok["arc_weights"], final_weights=[0.0, bad])
    assert Grammar.from_dfa(al, t, a, arc_weights=ok["arc_weights"], final_weights=[float("nan"), 1.0]).weighted    # not accepting: unread
    with pytest.raises(ValueError, match="go together"):
        Grammar.from_dfa(al, t, a, arc_weights=ok["arc_weights"])
    with pytest.raises(ValueError, match="go together"):
        Grammar.from_dfa(al, t, a, final_weights=ok["final_weights"])
    with pytest.raises(ValueError):
        Grammar.from_dfa(al, t, a, arc_weights=ok["arc_weights"][:1], final_weights=ok["final_weights"])
    with pytest.raises(ValueError):
        Grammar.from_dfa(al, t, a, arc_weights=ok["arc_weights"], final_weights=[0.0])
    with pytest.raises(ValueError):
        Grammar.from_dfa(al, t, a, arc_weights=[{"a": 0.5}, {}], final_weights=ok["final_weights"])


def test_packs_carry_weights_only_when_a_member_has_them():
    al = wc.letters(4)
    plain, heavy = Grammar.from_regex(al, "ab*"), Grammar.from_words(al, ["ab", "c"], [-1.0, -2.0])
    assert "arc_logw" not in pack_grammars([plain], "cpu") and "logw" not in pack_dense_grammars([plain], "cpu")
    p = pack_grammars([plain, heavy], "cpu")
    assert p["arc_logw"].numel() == plain.n_arcs + heavy.n_arcs + 1 and p["final_logw"].numel() == plain.n_states + heavy.n_states
    assert not p["arc_logw"][:plain.n_arcs].any() and np.array_equal(p["arc_logw"][plain.n_arcs:-1].numpy(), heavy.arc_logw)
    d = pack_dense_grammars([plain, heavy], "cpu")
    assert tuple(d["logw"].shape) == tuple(d["next"].shape) and d["final"].numel() == d["dist"].numel()
    assert not d["logw"][:plain.n_states].any() and np.array_equal(d["logw"][plain.n_states:].numpy(), heavy.dense_weights()[0])


# ------------------------------------------------------------------------------------------------ the C entries, no launch
def test_workspace_queries_and_host_checks():
    from vistaocr_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    q, qg = lib.vocr_ctc_grammar_weighted_workspace_bytes, lib.vocr_ctc_grammar_grad_weighted_workspace_bytes
    assert q(12, 4, 13, 2, 10, 30, 1) == lib.vocr_ctc_grammar_workspace_bytes(12, 4, 13, 2, 10, 30, 1) > 0
    assert qg(12, 4, 13, 2, 10, 30, 0) == lib.vocr_ctc_grammar_grad_workspace_bytes(12, 4, 13, 2, 10, 30, 0) > 0
    assert qg(12, 4, 13, 2, 10, 30, 1) == lib.vocr_ctc_grammar_grad_workspace_bytes(12, 4, 13, 2, 10, 30, 1) + 2 * 30 * 4   # the mirrored weights
    for bad in ((0, 4, 13, 2, 10, 30), (12, 4, 257, 2, 10, 30), (12, 4, 13, 0, 10, 30), (12, 4, 13, 2, 4000, 4193), (12, 4, 1, 2, 10, 30)):
        assert q(*bad, 1) == 0 and qg(*bad, 1) == 0, bad
    err = lambda: lib.vocr_last_error()
    sc = lambda aw, fw, **k: lib.vocr_ctc_grammar_scores_weighted(one, one, 12, 4, 13, None, one, one, k.get("g", 2), one, one, one, one, aw, fw,
                                                                 10, k.get("ma", 30), one, None, None, None, 0, one, k.get("ws", 1 << 30), None)
    assert sc(one, None) == -1 and b"vocr_ctc_grammar_scores_weighted: arc_logw and final_logw go together" in err()
    assert sc(None, one) == -1 and b"go together" in err()
    assert sc(one, one, ws=16) == -1 and b"vocr_ctc_grammar_scores_weighted: workspace too small" in err()
    assert sc(None, None, ws=16) == -1 and b"vocr_ctc_grammar_scores_weighted: workspace too small" in err()
    assert sc(one, one, g=0) == -1 and sc(one, one, ma=9000) == -1
    gd = lambda aw, fw, **k: lib.vocr_ctc_grammar_grad_weighted(one, one, 12, 4, 13, None, one, one, 2, one, one, one, one, aw, fw, 10, 30, one,
                                                               k.get("w", one), one, k.get("dl", one), one, k.get("ws", 1 << 30), None)
    assert gd(one, None) == -1 and b"vocr_ctc_grammar_grad_weighted: arc_logw and final_logw go together" in err()
    assert gd(one, one, ws=qg(12, 4, 13, 2, 10, 30, 1) - 1) == -1 and b"workspace too small" in err()
    assert gd(one, one, dl=None) == -1 and b"weights and dlogits go together" in err()
    bm = lambda lw, fn, **k: lib.vocr_ctc_grammar_beam_search_weighted(one, one, 12, 4, 13, None, k.get("K", 16), 4, one, one, one, lw, fn, 1, one,
                                                                      None, None, None, 0, 0, 0.0, k.get("gw", 1.0), 0.0, float("-inf"),
                                                                      one, one, one, None, one, k.get("ws", 1 << 30), None)
    assert bm(one, None) == -1 and b"vocr_ctc_grammar_beam_search_weighted: dfa_logw and dfa_final go together" in err()
    assert bm(None, one) == -1 and b"go together" in err()
    assert bm(one, one, gw=float("nan")) == -1 and b"grammar_weight must be finite" in err()
    assert bm(one, one, gw=float("inf")) == -1
    assert bm(one, one, K=129) == -1 and b"vocr_ctc_grammar_beam_search_weighted" in err()
    assert bm(one, one, ws=12 * 4 * 16 * 8 - 1) == -1 and b"workspace too small" in err()


# ------------------------------------------------------------------------------------------------ what the GPU tests rely on
@pytest.mark.parametrize("name", wc.BEAM_NAMES)
def test_beam_references_are_decided(name):
    """At most 1/8 of a case's lines lie within TAU of a neighbouring rank, by the restatement alone."""
    c, ref = wc.beam_case(name), wc.beam_reference(name)
    B = len(ref)
    assert 8 * (B - len(wc.decided(ref))) <= B, (name, [r.gap for r in ref])
    assert all(r.hyps for r in ref) or name == "dense", name


@pytest.mark.parametrize("name", sorted(wc.GUARDED_BEAM))
def test_guarded_beam_references_are_decided(name):
    ref = wc.guarded_beam_reference(name)
    B = len(ref)
    assert 8 * (B - len(wc.decided(ref))) <= B, (name, [r.gap for r in ref])


def test_as_given_tables_must_be_trimmed():
    al = wc.letters(4)
    ok = Grammar(al, [{1: 1}, {}], [False, True], arc_w=[{1: 0.5}, {}], final_w=[0.0, 1.0], as_given=True)
    assert ok.n_states == 2 and ok.weight_of([1]) == 1.5
    with pytest.raises(ValueError, match="trimmed"):                        # state 2 is unreachable
        Grammar(al, [{1: 1}, {}, {1: 1}], [False, True, False], arc_w=[{1: 0.5}, {}, {1: 0.0}], final_w=[0.0, 1.0, 0.0], as_given=True)
    with pytest.raises(ValueError, match="trimmed"):                        # state 2 is a dead end
        Grammar(al, [{1: 1, 2: 2}, {}, {}], [False, True, False], arc_w=[{1: 0.5, 2: 0.0}, {}, {}], final_w=[0.0, 1.0, 0.0], as_given=True)


def test_the_boosted_line_changes_its_reading():
    """Without the boost the 1-best is not the phrase; with it it is - with and without the 6-gram, each by more than TAU."""
    al, _ = wc.bc.english()
    want = [al.char_to_idx["u%04x" % ord(ch)] for ch in wc.BOOST_PHRASE]
    for name in ("boost", "boost_lm"):
        c = wc.beam_case(name)
        off, on = wc.beam_references(c, gw=0.0), wc.beam_reference(name)
        assert off[0].hyps[0][0] != want and on[0].hyps[0][0] == want and min(off[0].gap, on[0].gap) >= wc.TAU, (name, off, on)
        assert abs(on[0].hyps[0][4] - 3.0) < 1e-6


def test_sweep_cases_reach_their_branches():
    s3, s1 = wc.stage_seams()
    assert 2049 < s3 < s1 < 8192
    assert [wc.staging(*wc.tree_sizes(N)) for N in (2048, s3, s3 + 1, s1, s1 + 1, 8192)] == [3, 3, 1, 1, 0, 0]
    for name in wc.sweep_names():
        c = wc.sweep_case(name)
        ref = wr.search(c.x, c.lens, c.automata, c.canon)
        assert np.isfinite(ref["logp"]).any(), name


def test_bars_are_four_times_the_recorded_error_rounded_up():
    assert wc.one_digit_up(4 * 2.1e-6) == pytest.approx(9e-6) and wc.one_digit_up(4 * 2.5e-5) == pytest.approx(1e-4)
    assert wc.bars((3e-4, 0.0)) == (1e-3, 0.0)
