"""CPU: the fp64 restatement of the grammar-constrained beam search (tests/grammar_beam_ref.py) held to brute force, to the
unconstrained restatement (tests/beam_ref.py) under the automaton that accepts everything, and to the edge cases of the distance
rule; Grammar.dense_tables / pack_dense_grammars; the entry's host checks that need no device; and, from the restatement alone, the
floors of compared lines that pin the inputs of tests/test_grammar_beam_gpu.py (tests/grammar_beam_cases.py)."""
import ctypes

import numpy as np
import pytest

import vistaocr_amd as va
from tests import beam_ref as br
from tests import grammar_beam_cases as gc
from tests import grammar_beam_ref as gbr
from vistaocr_amd.grammar import Grammar, pack_dense_grammars


def test_brute_force():
    """V = 4, T = 6, `1 (2|3)* 1`, K = 128, nbest = 8, N(0, 2) logits, 30 seeds: the beam holds every viable prefix, so labels and
    order are brute force's filtered by Grammar.accepts, scores within 1e-9."""
    g = gc.tiny_grammar()
    tables = g.dense_tables()
    for seed in range(30):
        x = gc.tiny_logits(seed)
        want = gc.tiny_brute(seed)[:8]
        assert all(g.accepts(h[0]) for h in want)
        got, _ = gbr.beam_search(x, 6, tables, 128, nbest=8)
        assert [h[0] for h in got] == [h[0] for h in want], seed
        assert len(got) == 8
        for a, b in zip(got, want):
            assert np.allclose(a[1:], b[1:], rtol=0, atol=1e-9), seed


@pytest.mark.parametrize("with_lm", [False, True])
def test_sigma_star_is_the_unconstrained_search(with_lm):
    """The one-state automaton that accepts everything: hypotheses, scores and decision gaps are beam_ref.beam_search's, exactly."""
    al, canon = gc.bc.english()
    lm = gc.bc.char_lm5() if with_lm else None
    alpha, beta = (0.8, 0.5) if with_lm else (0.0, 0.0)
    rng = np.random.default_rng(11)
    V = len(canon)
    tables = gbr.sigma_star(V, canon)
    for K, nbest, L in ((1, 1, 12), (5, 3, 12), (16, 4, 9), (16, 16, 0)):
        x = rng.normal(0, 3, size=(12, V))
        for prune in (None, -4.0):
            a = br.beam_search(x, L, K, nbest=nbest, canon=canon, lm=lm, alpha=alpha, beta=beta, prune=prune)
            b = gbr.beam_search(x, L, tables, K, nbest=nbest, canon=canon, lm=lm, alpha=alpha, beta=beta, prune=prune)
            assert a == b, (K, nbest, L, prune)
    g = Grammar.from_regex(al, ".*")
    nxt, dist = g.dense_tables()
    assert np.array_equal(nxt, tables[0]) and np.array_equal(dist, tables[1])


def test_edge_cases_of_the_distance_rule():
    al = gc.letters(4)
    x = np.random.default_rng(3).normal(0, 2, size=(6, 4))
    five = Grammar.from_labels(al, [1, 2, 3, 1, 2]).dense_tables()
    assert gbr.beam_search(x[:4], 4, five, 16, nbest=4)[0] == []               # five symbols, four frames
    assert [h[0] for h in gbr.beam_search(x[:5], 5, five, 16, nbest=4)[0]] == [[1, 2, 3, 1, 2]]
    twice = Grammar.from_labels(al, [1, 1]).dense_tables()
    assert gbr.beam_search(x[:2], 2, twice, 16, nbest=4)[0] == []              # `1 1` needs a blank between: three frames
    h = gbr.beam_search(x[:3], 3, twice, 16, nbest=4)[0]
    assert [q[0] for q in h] == [[1, 1]] and abs(h[0][2] - br.ctc_logprob(br.class_logprobs(x[:3]), [1, 1])) < 1e-12
    empty = Grammar.from_labels(al, []).dense_tables()
    assert [q[0] for q in gbr.beam_search(x, 6, empty, 16, nbest=4)[0]] == [[]]
    assert [q[0] for q in gbr.beam_search(x, 0, empty, 16, nbest=4)[0]] == [[]]
    assert gbr.beam_search(x, 0, twice, 16, nbest=4)[0] == []                  # no frames: the empty labelling iff state 0 accepts
    # poisoned tables: a next state outside the automaton is no arc, a negative distance cannot accept
    nxt, dist = (a.copy() for a in gc.tiny_grammar().dense_tables())
    bad = nxt.copy()
    bad[bad >= 0] = 99
    assert gbr.beam_search(x, 6, (bad, dist), 16)[0] == []
    assert gbr.beam_search(x, 6, (nxt, np.full_like(dist, -1)), 16)[0] == []


def _bfs_dist(trans, accept):
    S = len(trans)
    dist = np.full(S, -1)
    for s in range(S):
        seen, frontier, d = {s}, [s], 0
        while frontier and dist[s] < 0:
            if any(accept[q] for q in frontier):
                dist[s] = d
                break
            frontier = [n for q in frontier for n in trans[q].values() if n not in seen and not seen.add(n)]
            d += 1
    return dist


def test_dense_tables():
    al = va.english_alphabet()
    canon = al.canonical_indices()
    rng = np.random.default_rng(5)
    grammars = [Grammar.from_regex(al, r"\d\d-\d\d"), Grammar.from_regex(al, r"(ab|cd)*e?"), Grammar.from_words(al, ["cat", "car", "dog", "-"]),
                Grammar.contains(al, "ab"), Grammar.from_labels(al, [])]
    for g in grammars:
        nxt, dist = g.dense_tables()
        trans, accept = g.dfa()
        assert nxt.dtype == np.int32 and dist.dtype == np.int32 and nxt.shape == (g.n_states, len(al)) and dist.shape == (g.n_states,)
        assert (nxt[:, [v for v in range(len(al)) if canon[v] != v or v == 0]] == -1).all()          # non-canonical columns, the blank
        assert int((nxt >= 0).sum()) == g.n_arcs and nxt.max() < g.n_states
        assert np.array_equal(dist == 0, np.asarray(accept)) and np.array_equal(dist, _bfs_dist(trans, accept))
        symbols = sorted({c for row in trans for c in row})
        for _ in range(200):                                                     # walking the table is Grammar.accepts
            y = [int(c) for c in rng.choice(symbols, size=rng.integers(0, 7))] if symbols else []
            s = 0
            for c in y:
                s = nxt[s, c] if s >= 0 else -1
            assert (s >= 0 and dist[s] == 0) == g.accepts(y), (g.name, y)
    none = Grammar.from_dfa(al, [{}], [False])                                   # the empty language: the start alone, unreachable
    assert none.dense_tables()[1].tolist() == [-1]


def test_pack_dense_grammars_and_the_cell_limit():
    al = va.english_alphabet()
    a, b = Grammar.from_regex(al, r"\d\d-\d\d"), Grammar.from_words(al, ["cat", "dog"])
    p = pack_dense_grammars([a, b], "cpu")
    assert p["state_off"].tolist() == [0, a.n_states, a.n_states + b.n_states] and p["num_grammars"] == 2
    assert tuple(p["next"].shape) == (a.n_states + b.n_states, len(al)) and p["next"].dtype == p["dist"].dtype == p["state_off"].dtype
    assert np.array_equal(p["next"][a.n_states:].numpy(), b.dense_tables()[0])  # local state numbers
    with pytest.raises(ValueError, match=r"%d states x %d symbols.*max_table_bytes=1000" % (a.n_states + b.n_states, len(al))):
        pack_dense_grammars([a, b], "cpu", max_table_bytes=1000)
    with pytest.raises(ValueError):
        pack_dense_grammars([], "cpu")
    big, words = gc.big_trie()
    assert big.n_states + big.n_arcs > va.ops.GRAMMAR_CELLS_MAX and len(words) >= 2500  # beyond the sweep kernels, and it packs
    assert pack_dense_grammars([big], "cpu")["num_states"] == big.n_states
    with pytest.raises(ValueError, match="no grammar"):
        va.GrammarBeamDecoder(al, [])
    with pytest.raises(ValueError, match="nbest <= beam"):
        va.GrammarBeamDecoder(al, a, beam=4, nbest=5)


def test_which_is_the_grammar_decoders_alone():
    """The search decoders share their public methods, which hand `which=` to the decoder's own search as it came: a decoder whose
    search takes no such argument refuses it with a TypeError, and `lang=` is refused under the decoder's own name - both before any
    device is touched."""
    import torch
    al = va.english_alphabet()
    x = torch.zeros(4, 1, len(al))
    for method in ("decode", "decode_nbest", "decode_aligned", "decode_alternatives"):
        with pytest.raises(TypeError, match="which"):
            getattr(va.BeamDecoder(al), method)(x, [4], which=[0])
    with pytest.raises(ValueError, match=r"^BeamDecoder: one alphabet per decoder \(lang is not supported\)$"):
        va.BeamDecoder(al).decode(x, [4], lang="en")
    with pytest.raises(ValueError, match=r"^GrammarBeamDecoder: one alphabet per decoder \(lang is not supported\)$"):
        va.GrammarBeamDecoder(al, Grammar.from_regex(al, r"\d")).decode(x, [4], lang="en", which=[0])
    with pytest.raises(ValueError, match=r"^BeamDecoder: need 1 <= nbest <= beam <= 128 \(beam=129 nbest=1\)$"):
        va.BeamDecoder(al, beam=129)


def test_host_checks_without_a_device():
    from vistaocr_amd import _lib
    lib = _lib.load()
    ws = lib.vocr_ctc_grammar_beam_workspace_bytes
    assert ws(294, 32, 96, 16, 1) == 294 * 32 * 16 * 8 == lib.vocr_ctc_beam_workspace_bytes(294, 32, 96, 16, 1)
    assert ws(294, 32, 257, 16, 1) == 0 and ws(294, 32, 96, 129, 1) == 0 and ws(294, 32, 96, 8, 9) == 0 and ws(0, 32, 96, 8, 1) == 0
    one = ctypes.c_void_p(16)
    need = ws(10, 2, 96, 8, 2)

    def call(g=1, tables=(one, one, one), which=one, nbytes=need, beam=8, nbest=2, lm=(None, None, None), w=0.0):
        return lib.vocr_ctc_grammar_beam_search(one, one, 10, 2, 96, None, beam, nbest, tables[0], tables[1], tables[2], g, which,
                                                lm[0], lm[1], lm[2], 0, 0, w, 0.0, float("-inf"), one, one, one, one, nbytes, None)

    assert call(g=0) == -1 and b"g >= 1" in lib.vocr_last_error()
    for k in range(3):
        assert call(tables=tuple(None if i == k else one for i in range(3))) == -1 and b"null automaton table" in lib.vocr_last_error()
    assert call(which=None) == -1
    assert call(nbytes=need - 1) == -1 and b"workspace too small" in lib.vocr_last_error()
    assert call(beam=129) == -1 and call(nbest=9) == -1 and call(lm=(one, None, None)) == -1 and call(w=float("nan")) == -1


def test_the_pinned_gpu_inputs_have_their_floors():
    """What pins tests/test_grammar_beam_gpu.py's dense and trie cases, from the restatement alone: at least 3/4 of the lines of every
    case are decided by TAU or more, and every compared line has a hypothesis."""
    for name in gc.DENSE + gc.TRIE:
        case, ref = gc.case(name), gc.reference(name)
        lines = gc.decided(ref)
        assert 4 * len(lines) >= 3 * case.x.shape[1], (name, len(lines))
        assert all(ref[b].hyps for b in lines), name
