"""CPU: the fp64 restatement of tests/grammar_grad_ref.py held to central differences of tests/grammar_ref.py's ln P, to the brute force
over all frame paths and to the CTC references on chains; Grammar.from_template / from_labels against an independent matcher; the host
logic of GrammarCTCLoss and of the chunking with the op stubbed; and the argument validation of vocr_ctc_grammar_grad /
vocr_ctc_grammar_grad_workspace_bytes, which needs no GPU."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import align_ref as ar
from tests import ctc_ref as cr
from tests import grammar_grad_ref as gg
from tests import grammar_ref as gr
from tests import nbest_ref as nr

NEG = -np.inf
CANON_PAIR = [0, 1, 1, 3, 4, 3]            # columns 1, 2 are one class, and 3, 5


def _dfa(V):
    # a(b|c)*d | c
    return gr.make(4, [(0, 1, 1), (1, 2, 1), (1, 3, 1), (1, 4, 2), (0, 3, 3)], [2, 3], V=V)


def _nfa(V):
    # two arcs with the same (src, class); (dst, class) groups of two arcs; a cycle
    return gr.make(4, [(0, 1, 1), (0, 1, 2), (1, 2, 3), (2, 2, 3), (2, 3, 3), (1, 3, 3), (3, 1, 3), (0, 2, 3), (3, 4, 0)], [3], V=V)


def _classes(V, canon):
    # arc classes given as members: 2 stands for class 1, 5 for class 3
    return gr.make(3, [(0, 2, 1), (1, 5, 1), (1, 4, 2), (0, 4, 2), (2, 1, 2)], [2], V=V, canon=canon)


@pytest.mark.parametrize("kind", ["dfa", "nfa", "classes"])
def test_gradient_equals_central_differences_of_the_older_restatement(kind):
    """h = 1e-5 in fp64 on grammar_ref.search's ln P, every element; 1e-6 of the line's largest element (truncation h^2 |f'''| / 6 and
    rounding 1e-16 |ln P| / h are both about 1e-10: slack, not tuning)"""
    T, V, h = 7, 6, 1e-5
    canon = CANON_PAIR if kind == "classes" else None
    a = {"dfa": _dfa, "nfa": _nfa}[kind](V) if canon is None else _classes(V, canon)
    rng = np.random.default_rng(["dfa", "nfa", "classes"].index(kind))
    lens = [7, 5, 6]
    x = rng.normal(0, 1.5, (T, 3, V))
    x[:, 2, {"dfa": 2, "nfa": 4, "classes": 5}[kind]] = -np.inf    # a dead column on the last line (classes: one member of a class)
    r = gg.run(x, lens, [a], [0, 0, 0], canon)
    assert np.isfinite(r["logp"]).all()
    assert np.allclose(r["logp"], gr.search(x, lens, [a], canon)["logp"][:, 0], rtol=0, atol=1e-12)
    assert np.allclose(r["occ"].sum(2)[:5], 1.0, atol=1e-12)       # the occupancies of a frame sum to 1
    for b, n in enumerate(lens):
        num = np.zeros((T, V))
        for t in range(n):
            for v in range(V):
                if not np.isfinite(x[t, b, v]):
                    continue
                xp, xm = x[:, b:b + 1].copy(), x[:, b:b + 1].copy()
                xp[t, 0, v] += h
                xm[t, 0, v] -= h
                num[t, v] = (gr.search(xp, [n], [a], canon)["logp"][0, 0] - gr.search(xm, [n], [a], canon)["logp"][0, 0]) / (2 * h)
        top = float(np.abs(r["grad"][:, b]).max())
        assert top > 1e-3
        assert float(np.abs(r["grad"][:, b] - num).max()) <= 1e-6 * top, (kind, b, float(np.abs(r["grad"][:, b] - num).max()), top)
        assert float(np.abs(r["grad"][n:, b]).max() if n < T else 0.0) == 0.0
        assert float(np.abs(r["grad"][:, b][~np.isfinite(x[:, b])]).max() if not np.isfinite(x[:, b]).all() else 0.0) == 0.0


def test_weights_scale_the_rows_and_bad_lines_are_zero():
    T, V = 6, 5
    a, bad = _dfa(V), dict(_dfa(V), cls=np.array([0, 2, 3, 4, 3], dtype=np.int32))      # an arc on the blank
    assert not gr.valid(bad, V, ar.classes_of(V), 4, 5)
    x = np.random.default_rng(4).normal(0, 1, (T, 5, V))
    x[:, 4, 1] = x[:, 4, 3] = -np.inf                              # no accepted path is left on the last line
    one = gg.run(x, [6] * 5, [a, bad], [0, 1, -1, 2, 0])
    w = np.array([-2.0, 1.0, 1.0, 1.0, 3.0])
    r = gg.run(x, [6] * 5, [a, bad], [0, 1, -1, 2, 0], None, w)
    assert np.isfinite(r["logp"][0]) and (r["logp"][1:] == NEG).all()
    assert np.array_equal(r["grad"][:, 0], -2.0 * one["grad"][:, 0]) and float(np.abs(r["grad"][:, 1:]).max()) == 0.0


def test_ln_p_equals_the_brute_force_over_all_paths():
    V = 3
    rng = np.random.default_rng(2)
    autos = [gr.make(2, [(0, 1, 1), (1, 2, 0)], [0], V=V), gr.make(3, [(0, 1, 1), (1, 1, 2), (2, 2, 2), (0, 2, 2)], [2], V=V),
             gr.make(1, [(0, 1, 0), (0, 2, 0)], [0], V=V), gr.make(2, [(0, 2, 1)], [1], V=V)]
    for T in (1, 2, 5, 7):
        x = rng.normal(0, 1.5, (T, len(autos), V))
        r = gg.run(x, [T] * len(autos), autos, range(len(autos)))
        for k, a in enumerate(autos):
            want, _ = gr.brute_force(x[:, k], a)
            assert (r["logp"][k] == NEG) == (want == NEG), (T, k)
            if want != NEG:
                assert abs(r["logp"][k] - want) < 1e-12, (T, k, r["logp"][k], want)
    assert abs(r["logp"][2]) < 1e-12                               # sigma star: P = 1


def test_a_chain_is_the_ctc_score_and_gradient():
    T, B, V = 12, 4, 7
    rng = np.random.default_rng(3)
    labs = [[1, 1, 3], [], [2, 5, 2, 6], [4] * 7]                  # the last does not fit 12 frames
    lens = [12, 5, 9, 12]
    x = rng.normal(0, 2, (T, B, V)).astype(np.float32)
    autos = [gr.make(len(l) + 1, [(i, c, i + 1) for i, c in enumerate(l)], [len(l)]) for l in labs]
    w = np.array([1.5, -1.0, 2.0, 1.0])
    r = gg.run(x, lens, autos, range(B), None, w)
    scores, grad = nr.nbest(torch.from_numpy(x), lens, [[l] for l in labs], None, w.reshape(B, 1))
    scores = scores.numpy()[:, 0]
    assert r["logp"][3] == NEG and scores[3] == NEG
    assert np.allclose(r["logp"][:3], scores[:3], rtol=0, atol=1e-12)
    assert float(np.abs(r["grad"] - grad.numpy()).max()) < 1e-13
    keep = [0, 1, 2]
    nll, g, _, _ = cr.ctc(torch.from_numpy(x[:, keep]), [v for b in keep for v in labs[b]], [len(labs[b]) for b in keep], [lens[b] for b in keep])
    assert np.allclose(-nll.numpy(), r["logp"][:3], rtol=0, atol=1e-12)
    assert float(np.abs(-g.numpy() * w[:3].reshape(1, 3, 1) - r["grad"][:, :3]).max()) < 1e-13


# ------------------------------------------------------------------------------------------------------------------ from_template
def _alphabet(n):
    import vistaocr_amd as va
    return va.Alphabet(["<ctc-blank>"] + ["u%04x" % (0x61 + i) for i in range(n)])


def _matches(items, lab, ANY, GAP, every):
    """an independent matcher: backtracking over the items"""
    if not items:
        return not lab
    it, rest = items[0], items[1:]
    if it is GAP:
        return any(all(v in every for v in lab[:k]) and _matches(rest, lab[k:], ANY, GAP, every) for k in range(len(lab) + 1))
    if not lab:
        return False
    if it is ANY:
        ok = lab[0] in every
    elif isinstance(it, (set, frozenset, list, tuple)):
        ok = lab[0] in [ord(v) - 0x60 if isinstance(v, str) else v for v in it]
    else:
        ok = lab[0] == (ord(it) - 0x60 if isinstance(it, str) else it)
    return ok and _matches(rest, lab[1:], ANY, GAP, every)


def _is_minimal_dfa(g, depth):
    """deterministic; every state reachable and live; no two states with the same language (suffixes up to `depth`, which separates the
    states of an automaton with at most depth + 1 of them)"""
    trans, accept = g.dfa()
    arcs = list(zip(g.arc_src.tolist(), g.arc_cls.tolist(), g.arc_dst.tolist()))
    assert len(set((s, c) for s, c, _ in arcs)) == len(arcs)
    assert arcs == sorted(arcs, key=lambda a: (a[2], a[1], a[0]))
    seen, todo = {0}, [0]
    while todo:
        for d in trans[todo.pop()].values():
            if d not in seen:
                seen.add(d)
                todo.append(d)
    assert seen == set(range(g.n_states))
    classes = sorted({c for row in trans for c in row})
    lang = []
    for s in range(g.n_states):
        words = set()
        for n in range(depth + 1):
            for wd in itertools.product(classes, repeat=n):
                q = s
                for c in wd:
                    q = trans[q].get(c)
                    if q is None:
                        break
                if q is not None and accept[q]:
                    words.add(wd)
        lang.append(frozenset(words))
    assert all(lang) or g.n_states == 1                            # live: every state accepts something
    assert len(set(lang)) == g.n_states


def test_from_template_accepts_what_an_independent_matcher_accepts():
    from vistaocr_amd import Grammar
    AL = _alphabet(4)
    A, G = Grammar.ANY, Grammar.GAP
    templates = [[1, 2, G, 3, 4], [G, 1, 2], [1, 2, G], [G], [A], [], [1, {2, 3}, A, [4, "a"]], [1, G, 1], [1, 1, G, 1, 1], [G, "b", G, A],
                 [G, G, 3], [A, A, G], ["a", "b", G, "c", "d"], [G, 1, A, 2], [{1, 2}, G, {1, 2}]]
    labellings = [list(l) for n in range(6) for l in itertools.product(range(1, 5), repeat=n)]
    assert len(labellings) == 1365
    for items in templates:
        g = Grammar.from_template(AL, items)
        for lab in labellings:
            assert g.accepts(lab) == _matches(items, lab, A, G, {1, 2, 3, 4}), (items, lab)
        _is_minimal_dfa(g, 4 if g.n_states > 4 else 3)
        assert g.n_states <= 6
    g = Grammar.from_template(AL, [G])
    assert g.n_states == 1 and g.n_arcs == 4 and bool(g.accept[0])
    # exclude: ANY and GAP do not stand for a reserved symbol
    g = Grammar.from_template(AL, [1, G, A], exclude=[4])
    for lab in labellings:
        assert g.accepts(lab) == _matches([1, G, A], lab, A, G, {1, 2, 3}), lab
    assert 4 not in g.arc_cls.tolist()
    with pytest.raises(ValueError, match="not one character"):
        Grammar.from_template(AL, ["ab"])
    with pytest.raises(ValueError, match="empty set"):
        Grammar.from_template(AL, [set()])
    with pytest.raises(ValueError, match="not a non-blank alphabet index"):
        Grammar.from_template(AL, [7])


def test_from_labels_is_the_chain():
    from vistaocr_amd import Grammar
    AL = _alphabet(4)
    g = Grammar.from_labels(AL, [1, 1, 3])
    assert g.n_states == 4 and g.n_arcs == 3 and g.accept.tolist() == [0, 0, 0, 1]
    assert (g.arc_src.tolist(), g.arc_cls.tolist(), g.arc_dst.tolist()) == ([0, 1, 2], [1, 1, 3], [1, 2, 3])
    assert g.accepts("aac") and not g.accepts("ac") and not g.accepts("aaca")
    e = Grammar.from_labels(AL, [])
    assert e.n_states == 1 and e.n_arcs == 0 and e.accepts([]) and not e.accepts([1])
    with pytest.raises(ValueError):
        Grammar.from_labels(AL, [0])


def test_an_oversized_template_is_a_value_error_that_names_its_sizes():
    import vistaocr_amd as va
    from vistaocr_amd import Grammar
    AL = va.english_alphabet()
    with pytest.raises(ValueError, match=r"\d+ states \+ \d+ arcs, more than .*8192"):
        Grammar.from_template(AL, [Grammar.GAP, "a"] + [Grammar.ANY] * 7)          # 2^8 states of 94 arcs each
    with pytest.raises(ValueError, match=r"\d+ states \+ \d+ arcs, more than"):
        Grammar.from_template(AL, [Grammar.GAP, "a"] + [Grammar.ANY] * 20)         # stopped inside the subset construction


# ------------------------------------------------------------------------------------------------------------- the criterion's host
def test_criterion_caches_grammars_and_shares_them_between_equal_targets():
    import vistaocr_amd as va
    from vistaocr_amd import Grammar
    AL = _alphabet(6)
    calls = []

    def to_grammar(labels):
        calls.append(labels)
        return Grammar.from_labels(AL, labels)

    crit = va.GrammarCTCLoss(AL, to_grammar, cache_size=3)
    grammars, which = crit.batch_grammars([1, 2, 3, 1, 2, 4, 1, 2], [2, 1, 2, 1, 2])      # (1,2) (3,) (1,2) (4,) (1,2)
    assert which == [0, 1, 0, 2, 0] and len(grammars) == 3 and calls == [(1, 2), (3,), (4,)]
    assert all(isinstance(k, tuple) and all(isinstance(v, int) for v in k) for k in calls)
    assert (crit.cache_misses, crit.cache_hits) == (3, 0)
    grammars2, which2 = crit.batch_grammars([4, 1, 2], [1, 2])
    assert grammars2[0] is grammars[2] and grammars2[1] is grammars[0] and which2 == [0, 1] and len(calls) == 3
    crit.batch_grammars([5], [1])                                                         # a fourth target evicts the oldest: (3,)
    assert len(crit._cache) == 3 and (3,) not in crit._cache and (1, 2) in crit._cache
    crit.batch_grammars([3], [1])
    assert calls[-1] == (3,) and len(calls) == 5
    empty, which3 = crit.batch_grammars([], [0, 0])                                       # the empty target is a target
    assert which3 == [0, 0] and empty[0].n_states == 1 and empty[0].n_arcs == 0


def test_criterion_builders_and_errors():
    import vistaocr_amd as va
    from vistaocr_amd import Grammar, ops
    AL = va.english_alphabet()
    star, q = AL.char_to_idx["u002a"], AL.char_to_idx["u003f"]
    crit = va.GrammarCTCLoss.with_gaps(AL, "*", "?")
    (g,), which = crit.batch_grammars([1, 2, star, 3, q], [5])
    assert g.accepts("abc.") and g.accepts("abzzzcz") and not g.accepts("abc") and not g.accepts("ab*c*") and not g.accepts("abc?")
    assert star not in g.arc_cls.tolist() and q not in g.arc_cls.tolist()
    same = va.GrammarCTCLoss.with_gaps(AL, star, q).batch_grammars([1, 2, star, 3, q], [5])[0][0]
    assert same.dfa() == g.dfa()
    (c,), _ = va.GrammarCTCLoss.exact(AL).batch_grammars([1, 2, 2], [3])
    assert c.dfa() == Grammar.from_labels(AL, "abb").dfa()
    for bad in ("**", "é", 0, len(AL)):
        with pytest.raises(ValueError, match="with_gaps"):
            va.GrammarCTCLoss.with_gaps(AL, bad)
    with pytest.raises(ValueError, match="must differ"):
        va.GrammarCTCLoss.with_gaps(AL, "*", star)
    with pytest.raises(TypeError, match="callable"):
        va.GrammarCTCLoss(AL, None)
    with pytest.raises(ValueError, match="cache_size"):
        va.GrammarCTCLoss(AL, lambda l: None, cache_size=0)
    with pytest.raises(TypeError, match="not a Grammar"):
        va.GrammarCTCLoss(AL, lambda l: "abc").batch_grammars([1], [1])
    rng = np.random.default_rng(0)                                                        # random words: their trie does not fold up
    words = sorted({"".join(chr(0x61 + int(v)) for v in rng.integers(0, 26, 5)) for _ in range(8000)})
    big = Grammar.from_words(AL, words)
    assert big.n_states + big.n_arcs > ops.GRAMMAR_CELLS_MAX
    with pytest.raises(ValueError, match=r"%d states \+ %d arcs" % (big.n_states, big.n_arcs)):
        va.GrammarCTCLoss(AL, lambda l: big).batch_grammars([1], [1])
    crit = va.GrammarCTCLoss.exact(AL)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(torch.zeros(4, 1, len(AL)), torch.tensor([1], dtype=torch.int32), torch.tensor([4], dtype=torch.int32),
             torch.tensor([1], dtype=torch.int32))


def test_pack_batch_is_one_buffer_with_the_tables_of_pack_grammars():
    import vistaocr_amd as va
    from vistaocr_amd import Grammar
    from vistaocr_amd.grammar import pack_grammars
    from vistaocr_amd.grammar_loss import pack_batch
    AL = _alphabet(6)
    grammars = [Grammar.from_labels(AL, [1, 2, 2]), Grammar.from_template(AL, [Grammar.GAP, 3]), Grammar.from_labels(AL, [])]
    packed, which, lens = pack_batch(grammars, [2, 0, 0, 1], [9, 8, 7, 6], torch.device("cpu"))
    want = pack_grammars(grammars, torch.device("cpu"))
    for k in ("state_off", "arc_off", "src", "cls", "dst", "accept"):
        assert packed[k].dtype == torch.int32 and torch.equal(packed[k], want[k]), k
    assert (packed["max_states"], packed["max_arcs"]) == (want["max_states"], want["max_arcs"]) == (4, max(g.n_arcs for g in grammars))
    assert which.tolist() == [2, 0, 0, 1] and lens.tolist() == [9, 8, 7, 6] and which.dtype == lens.dtype == torch.int32


def test_chunk_boundaries_with_the_op_stubbed(monkeypatch):
    """consecutive ranges of as many lines as the limit holds; every call gets the same tables and its own slice; the pieces come back in
    order"""
    from vistaocr_amd import grammar, ops
    T, B, V = 10, 7, 5
    packed = {"max_states": 6, "max_arcs": 14}
    one = ops.grammar_lattice_bytes(T, 1, 6, 14)
    assert one == 10 * 20 * 4
    assert grammar.lattice_chunks(T, B, 6, 14) == [(0, 7)]
    assert grammar.lattice_chunks(T, B, 6, 14, 3 * one) == [(0, 3), (3, 6), (6, 7)]
    assert grammar.lattice_chunks(T, B, 6, 14, 3 * one + one - 1) == [(0, 3), (3, 6), (6, 7)]
    assert grammar.lattice_chunks(T, B, 6, 14, 7 * one) == [(0, 7)] and grammar.lattice_chunks(T, B, 6, 14, one) == [(b, b + 1) for b in range(7)]
    assert grammar.lattice_chunks(T, B, 6, 14, 1 << 40) == [(0, 7)]                      # never beyond the kernel's own limit
    with pytest.raises(ValueError, match="exceed the limit"):
        grammar.lattice_chunks(T, B, 6, 14, one - 1)
    big = grammar.lattice_chunks(2000, 64, 4000, 4192)                                   # 65.5 MB a line: 32 lines fill 2 GiB
    assert big == [(0, 32), (32, 64)]
    seen = []

    def stub(logits, lens, gp, which, canon=None, weights=None):
        assert gp is packed and canon == "canon"
        seen.append((tuple(logits.shape), lens.tolist(), which.tolist(), weights.tolist()))
        return logits[0, :, 0].clone(), logits * 2.0

    monkeypatch.setattr(ops, "ctc_grammar_grad", stub)
    x = torch.arange(T * B * V, dtype=torch.float32).reshape(T, B, V)
    lens, which = torch.arange(B, dtype=torch.int32), torch.arange(B, dtype=torch.int32) % 3
    logp, dl = grammar.grammar_grad_chunked(x, lens, packed, which, "canon", -1.0, 3 * one)
    assert [s[0] for s in seen] == [(T, 3, V), (T, 3, V), (T, 1, V)]
    assert [v for s in seen for v in s[1]] == list(range(B)) and [v for s in seen for v in s[2]] == [0, 1, 2, 0, 1, 2, 0]
    assert all(s[3] == [-1.0] * len(s[1]) for s in seen)
    assert torch.equal(logp, x[0, :, 0]) and torch.equal(dl, x * 2.0)
    del seen[:]
    logp, dl = grammar.grammar_grad_chunked(x, lens, packed, which, "canon", 1.0)
    assert len(seen) == 1 and seen[0][0] == (T, B, V) and torch.equal(dl, x * 2.0)


# ------------------------------------------------------------------------------------------------------------------------- the ABI
def test_argument_validation_without_gpu():
    from vistaocr_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "vocr_ctc_grammar_grad") and hasattr(lib, "vocr_ctc_grammar_grad_workspace_bytes")
    one = ctypes.c_void_p(16)
    ws = lib.vocr_ctc_grammar_grad_workspace_bytes
    scores = lib.vocr_ctc_grammar_workspace_bytes
    assert ws(294, 32, 96, 8, 40, 60, 0) == scores(294, 32, 96, 8, 40, 60, 0) > 294 * 32 * 96 * 4       # scores only: nothing stored
    assert ws(294, 32, 96, 8, 40, 60, 1) > ws(294, 32, 96, 8, 40, 60, 0) + 294 * 32 * 100 * 4
    assert ws(294, 32, 96, 8, 40, 60, 1) < ws(294, 32, 96, 8, 40, 60, 0) + 294 * 32 * 100 * 4 + (1 << 16)  # the mirrored tables are small
    assert ws(294, 32, 1, 8, 40, 60, 1) == 0 and ws(294, 32, 257, 8, 40, 60, 1) == 0 and ws(0, 32, 96, 8, 40, 60, 1) == 0
    assert ws(294, 0, 96, 8, 40, 60, 1) == 0 and ws(294, 32, 96, 0, 40, 60, 1) == 0 and ws(294, 32, 96, 8, 0, 60, 1) == 0
    assert ws(294, 32, 96, 8, 40, -1, 1) == 0
    assert ws(16, 2, 70, 1, 4097, 4095, 1) > 0 and ws(16, 2, 70, 1, 4097, 4096, 1) == 0 and ws(16, 2, 70, 1, 4097, 4096, 0) == 0   # 8192 cells
    # the stored lattice: t * b * (max_states + max_arcs) * 4 bytes within 2 GiB - 2000 * 32 * 8192 * 4 = 2.10e9 fits, 33 lines do not
    assert ws(2000, 32, 96, 4, 4096, 4096, 1) > 2000 * 32 * 8192 * 4 and ws(2000, 33, 96, 4, 4096, 4096, 1) == 0
    assert ws(2000, 33, 96, 4, 4096, 4096, 0) > 0                                          # ... which a scores-only call does not store
    assert ws(1 << 20, 1 << 11, 96, 1, 2, 1, 0) == 0                                       # t * b * g < 2^31

    def go(logits=one, lens=one, t=20, b=2, v=10, canon=None, s_off=one, a_off=one, g=2, src=one, cls=one, dst=one, accept=one, ms=5, ma=6,
           which=one, weights=one, logp=one, dlogits=one, wsp=one, nbytes=1 << 30):
        return lib.vocr_ctc_grammar_grad(logits, lens, t, b, v, canon, s_off, a_off, g, src, cls, dst, accept, ms, ma, which, weights, logp,
                                         dlogits, wsp, nbytes, None)

    for kw in (dict(logits=None), dict(lens=None), dict(s_off=None), dict(a_off=None), dict(accept=None), dict(which=None), dict(logp=None),
               dict(wsp=None), dict(src=None), dict(cls=None), dict(dst=None)):
        assert go(**kw) == -1 and b"vocr_ctc_grammar_grad: null pointer" in lib.vocr_last_error(), kw
    assert go(src=None, cls=None, dst=None, ma=0, nbytes=0) == -1 and b"workspace too small" in lib.vocr_last_error()   # no arcs: no arc tables
    assert go(dlogits=None) == -1 and b"vocr_ctc_grammar_grad: weights and dlogits go together" in lib.vocr_last_error()
    assert go(weights=None) == -1 and b"vocr_ctc_grammar_grad: weights and dlogits go together" in lib.vocr_last_error()
    assert go(v=257) == -1 and b"2 <= v <= 256" in lib.vocr_last_error()
    assert go(v=1) == -1 and go(t=0) == -1 and go(b=0) == -1 and go(g=0) == -1 and go(ms=0) == -1 and go(ma=-1) == -1
    assert go(ms=4097, ma=4096) == -1 and b"max_states + max_arcs <= 8192" in lib.vocr_last_error()
    assert go(t=2000, b=33, v=96, ms=4096, ma=4096) == -1 and b"vocr_ctc_grammar_grad: unsupported shape" in lib.vocr_last_error()
    need = ws(20, 2, 10, 2, 5, 6, 1)
    assert go(nbytes=need - 1) == -1 and b"vocr_ctc_grammar_grad: workspace too small" in lib.vocr_last_error()
    assert go(weights=None, dlogits=None, nbytes=ws(20, 2, 10, 2, 5, 6, 0) - 1) == -1 and b"workspace too small" in lib.vocr_last_error()
    assert go(wsp=ctypes.c_void_p(24)) == -1 and b"16-byte aligned" in lib.vocr_last_error()
