"""GPU: the CTC entry points that SEARCH, and the scorer of their results, each called on the C entry (_lib.call) in memory the test owns
to the byte (tests/guarded.py, tests/ctc_guarded.py): vocr_ctc_beam_search, vocr_ctc_word_beam_search, vocr_ctc_grammar_scores,
vocr_ctc_grammar_grad, vocr_edit_stats.  The other six entries and what every case holds of a call (accuracy at the entry's own suite's
bar, every output element written, no NaN out of the NaN-filled workspace and bands, every band intact, the same bits on a second call
and from the ops.* wrapper, the refusal of a workspace 16 bytes short): tests/test_ctc_guarded_gpu.py.  Here the elements no path
reaches are out_labels zero past a hypothesis's length, length 0 and total -inf of a rank the search did not fill, -1 lengths where no
labelling is accepted, gradient rows past lens and of lines without a match zero, -1 statistics that were not asked for or belong to an
invalid pair, operation codes 0 past a trace's end.

entry                       branch of the host plan                                         case that takes it
vocr_ctc_beam_search,       beam 1 / 16 / 128                                               K1 (word: wK1) / K16, K16_lm (wK16) / K128 (wK128)
vocr_ctc_word_beam_search   nbest 1 / nbest = beam                                          K1, K128 / K16, K16_lm, wK16
                            with / without the LM tables (character search)                 K16_lm / the others
                            a line so short that fewer than nbest prefixes exist            lens 1 in K16, K16_lm, wK16: at most V prefixes
                            lens 0 / lens greater than T                                    every case has both
                            V = 2 / V = 256                                                 V2_K16 / V256_K16, wV256_K16 (the word search
                                                                                            needs a lexicon: no V = 2)
                            asserted: the workspace grows with T * beam nodes per line (the header's node pool)
vocr_ctc_grammar_scores     want_best 0 / 1                                                 every case runs both; asserted: the sizes differ
                                                                                            by the back pointers, align16(T B G N 4)
                            one automaton / several                                         one / several, unstaged
                            tables staged in LDS / too large for that: the call's           one, several / unstaged (a prefix-closed chain of
                            lds = (4 N + 512) 4 plus staged = align16(16 arcs + 8 states    3000 labels: N = 6001, 98064 + 72208 B > 150528 B;
                            + 4 (arcs / 64 + 2)) against 147 KiB                            several: N = 9, a few hundred bytes)
                            an invalid automaton between valid ones                         several (arcs out of order)
                            V = 2 / V = 256                                                 V2 / V256
vocr_ctc_grammar_grad       want_grad 0 / 1                                                 every case runs both; asserted: the scores-only
                                                                                            size is the class log-probabilities + one plan
                            which[b] pointing several lines at one automaton                which (lines 0 and 1), V2
                            a line without a match / an invalid automaton / which outside   which (lines 2 / 3 / 4)
vocr_edit_stats             want = characters, words, both, characters + trace, all three   seams runs 1, 2, 3, 5, 7
                            a table that fits BP_LDS (8192 words) / needs the slab          seams: 5 * 128 = 640 words, workspace 16 B / slab:
                                                                                            ceil(260 / 16) * pad64(520) = 17 * 576 = 9792 words
                            lengths 63 / 64 / 65 on either side, an empty side              seams
                            confusion NULL / given                                          slab (want 5) / seams (want 7), slab (want 7)
                            more pairs than workgroups (256 with a trace): a slab reused    slab: 258 pairs, pairs 0 and 256 (one workgroup's
                                                                                            first and second) both need it, 1 and 257 too
                            asserted: workspace = 16 + min(np, 256) * slab words * 4
                            V = 8 throughout: the reference works on an Alphabet, and V does not enter the host plan
Run with -s for the table (profiles/ctc_guarded_errors.txt keeps it)."""
import os
import tempfile
import time

import numpy as np
import pytest
import torch

from tests import align_ref as ar
from tests import beam_data as bd
from tests import ctc_guarded as cg
from tests import grammar_grad_ref as gg
from tests import grammar_ref as gr
from tests import guarded as gd

pytestmark = pytest.mark.gpu
NEG = -np.inf
I32, F32, U8 = torch.int32, torch.float32, torch.uint8


@pytest.fixture(scope="module", autouse=True)
def _table():
    cg.T0[0] = time.time()
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)
    cg.print_table("ctc-guarded: searches and edit statistics")


def _i32(a):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.int32)))


def _align16(n):
    return (n + 15) // 16 * 16


def _dev(t):
    return None if t is None else t.to("cuda")


# ------------------------------------------------------------------------------------------- vocr_ctc_beam_search / _word_beam_search
V_CHAR = 12
_lms = {}


def _char_lm3():
    """a character 3-gram over blank + 11 letters (tests/beam_data.py's writer)"""
    import vistaocr_amd as va
    from tests.beam_cases import _letters_alphabet
    if "char" not in _lms:
        al = _letters_alphabet(V_CHAR)
        with tempfile.TemporaryDirectory() as d:
            path = bd.write_char_arpa(os.path.join(d, "char3.arpa"), [al.idx_to_char[c] for c in range(1, V_CHAR)], order=3, seed=3)
            _lms["char"] = va.CharNgramLM.from_arpa(path, al)
    return _lms["char"]


# name: (group of tests/beam_cases.py's bars, seed, T, V, K, nbest, lens, with LM)
BEAM_CASES = {
    "K1": ("dense", 11, 12, V_CHAR, 1, 1, [12, 0, 17, 5], False),
    "K16": ("dense", 12, 12, V_CHAR, 16, 16, [12, 1, 0, 19], False),
    "K16_lm": ("dense_lm", 13, 12, V_CHAR, 16, 16, [1, 12, 0, 14], True),
    "K128": ("dense", 14, 8, V_CHAR, 128, 1, [8, 0, 9, 3], False),
    "V2_K16": ("dense", 16, 12, 2, 16, 16, [12, 1, 0, 13], False),
    "V256_K16": ("big", 15, 6, 256, 16, 4, [6, 0, 7], False),
}
# name: (group, seed, T, the tiny word LM of tests/beam_cases.py ("de": V = 9, "v256": V = 256), K, nbest, lens)
WORD_CASES = {
    "wK1": ("word_oov", 23, 12, "de", 1, 1, [12, 0, 13, 4]),
    "wK16": ("word_oov", 21, 12, "de", 16, 16, [12, 1, 0, 15]),
    "wK128": ("word_oov", 22, 8, "de", 128, 1, [8, 0, 11, 2]),
    "wV256_K16": ("word_big", 24, 6, "v256", 16, 4, [6, 0, 8]),
}


def _search_checks(name, case, ref, run, T, nbest):
    """tests/beam_cases.py's comparison on the decided lines, and on EVERY line what the header says of each element"""
    from tests import beam_cases as bc
    lab, ln, sc = run.host("labels"), run.host("lens"), run.host("scores")
    _, err = bc.compare("guarded " + name, case, ref, lab, ln, sc)
    for b in range(lab.shape[0]):
        filled = np.isfinite(sc[b, :, 0])
        assert not filled[1:][~filled[:-1]].any(), (name, b)                    # best first: no filled rank behind an unfilled one
        assert (sc[b, ~filled, 0] == NEG).all() and (ln[b, ~filled] == 0).all(), (name, b)
        assert filled[0], (name, b)                                             # the empty labelling at least
        for q in range(nbest):
            assert 0 <= ln[b, q] <= min(max(case.lens[b], 0), T) and not lab[b, q, ln[b, q]:].any(), (name, b, q)
            assert (lab[b, q, :ln[b, q]] > 0).all(), (name, b, q)
        if case.lens[b] <= 0:
            assert filled.sum() == 1 and ln[b, 0] == 0 and sc[b, 0, 1] == 0.0, (name, b)
        if case.lens[b] == 1:
            assert filled.sum() <= case.x.shape[2], (name, b)    # one frame: the empty prefix and one per symbol
    bar = np.asarray(bc.bars(case.group))
    return float((err[bar > 0] / bar[bar > 0]).max())                           # a bar of 0 (no LM: the LM score is 0) was held exactly


@pytest.mark.parametrize("name", sorted(BEAM_CASES))
def test_ctc_beam_search(name):
    from tests import beam_cases as bc
    from tests import beam_ref as br
    from vistaocr_amd import _lib, ops
    group, seed, T, V, K, nbest, lens, with_lm = BEAM_CASES[name]
    B = len(lens)
    x = bd.dense_logits(np.random.default_rng(seed), T, B, V)
    lm = _char_lm3() if with_lm else None
    alpha, beta = (0.8, 1.0) if with_lm else (0.0, 0.0)
    case = bc._case(group, x, K, nbest, lens=lens, lm=lm, alpha=alpha, beta=beta, dense=False)
    ref = []
    for b in range(B):
        hyps, gap = br.beam_search(x[:, b], lens[b], K, nbest=nbest, lm=lm, alpha=alpha, beta=beta)
        ref.append(bc.Ref(hyps, gap, {}))
    lib = _lib.load()
    nbytes = lib.vocr_ctc_beam_workspace_bytes(T, B, V, K, nbest)
    assert nbytes > lib.vocr_ctc_beam_workspace_bytes(T - 1, B, V, K, nbest) > 0     # the node pool: T * beam nodes per line
    tabs = lm.to("cpu") if with_lm else None
    S = int(tabs["lm_logp"].shape[0]) if with_lm else 0
    ins = dict(x=torch.from_numpy(x), lens=(_i32(lens), 0), lm_logp=tabs["lm_logp"] if with_lm else None,
               lm_next=(tabs["lm_next"], 0) if with_lm else None, lm_eos=tabs["lm_eos"] if with_lm else None)
    outs = dict(labels=((B, nbest, T), I32), lens=((B, nbest), I32), scores=((B, nbest, 3), F32))
    ins["lens_in"] = ins.pop("lens")
    args = lambda p, ws, nb: (p["x"], p["lens_in"], T, B, V, None, K, nbest, p["lm_logp"], p["lm_next"], p["lm_eos"], S,
                              int(tabs["start"]) if with_lm else 0, alpha, beta, float("-inf"), p["labels"], p["lens"], p["scores"], ws, nb,
                              ops._stream())
    run = cg.guarded_runs("vocr_ctc_beam_search", name, ins, outs, nbytes, args)
    frac = _search_checks(name, case, ref, run, T, nbest)
    cg.row("vocr_ctc_beam_search", name, "beam %d, nbest %d, %s" % (K, nbest, "LM tables" if with_lm else "no LM"), frac, nbytes)
    wr = ops.ctc_beam_search(_dev(torch.from_numpy(x)), lens, None, K, nbest, lm.to("cuda") if with_lm else None, alpha, beta)
    assert all(cg.same_bits(g, run.out(o)) for g, o in zip(wr, ("labels", "lens", "scores"))), name


@pytest.mark.parametrize("name", sorted(WORD_CASES))
def test_ctc_word_beam_search(name):
    from tests import beam_cases as bc
    from tests import word_beam_ref as wbr
    from vistaocr_amd import _lib, ops
    from vistaocr_amd.ops import _WORD_LM_FLOAT, _WORD_LM_INT
    group, seed, T, kind, K, nbest, lens = WORD_CASES[name]
    B = len(lens)
    lm = bc.tiny_word_lm(kind)
    V = lm.to("cpu")["kind"].numel()
    alpha, beta, oov = 0.8, 1.0, -2.5
    x = bd.dense_logits(np.random.default_rng(seed), T, B, V)
    case = bc._case(group, x, K, nbest, lens=lens, lm=lm, alpha=alpha, beta=beta, oov=oov, dense=False)
    ref = []
    for b in range(B):
        hyps, gap = wbr.beam_search(x[:, b], lens[b], K, lm, nbest=nbest, alpha=alpha, beta=beta, oov=oov)
        ref.append(bc.Ref(hyps, gap, {}))
    lib = _lib.load()
    nbytes = lib.vocr_ctc_word_beam_workspace_bytes(T, B, V, K, nbest)
    assert nbytes > lib.vocr_ctc_word_beam_workspace_bytes(T - 1, B, V, K, nbest) > 0
    tabs = lm.to("cpu")
    ins = dict(x=torch.from_numpy(x), lens_in=(_i32(lens), 0))
    for k in _WORD_LM_INT:
        ins[k] = (tabs[k].contiguous(), 0)
    for k in _WORD_LM_FLOAT:
        ins[k] = tabs[k].contiguous()
    Nn, S, E, W = tabs["trie_tok"].numel(), tabs["bow"].numel(), tabs["succ_tok"].numel(), int(tabs["num_tokens"])
    outs = dict(labels=((B, nbest, T), I32), lens=((B, nbest), I32), scores=((B, nbest, 3), F32))
    args = lambda p, ws, nb: (p["x"], p["lens_in"], T, B, V, None, K, nbest, p["kind"], p["tok"], p["trie_next"], p["trie_tok"],
                              p["trie_la"], Nn, p["off"], p["succ_tok"], p["succ_logp"], p["succ_next"], p["bow"], p["back"], S, E, W,
                              int(tabs["start"]), int(tabs["unk"]), int(tabs["eos"]), alpha, beta, oov, p["labels"], p["lens"],
                              p["scores"], ws, nb, ops._stream())
    run = cg.guarded_runs("vocr_ctc_word_beam_search", name, ins, outs, nbytes, args)
    frac = _search_checks(name, case, ref, run, T, nbest)
    cg.row("vocr_ctc_word_beam_search", name, "beam %d, nbest %d" % (K, nbest), frac, nbytes)
    wr = ops.ctc_word_beam_search(_dev(torch.from_numpy(x)), lens, None, lm.to("cuda"), K, nbest, alpha, beta, oov)
    assert all(cg.same_bits(g, run.out(o)) for g, o in zip(wr, ("labels", "lens", "scores"))), name


# ------------------------------------------------------------------------------------------ vocr_ctc_grammar_scores / _grammar_grad
def _chain(labels, accept_all=False):
    L = len(labels)
    return gr.make(L + 1, [(i, c, i + 1) for i, c in enumerate(labels)], range(L + 1) if accept_all else [L])


def _unsorted(a):
    return dict(a, src=a["src"][::-1].copy(), cls=a["cls"][::-1].copy(), dst=a["dst"][::-1].copy())


def _grammar_case(name):
    """(x numpy [T,B,V], lens, automata)"""
    rng = np.random.default_rng([61, sorted(GRAMMAR_NAMES).index(name)])
    if name == "one":
        return bd.dense_logits(rng, 9, 2, 6, 2.0), [9, 0], [_chain([1, 2])]
    if name == "several":
        star = gr.make(2, [(0, 1, 1), (1, 2, 0)], [0], V=6)                      # (ab)*: the start accepts
        autos = [star, _unsorted(_chain([4, 5, 2])), _chain([3, 3, 5]), gr.make(1, [(0, c, 0) for c in range(1, 6)], [0], V=6)]
        return bd.dense_logits(rng, 9, 3, 6, 2.0), [9, 5, 0], autos
    if name == "unstaged":
        return bd.dense_logits(rng, 6, 1, 4, 2.0), [6], [_chain([1 + i % 3 for i in range(3000)], accept_all=True), _chain([2])]
    if name == "V2":
        return bd.dense_logits(rng, 7, 2, 2, 2.0), [7, 2], [_chain([1]), _chain([1, 1])]
    x = bd.dense_logits(rng, 6, 2, 256, 2.0)
    return x, [6, 9], [_chain([255, 1]), gr.make(1, [(0, c, 0) for c in (7, 200, 255)], [0], V=256)]


GRAMMAR_NAMES = ["one", "several", "unstaged", "V2", "V256"]


def _packed(automata):
    cat = lambda k: _i32(np.concatenate([np.asarray(a[k], dtype=np.int32) for a in automata]))
    return dict(state_off=_i32(np.cumsum([0] + [a["S"] for a in automata])), arc_off=_i32(np.cumsum([0] + [len(a["src"]) for a in automata])),
                src=cat("src"), cls=cat("cls"), dst=cat("dst"), accept=cat("accept")), \
        max(a["S"] for a in automata), max(len(a["src"]) for a in automata)


def _gp_dev(tabs, ms, ma):
    gp = {k: _dev(v) for k, v in tabs.items()}
    gp["max_states"], gp["max_arcs"] = ms, ma
    return gp


@pytest.mark.parametrize("name", GRAMMAR_NAMES)
def test_ctc_grammar_scores(name):
    from tests.test_grammar_gpu import bound
    from vistaocr_amd import _lib, ops
    x, lens, autos = _grammar_case(name)
    T, B, V = x.shape
    G = len(autos)
    tabs, ms, ma = _packed(autos)
    N = ms + ma
    lib = _lib.load()
    nbytes, small = lib.vocr_ctc_grammar_workspace_bytes(T, B, V, G, ms, ma, 1), lib.vocr_ctc_grammar_workspace_bytes(T, B, V, G, ms, ma, 0)
    assert small > 0 and nbytes - small == _align16(T * B * G * N * 4)          # the back pointers when want_best
    staged = (4 * N + 512) * 4 + _align16(16 * ma + 8 * ms + 4 * (ma // 64 + 2)) <= 147 * 1024
    assert staged == (name != "unstaged")
    ins = dict(x=torch.from_numpy(x), lens_in=(_i32(lens), 0))
    ins.update({k: (v, 0) for k, v in tabs.items()})
    args = lambda p, ws, nb: (p["x"], p["lens_in"], T, B, V, None, p["state_off"], p["arc_off"], G, p["src"], p["cls"], p["dst"], p["accept"],
                              ms, ma, p["logp"], p["best"], p["labels"], p["lens"], T + 2, ws, nb, ops._stream())
    outs = dict(logp=((B, G), F32), best=((B, G), F32), labels=((B, G, T + 2), I32), lens=((B, G), I32))
    run = cg.guarded_runs("vocr_ctc_grammar_scores", name, ins, outs, nbytes, args)
    only = cg.guarded_runs("vocr_ctc_grammar_scores", name, ins, dict(outs, best=None, labels=None, lens=None), small, args)
    assert cg.same_bits(only.out("logp"), run.out("logp")), name                # the same bits with and without best paths
    # tests/test_grammar_gpu.py's _check, on the guarded outputs
    ref = gr.search(x, lens, autos, None, ms, ma)
    cls = ar.classes_of(V, None)
    logp, best, labels, ln = (run.host(o) for o in ("logp", "best", "labels", "lens"))
    D = np.array([gr.max_in_degree(a) for a in autos])[None, :]
    Tb = np.clip(np.asarray(lens), 0, T)[:, None]
    Ns = np.array([a["S"] + len(a["src"]) for a in autos])[None, :]
    frac = 0.0
    for g, r in ((logp, ref["logp"]), (best, ref["best"])):
        assert not np.isnan(g).any() and not np.any(g == np.inf), name
        assert np.array_equal(g == NEG, r == NEG), (name, g, r)
        fin = r != NEG
        if fin.any():
            d = np.abs(g.astype(np.float64) - np.where(fin, r, 0.0))[fin]
            frac = max(frac, float((d / np.broadcast_to(bound(Tb, np.where(fin, r, 0.0), D, Ns), r.shape)[fin]).max()))
    dead = ref["best"] == NEG
    assert np.all(ln[dead] == -1) and np.all(ln[~dead] >= 0), name
    assert not labels[dead].any(), name                                         # nothing accepted: a row of zeros
    for b, g in np.argwhere(~dead):
        assert gr.accepts(autos[g], labels[b, g, :ln[b, g]], cls) and not labels[b, g, ln[b, g]:].any(), (name, int(b), int(g))
    vit = ops.ctc_align(_dev(torch.from_numpy(x)), lens, run.out("labels").clone(), run.out("lens").clone())[0][..., 0].cpu().numpy()
    if (~dead).any():
        d = np.abs(vit.astype(np.float64)[~dead] - best.astype(np.float64)[~dead])
        frac = max(frac, float((d / np.broadcast_to(bound(Tb, np.where(dead, 0.0, ref["best"]), D, Ns), dead.shape)[~dead]).max()))
    cg.row("vocr_ctc_grammar_scores", name, "G %d, N %d, %s, want_best 1 (0: %d B)" % (G, N, "staged" if staged else "not staged", small),
           frac, nbytes)
    assert frac <= 1.0, (name, frac)
    wr = ops.ctc_grammar_scores(_dev(torch.from_numpy(x)), lens, _gp_dev(tabs, ms, ma), None, True)
    assert cg.same_bits(wr[0], run.out("logp")) and cg.same_bits(wr[1], run.out("best")) and cg.same_bits(wr[3], run.out("lens")), name
    assert cg.same_bits(wr[2], run.out("labels")[:, :, :T].contiguous()) and not run.host("labels")[:, :, T:].any(), name
    w0 = ops.ctc_grammar_scores(_dev(torch.from_numpy(x)), lens, _gp_dev(tabs, ms, ma), None, False)
    assert cg.same_bits(w0[0], run.out("logp")) and w0[1] is None and w0[2] is None and w0[3] is None, name


# name: (the grammar-gradient suite's family, x, lens, automata, which)
def _grad_case(name):
    rng = np.random.default_rng([67, len(name)])
    if name == "which":
        T, V = 12, 6
        autos = [_chain([1, 2]), _unsorted(_chain([4, 5, 2])), gr.make(2, [(0, 1, 1), (1, 2, 0)], [0], V=V), _chain([3, 3, 5])]
        lens = [12, 9, 2, 12, 12]
        return "which", bd.dense_logits(rng, T, 5, V, 2.0), lens, autos, [0, 0, 3, 1, 4]    # line 2: 3 3 5 needs 4 frames
    if name == "V2":
        return "lens", bd.dense_logits(rng, 9, 3, 2, 2.0), [9, 0, 4], [_chain([1]), _chain([1, 1])], [1, 0, 1]
    autos = [_chain([255, 1]), gr.make(1, [(0, c, 0) for c in (7, 200, 255)], [0], V=256)]
    return "which", bd.dense_logits(rng, 6, 2, 256, 2.0), [6, 5], autos, [1, 0]


@pytest.mark.parametrize("name", ["which", "V2", "V256"])
def test_ctc_grammar_grad(name):
    from tests.test_grammar_grad_gpu import TOL, _errors, _weights
    from vistaocr_amd import _lib, ops
    family, x, lens, autos, which = _grad_case(name)
    T, B, V = x.shape
    G = len(autos)
    tabs, ms, ma = _packed(autos)
    w = _weights(np.random.default_rng([17, B]), B)
    lib = _lib.load()
    nbytes = lib.vocr_ctc_grammar_grad_workspace_bytes(T, B, V, G, ms, ma, 1)
    small = lib.vocr_ctc_grammar_grad_workspace_bytes(T, B, V, G, ms, ma, 0)
    plan = _align16(G * 4) + _align16(G * ms * 8) + _align16(G * ma * 16) + _align16(G * (ma // 64 + 2) * 4)
    assert small == _align16(T * B * V * 4) + plan and nbytes >= small + plan + _align16(T * B * (ms + ma) * 4)
    ins = dict(x=torch.from_numpy(x), lens_in=(_i32(lens), 0), which=(_i32(which), 0))
    ins.update({k: (v, 0) for k, v in tabs.items()})
    args = lambda p, ws, nb: (p["x"], p["lens_in"], T, B, V, None, p["state_off"], p["arc_off"], G, p["src"], p["cls"], p["dst"], p["accept"],
                              ms, ma, p["which"], p.get("w"), p["logp"], p["dl"], ws, nb, ops._stream())
    outs = dict(logp=((B,), F32), dl=((T, B, V), F32))
    run = cg.guarded_runs("vocr_ctc_grammar_grad", name, dict(ins, w=torch.from_numpy(w)), outs, nbytes, args)
    only = cg.guarded_runs("vocr_ctc_grammar_grad", name, ins, dict(outs, dl=None), small, args)
    assert cg.same_bits(only.out("logp"), run.out("logp")), name
    ref = gg.run(x, lens, autos, which, None, w.astype(np.float64), ms, ma)
    serr, gerr = _errors(name, _dev(torch.from_numpy(x)), lens, run.out("logp"), run.out("dl"), ref, w)
    tol_s, tol_g = TOL[family]
    cg.row("vocr_ctc_grammar_grad", name, "want_grad 1 (0: %d B), family %s" % (small, family), max(serr / tol_s, gerr / tol_g), nbytes)
    assert serr <= tol_s and gerr <= tol_g, (name, family, serr, gerr)
    if name == "which":
        fin = np.isfinite(run.host("logp"))
        assert fin.tolist() == [True, True, False, False, False] and not run.host("dl")[:, 2:].any(), name
    gp = _gp_dev(tabs, ms, ma)
    l3, g3 = ops.ctc_grammar_grad(_dev(torch.from_numpy(x)), lens, gp, _dev(_i32(which)), None, _dev(torch.from_numpy(w)))
    assert cg.same_bits(l3, run.out("logp")) and cg.same_bits(g3, run.out("dl")), name
    l4, g4 = ops.ctc_grammar_grad(_dev(torch.from_numpy(x)), lens, gp, _dev(_i32(which)))
    assert g4 is None and cg.same_bits(l4, run.out("logp")), name
    sc = ops.ctc_grammar_scores(_dev(torch.from_numpy(x)), lens, gp, None, False)[0].cpu().numpy()
    for b, k in enumerate(which):                                               # the bits of the scorer's [b][which[b]]
        if 0 <= k < G:
            assert run.host("logp")[b].tobytes() == sc[b, k].tobytes(), (name, b)


# ---------------------------------------------------------------------------------------------------------------- vocr_edit_stats
def _stats_case(name):
    """(hyps, refs, pairs): label lists over tests/test_score_gpu.py's 8-symbol alphabet, and (a, b) index pairs"""
    from tests.test_score_gpu import AL8, _mutated, _seq
    rng = np.random.default_rng([71, len(name)])
    if name == "seams":
        refs = [_seq(rng, AL8, n) for n in (63, 64, 65, 5, 0)]
        hyps = [_mutated(rng, AL8, refs[i], n) for i, n in enumerate((65, 64, 63, 0, 4))] + [[2, 0, 3], []]
        pairs = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 1), (6, 4), (0, 2), (2, 0), (1, 7), (1, 1)]   # (5, 1): a label 0; (1, 7): no such row
        return hyps, refs, pairs
    big_r = [_seq(rng, AL8, 520), _seq(rng, AL8, 517)]
    big_h = [_mutated(rng, AL8, big_r[0], 260), _mutated(rng, AL8, big_r[1], 257)]
    refs = big_r + [_seq(rng, AL8, n) for n in (3, 7, 0, 12)]
    hyps = big_h + [_mutated(rng, AL8, refs[2 + i], n) for i, n in enumerate((4, 7, 2, 0))]
    pairs = [(0, 0), (1, 1)] + [(2 + i % 4, 2 + i % 4) for i in range(254)] + [(1, 1), (0, 1)]
    return hyps, refs, pairs


@pytest.mark.parametrize("name,want", [("seams", 1), ("seams", 2), ("seams", 3), ("seams", 5), ("seams", 7), ("slab", 5), ("slab", 7)])
def test_edit_stats(name, want):
    from tests.test_score_gpu import AL8, _expect
    from vistaocr_amd import _lib, ops
    from vistaocr_amd.lm import class_kinds
    hyps, refs, pairs = _stats_case(name)
    V, npairs = len(AL8), len(pairs)
    max_a, max_b = max(len(h) for h in hyps), max(len(r) for r in refs)
    a, alens = gd.pack_rows(hyps, max_a + 3, V)
    b, blens = gd.pack_rows(refs, max_b + 3, V)
    na, nb = len(hyps), len(refs)
    trace, with_conf = bool(want & 4), bool(want & 4) and not (name == "slab" and want == 5)
    ops_stride = (max_a + max_b + 3) // 4 * 4                                   # whole 32-bit words for the guard bands
    table = (max_a + 15) // 16 * ((max_b + 63) // 64 * 64)
    slab = table if trace and table > 8192 else 0
    nbytes = _lib.load().vocr_edit_stats_workspace_bytes(na, nb, npairs, V, max_a, max_b, want)
    assert nbytes == 16 + min(npairs, 256) * slab * 4 and (slab > 0) == (name == "slab")
    assert name != "slab" or (npairs > 256 and len(hyps[pairs[256][0]]) > 256)  # a workgroup's second pair needs its slab again
    canon, kinds = _i32(AL8.canonical_indices()), torch.from_numpy(class_kinds(AL8))
    ins = dict(a=(a, V), alens=(alens, 0), b=(b, V), blens=(blens, 0), pairs=(_i32(pairs).reshape(-1, 2), 0), canon=(canon, 0),
               kinds=(kinds, 0), conf=(torch.zeros(V, V, dtype=I32), 0) if with_conf else None)
    outs = dict(stats=((npairs, 12), I32), ops=((npairs, ops_stride), U8) if trace else None)
    args = lambda p, ws, nbts: (p["a"], p["alens"], na, max_a + 3, max_a, p["b"], p["blens"], nb, max_b + 3, max_b, p["pairs"], npairs,
                                p["canon"], p["kinds"], V, want, p["stats"], p["conf"], p["ops"], ops_stride, ws, nbts, ops._stream())
    run = cg.guarded_runs("vocr_edit_stats", "%s_want%d" % (name, want), ins, outs, nbytes, args, inout=("conf",))
    st = run.host("stats")
    tr = run.host("ops")
    want_conf = np.zeros((V, V), dtype=np.int64)
    cache = {}
    for p, (i, j) in enumerate(pairs):
        bad = i >= na or j >= nb or any(not 0 < v < V for v in hyps[i]) or any(not 0 < v < V for v in refs[j])
        if bad:
            assert (st[p] == -1).all() and (tr is None or not tr[p].any()), (name, want, p)
            continue
        if (i, j) not in cache:
            cache[(i, j)] = _expect(AL8, hyps[i], refs[j])
        es, eo, ec = cache[(i, j)]
        chars = [es[0]] + (es[1:4] if trace else [-1] * 3) + es[4:6] if want & 1 else [-1] * 6
        words = [es[6]] + (es[7:10] if trace else [-1] * 3) + es[10:12] if want & 2 else [-1] * 6
        assert st[p].tolist() == chars + words, (name, want, p, st[p].tolist(), chars + words)
        if trace:
            assert tr[p, :len(eo)].tolist() == eo.tolist() and not tr[p, len(eo):].any(), (name, want, p)
            want_conf += ec
    if with_conf:
        assert np.array_equal(run.ins["conf"].t.cpu().numpy(), want_conf), (name, want)
    cg.row("vocr_edit_stats", "%s_want%d" % (name, want), "%d pairs, table %d words: %s, confusion %s"
           % (npairs, table, "slab" if slab else "LDS" if trace else "no trace", "given" if with_conf else "NULL"), 0.0, nbytes)
    conf = torch.zeros(V, V, dtype=I32, device="cuda") if with_conf else None
    wr = ops.edit_stats(_dev(a[:, :max_a].contiguous()), _dev(alens), _dev(b[:, :max_b].contiguous()), _dev(blens),
                        _dev(_i32(pairs).reshape(-1, 2)), V, _dev(canon), _dev(kinds), want, confusion=conf, ops=trace)
    if trace:
        assert cg.same_bits(wr[0], run.out("stats")) and cg.same_bits(wr[1], run.out("ops")[:, :max_a + max_b].contiguous()), (name, want)
        assert not run.host("ops")[:, max_a + max_b:].any()
    else:
        assert cg.same_bits(wr, run.out("stats")), (name, want)
    if with_conf:
        assert cg.same_bits(conf, run.ins["conf"].t), (name, want)
