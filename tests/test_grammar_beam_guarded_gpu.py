"""GPU: vocr_ctc_grammar_beam_search called on the C entry (_lib.call) in memory the test owns to the byte (tests/guarded.py,
tests/ctc_guarded.py), as tests/test_ctc_guarded_search_gpu.py calls the other searches: every output element written over its
poison, no NaN out of a NaN-filled workspace of exactly the reported size, every guard band - logits, lengths, the automaton tables,
which, the LM tables, outputs, workspace - intact, the same bits on a second call and from ops.ctc_grammar_beam_search, and a short
workspace (16 bytes, and one byte) refused before any launch.

case     branch
K1       beam 1, nbest 1, no LM; one automaton
K16      beam 16, nbest 16, no LM; three automata through which, one index outside [0, g), a line of length 0 and one of length 1
K16_lm   the same with the LM tables
K128     beam 128, nbest 1; a line longer than T
Every case has a line of length 0.  Run with -s for the table."""
import time

import numpy as np
import pytest
import torch

from tests import beam_data as bd
from tests import ctc_guarded as cg
from tests import grammar_beam_cases as gc
from vistaocr_amd.grammar import Grammar, pack_dense_grammars

pytestmark = pytest.mark.gpu
NEG = -np.inf
I32, F32 = torch.int32, torch.float32
V = 13


@pytest.fixture(scope="module", autouse=True)
def _table():
    cg.T0[0] = time.time()
    yield
    cg.print_table("ctc-guarded: the grammar-constrained beam search")


def _i32(a):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.int32)))


def _grammars():
    al = gc.field_alphabet()
    return [gc.field_grammar(), Grammar.from_regex(al, r"a\d+"), Grammar.from_regex(al, r"-?\d{3}")]


# name: (seed, T, K, nbest, lens, which (None: one automaton), with LM)
CASES = {
    "K1": (31, 12, 1, 1, [12, 0, 17, 6], None, False),
    "K16": (32, 12, 16, 16, [12, 1, 0, 19, 12, 12], [0, 1, 2, 1, 5, 2], False),
    "K16_lm": (33, 12, 16, 16, [1, 12, 0, 14, 12, 12], [1, 0, 0, 2, -1, 1], True),
    "K128": (34, 8, 128, 1, [8, 0, 9, 5], None, False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_ctc_grammar_beam_search(name):
    from vistaocr_amd import _lib, ops
    seed, T, K, nbest, lens, which, with_lm = CASES[name]
    B = len(lens)
    grammars = _grammars() if which is not None else _grammars()[:1]
    which_l = [0] * B if which is None else which
    x = bd.dense_logits(np.random.default_rng(seed), T, B, V)
    lm = gc.field_lm() if with_lm else None
    alpha, beta = (0.8, 0.6) if with_lm else (0.0, 0.0)
    case = gc.Case("guarded", x, lens, K, nbest, grammars, which_l, None, lm, alpha, beta)
    ref = gc.references(case)
    lib = _lib.load()
    nbytes = lib.vocr_ctc_grammar_beam_workspace_bytes(T, B, V, K, nbest)
    assert nbytes == T * B * K * 8 > lib.vocr_ctc_grammar_beam_workspace_bytes(T - 1, B, V, K, nbest) > 0    # T * beam nodes per line
    packed = pack_dense_grammars(grammars, "cpu")
    G = len(grammars)
    tabs = lm.to("cpu") if with_lm else None
    S = int(tabs["lm_logp"].shape[0]) if with_lm else 0
    ins = dict(x=torch.from_numpy(x), lens_in=(_i32(lens), 0), state_off=(packed["state_off"], 1 << 30), next=(packed["next"], 1 << 30),
               dist=(packed["dist"], 0), which=(_i32(which_l), 0), lm_logp=tabs["lm_logp"] if with_lm else None,
               lm_next=(tabs["lm_next"], 1 << 30) if with_lm else None, lm_eos=tabs["lm_eos"] if with_lm else None)
    outs = dict(labels=((B, nbest, T), I32), lens=((B, nbest), I32), scores=((B, nbest, 3), F32))

    def args(p, ws, nb, short=0):
        return (p["x"], p["lens_in"], T, B, V, None, K, nbest, p["state_off"], p["next"], p["dist"], G, p["which"], p["lm_logp"],
                p["lm_next"], p["lm_eos"], S, int(tabs["start"]) if with_lm else 0, alpha, beta, float("-inf"), p["labels"], p["lens"],
                p["scores"], ws, nb - short, ops._stream())

    run = cg.guarded_runs("vocr_ctc_grammar_beam_search", name, ins, outs, nbytes, args)
    # one byte short, the workspace itself whole: refused before any launch
    cg.Call("vocr_ctc_grammar_beam_search", ins, outs, nbytes, lambda p, ws, nb: args(p, ws, nb, short=1),
            refuse=True).assert_nothing_launched(name)
    lab, ln, sc = run.host("labels"), run.host("lens"), run.host("scores")
    err = gc.compare("guarded " + name, case, ref, lab, ln, sc, floor=(B + 1) // 2)
    for b in range(B):
        Lb = min(max(lens[b], 0), T)
        for q in range(nbest):
            assert 0 <= ln[b, q] <= Lb and not lab[b, q, ln[b, q]:].any() and (lab[b, q, :ln[b, q]] > 0).all(), (name, b, q)
        assert np.isfinite(sc[b, 0, 0]) == bool(ref[b].hyps), (name, b)
        if not 0 <= which_l[b] < G or Lb == 0:
            assert not np.isfinite(sc[b, :, 0]).any(), (name, b)                # no automaton; no frames and a start that does not accept
    bar = np.asarray(gc.bars("guarded"))
    cg.row("vocr_ctc_grammar_beam_search", name, "beam %d, nbest %d, %d automata, %s" % (K, nbest, G, "LM tables" if with_lm else "no LM"),
           float((err[bar > 0] / bar[bar > 0]).max()), nbytes)
    dev = {k: (v.to("cuda") if torch.is_tensor(v) else v) for k, v in packed.items()}
    wr = ops.ctc_grammar_beam_search(torch.from_numpy(x).cuda(), lens, dev, which_l, None, K, nbest, lm.to("cuda") if with_lm else None,
                                     alpha, beta)
    assert all(cg.same_bits(g, run.out(o)) for g, o in zip(wr, ("labels", "lens", "scores"))), name
