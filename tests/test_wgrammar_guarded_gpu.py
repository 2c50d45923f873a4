"""GPU: the three weighted grammar entries called on the C entry (_lib.call) in memory the test owns to the byte (tests/guarded.py,
tests/ctc_guarded.py): every output element written over its poison, no NaN out of a NaN-filled workspace of exactly the reported
size, every guard band - logits, lengths, the automaton tables, the WEIGHT tables in buffers of exactly E, S and states x V floats,
which, outputs, workspace - intact, the same bits on a second call, a workspace 16 bytes short and one byte short refused before any
launch.  Run with -s for the table.

entry                                   case      branch
vocr_ctc_grammar_scores_weighted        small     three automata, 256 threads, plan and weights staged; lines of length 0 and 1
                                        big       a tree of 8192 cells, 1024 threads, nothing staged
vocr_ctc_grammar_grad_weighted          small     the same with which (one index outside [0, g)) and per-line weights
                                        big       the tree
vocr_ctc_grammar_beam_search_weighted   K16       beam 16, nbest 16, three automata through which, one index outside, the trigram
                                        K128      beam 128, nbest 1, no LM
The beam cases and their references are tests/wgrammar_cases.py's (GUARDED_BEAM); tests/test_wgrammar_cpu.py holds them to at most one
undecided line in eight."""
import time

import numpy as np
import pytest
import torch

from tests import beam_data as bd
from tests import ctc_guarded as cg
from tests import grammar_beam_cases as gc
from tests import grammar_ref as gr
from tests import wgrammar_cases as wc
from tests import wgrammar_ref as wr
from vistaocr_amd.grammar import pack_dense_grammars

pytestmark = pytest.mark.gpu
NEG = -np.inf
I32, F32 = torch.int32, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _table():
    cg.T0[0] = time.time()
    yield
    cg.print_table("ctc-guarded: the weighted grammar entries")


def _i32(a):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.int32)))


def _f32(a):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))


def _sweep(name):
    c = wc.sweep_case("slack" if name == "small" else "cells8192")
    lens = [12, 0, 1, 9] if name == "small" else list(c.lens)
    ms = c.max_states or max(a["S"] for a in c.automata)
    ma = c.max_arcs or max(len(a["src"]) for a in c.automata)
    cat = lambda k: np.concatenate([np.asarray(a[k]) for a in c.automata])
    ins = dict(x=torch.from_numpy(np.ascontiguousarray(c.x, dtype=np.float32)), lens_in=(_i32(lens), 0),
               canon=None if c.canon is None else (_i32(c.canon), 0),
               state_off=(_i32(np.cumsum([0] + [a["S"] for a in c.automata])), 0),
               arc_off=(_i32(np.cumsum([0] + [len(a["src"]) for a in c.automata])), 0),
               src=(_i32(cat("src")), 0), cls=(_i32(cat("cls")), 1), dst=(_i32(cat("dst")), 0), accept=(_i32(cat("accept")), 0),
               arc_logw=_f32(cat("w")), final_logw=_f32(cat("fw")))                  # exactly E and S floats, NaN bands
    return c, lens, ms, ma, ins


@pytest.mark.parametrize("name", ["small", "big"])
def test_ctc_grammar_scores_weighted(name):
    from vistaocr_amd import _lib, ops
    c, lens, ms, ma, ins = _sweep(name)
    T, B, V = c.x.shape
    G = len(c.automata)
    nbytes = _lib.load().vocr_ctc_grammar_weighted_workspace_bytes(T, B, V, G, ms, ma, 1)
    assert nbytes > 0
    outs = dict(logp=((B, G), F32), best=((B, G), F32), labels=((B, G, T), I32), lens=((B, G), I32))

    def args(p, ws, nb, short=0):
        return (p["x"], p["lens_in"], T, B, V, p["canon"], p["state_off"], p["arc_off"], G, p["src"], p["cls"], p["dst"], p["accept"],
                p["arc_logw"], p["final_logw"], ms, ma, p["logp"], p["best"], p["labels"], p["lens"], T, ws, nb - short, ops._stream())

    run = cg.guarded_runs("vocr_ctc_grammar_scores_weighted", name, ins, outs, nbytes, args)
    cg.Call("vocr_ctc_grammar_scores_weighted", ins, outs, nbytes, lambda p, ws, nb: args(p, ws, nb, short=1),
            refuse=True).assert_nothing_launched(name)
    ref = wr.search(c.x, lens, c.automata, c.canon)
    frac = 0.0
    D = np.array([gr.max_in_degree(a) for a in c.automata])[None, :]
    N = np.array([a["S"] + len(a["src"]) for a in c.automata])[None, :]
    W = np.array([[wr.accumulated_weight(a, min(max(n, 0), T)) for a in c.automata] for n in lens])
    for got, want in ((run.host("logp"), ref["logp"]), (run.host("best"), ref["best"])):
        fin = want != NEG
        assert np.array_equal(got == NEG, ~fin), name
        bnd = wc.bound(np.clip(np.asarray(lens), 0, T)[:, None], np.where(fin, want, 0.0), D, N, W)
        frac = max(frac, float((np.abs(got - np.where(fin, want, 0.0)) / bnd)[fin].max()))
    assert frac <= 1.0, (name, frac)
    cg.row("vocr_ctc_grammar_scores_weighted", name, "%d automata, %d cells, staging %d" % (G, ms + ma, wc.staging(ms, ma)), frac, nbytes)


@pytest.mark.parametrize("name", ["small", "big"])
def test_ctc_grammar_grad_weighted(name):
    from vistaocr_amd import _lib, ops
    c, lens, ms, ma, ins = _sweep(name)
    T, B, V = c.x.shape
    G = len(c.automata)
    which = [b % G for b in range(B)]
    if name == "small":
        which[-1] = G
    w = np.array([1.5, -0.5, 2.0, -1.25][:B], dtype=np.float32)
    ins = dict(ins, which=(_i32(which), 0), weights=_f32(w))
    nbytes = _lib.load().vocr_ctc_grammar_grad_weighted_workspace_bytes(T, B, V, G, ms, ma, 1)
    assert nbytes > _lib.load().vocr_ctc_grammar_grad_workspace_bytes(T, B, V, G, ms, ma, 1) > 0
    outs = dict(logp=((B,), F32), dlogits=((T, B, V), F32))

    def args(p, ws, nb, short=0):
        return (p["x"], p["lens_in"], T, B, V, p["canon"], p["state_off"], p["arc_off"], G, p["src"], p["cls"], p["dst"], p["accept"],
                p["arc_logw"], p["final_logw"], ms, ma, p["which"], p["weights"], p["logp"], p["dlogits"], ws, nb - short, ops._stream())

    run = cg.guarded_runs("vocr_ctc_grammar_grad_weighted", name, ins, outs, nbytes, args)
    cg.Call("vocr_ctc_grammar_grad_weighted", ins, outs, nbytes, lambda p, ws, nb: args(p, ws, nb, short=1),
            refuse=True).assert_nothing_launched(name)
    ref = wr.run(c.x, lens, c.automata, which, c.canon, w.astype(np.float64))
    from tests.test_grammar_grad_gpu import _errors
    serr, gerr = _errors(name, run.out("dlogits").new_tensor(c.x), lens, run.out("logp"), run.out("dlogits"), ref, w)
    bar_s, bar_g = wc.bars(wc.GRAD_RECORDED["slack" if name == "small" else "max"])
    assert serr <= bar_s and gerr <= bar_g, (name, serr, gerr)
    cg.row("vocr_ctc_grammar_grad_weighted", name, "%d automata, %d cells, staging %d" % (G, ms + ma, wc.staging(ms, ma)),
           max(serr / bar_s, gerr / bar_g), nbytes)


@pytest.mark.parametrize("name", sorted(wc.GUARDED_BEAM))
def test_ctc_grammar_beam_search_weighted(name):
    from vistaocr_amd import _lib, ops
    seed, T, K, nbest, lens, which, with_lm = wc.GUARDED_BEAM[name]
    case = wc.guarded_beam_case(name)
    B, V = len(lens), 13
    grammars, x, lm, alpha, beta, gw = case.grammars, case.x, case.lm, case.alpha, case.beta, case.gw
    ref = wc.guarded_beam_reference(name)
    nbytes = _lib.load().vocr_ctc_grammar_beam_workspace_bytes(T, B, V, K, nbest)
    packed = pack_dense_grammars(grammars, "cpu")
    states = int(packed["dist"].numel())
    assert tuple(packed["logw"].shape) == (states, V) and tuple(packed["final"].shape) == (states,)
    tabs = lm.to("cpu") if with_lm else None
    S = int(tabs["lm_logp"].shape[0]) if with_lm else 0
    ins = dict(x=torch.from_numpy(x), lens_in=(_i32(lens), 0), state_off=(packed["state_off"], 1 << 30), next=(packed["next"], 1 << 30),
               dist=(packed["dist"], 0), logw=packed["logw"], final=packed["final"], which=(_i32(which), 0),
               lm_logp=tabs["lm_logp"] if with_lm else None, lm_next=(tabs["lm_next"], 1 << 30) if with_lm else None,
               lm_eos=tabs["lm_eos"] if with_lm else None)
    outs = dict(labels=((B, nbest, T), I32), lens=((B, nbest), I32), scores=((B, nbest, 3), F32), grammar=((B, nbest), F32))

    def args(p, ws, nb, short=0):
        return (p["x"], p["lens_in"], T, B, V, None, K, nbest, p["state_off"], p["next"], p["dist"], p["logw"], p["final"], 3, p["which"],
                p["lm_logp"], p["lm_next"], p["lm_eos"], S, int(tabs["start"]) if with_lm else 0, alpha, gw, beta, float("-inf"),
                p["labels"], p["lens"], p["scores"], p["grammar"], ws, nb - short, ops._stream())

    run = cg.guarded_runs("vocr_ctc_grammar_beam_search_weighted", name, ins, outs, nbytes, args)
    cg.Call("vocr_ctc_grammar_beam_search_weighted", ins, outs, nbytes, lambda p, ws, nb: args(p, ws, nb, short=1),
            refuse=True).assert_nothing_launched(name)
    lab, ln, sc, og = run.host("labels"), run.host("lens"), run.host("scores"), run.host("grammar")
    out_of_range = [b for b, k in enumerate(which) if not 0 <= k < 3]
    for b in out_of_range:
        assert not np.isfinite(sc[b, :, 0]).any() and not ln[b].any() and not og[b].any(), (name, b)
    bar = np.asarray(wc.bars(wc.BEAM_RECORDED["guarded"]))
    lines = [b for b in wc.decided(ref)]
    err = np.zeros(4)
    for b in lines:
        got = [lab[b, q, :ln[b, q]].tolist() for q in range(nbest) if np.isfinite(sc[b, q, 0])]
        assert got == [h[0] for h in ref[b].hyps], (name, b)
        for q, h in enumerate(ref[b].hyps):
            err = np.maximum(err, np.abs(np.append(sc[b, q], og[b, q]).astype(np.float64) - np.asarray(h[1:])))
    print("wgrammar-beam-errors %-12s group guarded  K %3d  compared %d/%d  max |score - fp64|: total %.2e acoustic %.2e lm %.2e grammar %.2e"
          % (name, K, len(lines), B, *err))
    assert 8 * (B - len(lines)) <= B and (err <= bar).all(), (name, len(lines), err, bar)     # at most 1/8 of the lines undecided
    cg.row("vocr_ctc_grammar_beam_search_weighted", name, "beam %d, nbest %d, 3 automata, %s" % (K, nbest, "LM tables" if with_lm else "no LM"),
           float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0, nbytes)
