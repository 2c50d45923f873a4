"""GPU: vocr_ctc_grammar_grad (vistaocr_amd/csrc/ctc_grammar.hip), ops.ctc_grammar_grad, GrammarMatcher.line_log_prob and
GrammarCTCLoss against the fp64 restatement of tests/grammar_grad_ref.py (itself held to central differences, a brute force over all
frame paths and the CTC references in tests/test_grammar_grad_cpu.py).

EVERY element of every output is compared, no line and no element left out: -inf exactly where the restatement has it and never a NaN;
exact zeros in the rows past `lens`, in every row of a line without a score, and in a column whose logit is -inf; the rest within the
family's tolerance.  Scores: |ln P - ref| / max(|ln P|, 1).  Gradient: per line, max |g - ref| / (the line's largest |ref|), with
weights of both signs.  The C entry is called with every buffer - outputs and workspace - NaN-filled first.

THE TOLERANCES are not derived: each family gets 4x the largest error it showed on an MI355X, rounded up to one digit
(profiles/ctc_grammar_grad_errors.txt lists the measured maxima; results are bit-identical from run to run, so the margin is for other
inputs of the same family, not for noise).  Every case prints its figures before it asserts ("grammar-grad-errors ...").  One cap
keeps a tolerance from hiding a fault: on the chain family the error must stay within 10x what vocr_ctc_nbest_grad shows on the very
same inputs (the two kernels compute the same quantity in the same arithmetic), and that is asserted, not only recorded.

What the shapes are for (the constants are the kernel's): a state with WAVE_DEG = 64 or more incoming arcs is scanned by a wave, not a
lane, in the forward plan (in-degree) and in the mirrored plan (out-degree): hubs of 63, 64, 65.  A call whose max_states + max_arcs
exceeds 2048 runs 1024 threads, else 256: trees of N = 2048 and 2049 cells.  The plan is staged in LDS while
16 N + 2048 + align16(16 max_arcs + 8 max_states + 4 (max_arcs / 64 + 2)) <= 147 KiB (plan_for): for the two-level tree of V = 70 that
holds up to N = 5296 (2649 states, 2647 arcs) and no longer at N = 5297 (2649, 2648).  N = 8192 is the largest automaton.  Chains of
L = 31, 32, 33 are the CTC kernels' one-wave seam, kept for the comparison with vocr_ctc_nbest_grad."""
import numpy as np
import pytest
import torch

from tests import align_ref as ar
from tests import ctc_ref as cr
from tests import grammar_grad_ref as gg
from tests import grammar_ref as gr
from tests.beam_data import dense_logits

pytestmark = pytest.mark.gpu
NAN = float("nan")
NEG = -np.inf
PEAKY = ("peaky", 8.0, 1.0)
CANON9 = [0, 1, 1, 3, 4, 4, 4, 7, 8]          # classes of 2 ({1, 2}) and 3 ({4, 5, 6}) members; V >= 9

# family: (scores, gradient) = 4x the maxima of profiles/ctc_grammar_grad_errors.txt, rounded up to one digit
TOL = {
    "chains_peaky": (9e-6, 6e-5),             # profiles/ctc_grammar_grad_errors.txt: 2.1e-06, 1.3e-05
    "chains_dense": (2e-6, 9e-4),             # profiles/ctc_grammar_grad_errors.txt: 3.4e-07, 2.1e-04
    "nbest_chain": (9e-6, 9e-4),              # vocr_ctc_nbest_grad on the chains' inputs, both regimes: 2.1e-06, 2.1e-04
    "degree": (8e-6, 4e-5),                   # profiles/ctc_grammar_grad_errors.txt: 1.8e-06, 7.7e-06
    "templates": (2e-5, 2e-4),                # profiles/ctc_grammar_grad_errors.txt: 3.1e-06, 3.4e-05
    "cells": (4e-6, 3e-5),                    # profiles/ctc_grammar_grad_errors.txt: 8.7e-07, 6.4e-06
    "lens": (3e-7, 9e-6),                     # profiles/ctc_grammar_grad_errors.txt: 5.8e-08, 2.2e-06
    "which": (4e-6, 2e-4),                    # profiles/ctc_grammar_grad_errors.txt: 1.0e-06, 3.6e-05
    "classes": (7e-6, 2e-4),                  # profiles/ctc_grammar_grad_errors.txt: 1.6e-06, 3.8e-05
    "nfa": (6e-6, 3e-4),                      # profiles/ctc_grammar_grad_errors.txt: 1.3e-06, 6.8e-05
    "criterion": (6e-6, 3e-4),                # profiles/ctc_grammar_grad_errors.txt: 1.5e-06, 5.6e-05
}


def _ops():
    from vistaocr_amd import ops
    return ops


def _pack(automata, max_states=None, max_arcs=None):
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    cat = lambda k: i32(np.concatenate([np.asarray(a[k], dtype=np.int32) for a in automata]))
    return {"state_off": i32(np.cumsum([0] + [a["S"] for a in automata])), "arc_off": i32(np.cumsum([0] + [len(a["src"]) for a in automata])),
            "src": cat("src"), "cls": cat("cls"), "dst": cat("dst"), "accept": cat("accept"),
            "max_states": max(a["S"] for a in automata) if max_states is None else max_states,
            "max_arcs": max(len(a["src"]) for a in automata) if max_arcs is None else max_arcs}


def _raw(x, lens, gp, which, canon=None, weights=None):
    """the C entry point itself, every buffer NaN-filled first; device tensors (logp [B], dlogits [T,B,V] or None)"""
    from vistaocr_amd import _lib
    ops = _ops()
    T, B, V = x.shape
    G = int(gp["state_off"].numel()) - 1
    nbytes = _lib.load().vocr_ctc_grammar_grad_workspace_bytes(T, B, V, G, gp["max_states"], gp["max_arcs"], 0 if weights is None else 1)
    assert nbytes > 0
    ws = torch.full(((nbytes + 3) // 4,), NAN, dtype=torch.float32, device=x.device)
    logp = torch.full((B,), NAN, dtype=torch.float32, device=x.device)
    dl = torch.full((T, B, V), NAN, dtype=torch.float32, device=x.device) if weights is not None else None
    p = ops._p
    _lib.call("vocr_ctc_grammar_grad", p(x), p(lens), T, B, V, p(canon), p(gp["state_off"]), p(gp["arc_off"]), G, p(gp["src"]), p(gp["cls"]),
              p(gp["dst"]), p(gp["accept"]), gp["max_states"], gp["max_arcs"], p(which), p(weights), p(logp), p(dl), p(ws), ws.numel() * 4,
              ops._stream())
    return logp, dl


def _weights(rng, B):
    """fp32 weights of both signs, away from 0"""
    w = rng.normal(0, 1, B)
    w = np.sign(w) * (0.5 + np.abs(w))
    w[::2] = -np.abs(w[::2])
    w[1::2] = np.abs(w[1::2])
    return w.astype(np.float32)


def _dev(x, lens, which, canon, w):
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return (x.float().contiguous().cuda(), torch.tensor([int(v) for v in lens], dtype=torch.int32).cuda(),
            torch.tensor([int(v) for v in which], dtype=torch.int32).cuda(),
            None if canon is None else torch.tensor(canon, dtype=torch.int32).cuda(),
            None if w is None else torch.from_numpy(np.asarray(w, dtype=np.float32)).cuda())


def _errors(name, x, lens, logp, grad, ref, w=None):
    """the exact parts asserted; (score error, gradient error) in the units of TOL.  A line whose automaton accepts EVERY labelling
    (the template [GAP]) has P = 1 and a gradient that is identically zero: the restatement returns its own fp64 rounding there
    (|ln P| and |g| of 1e-16), and a ratio to that measures nothing.  Such a line (|ln P_ref| < 1e-12) is held to the scale every
    element has before the cancellation instead, max |g| / |w_b| (each element is w_b p (occ / P - 1) with |p (occ / P - 1)| <= 1): it
    is compared, against the same tolerance, not left out."""
    T, B, V = x.shape
    got_p = logp.cpu().double().numpy()
    assert not np.isnan(got_p).any() and not (got_p == np.inf).any(), (name, got_p)
    fin = ref["logp"] != NEG
    assert np.array_equal(got_p == NEG, ~fin), (name, got_p, ref["logp"])
    serr = float((np.abs(got_p[fin] - ref["logp"][fin]) / np.maximum(np.abs(ref["logp"][fin]), 1.0)).max()) if fin.any() else 0.0
    gerr = 0.0
    if grad is not None:
        got_g, g = grad.cpu().double().numpy(), ref["grad"]
        assert np.isfinite(got_g).all(), name
        xn = np.asarray(x.cpu().numpy() if torch.is_tensor(x) else x)
        for b in range(B):
            n = min(max(int(lens[b]), 0), T)
            assert float(np.abs(got_g[n:, b]).max() if n < T else 0.0) == 0.0, (name, b)
            assert float(np.abs(got_g[:, b][xn[:, b] == NEG]).max() if (xn[:, b] == NEG).any() else 0.0) == 0.0, (name, b)
            top = float(np.abs(g[:, b]).max())
            if not fin[b] or top == 0.0:
                assert float(np.abs(got_g[:, b]).max()) == 0.0, (name, b)
            elif abs(ref["logp"][b]) < 1e-12 and n > 0:
                assert w is not None and top < 1e-12 * abs(float(w[b])), (name, b, top)
                gerr = max(gerr, float(np.abs(got_g[:, b] - g[:, b]).max()) / abs(float(w[b])))
            else:
                gerr = max(gerr, float(np.abs(got_g[:, b] - g[:, b]).max()) / top)
    return serr, gerr


def _check(name, family, x, lens, automata, which, canon=None, seed=0, max_states=None, max_arcs=None, need_finite=1):
    """one call against the restatement; returns (device inputs, logp, grad, ref, serr, gerr)"""
    T, B, V = x.shape
    w = _weights(np.random.default_rng([17, seed]), B)
    ref = gg.run(x, lens, automata, which, canon, w.astype(np.float64), max_states, max_arcs)
    gp = _pack(automata, max_states, max_arcs)
    xd, ld, wd, cd, wt = _dev(x, lens, which, canon, w)
    logp, grad = _raw(xd, ld, gp, wd, cd, wt)
    serr, gerr = _errors(name, xd, lens, logp, grad, ref, w)
    fin = ref["logp"] != NEG
    print("grammar-grad-errors %-22s family %-13s T %3d B %2d V %3d G %2d cells <= %4d  finite %2d / %2d  max |lnP| %8.3f  score %.1e  grad %.1e"
          % (name, family, T, B, V, len(automata), gp["max_states"] + gp["max_arcs"], int(fin.sum()), B,
             float(np.abs(ref["logp"][fin]).max()) if fin.any() else 0.0, serr, gerr))
    assert int(fin.sum()) >= need_finite, (name, ref["logp"])
    tol_s, tol_g = TOL[family]
    assert serr <= tol_s and gerr <= tol_g, (name, serr, gerr)
    return (xd, ld, gp, wd, cd, wt), logp, grad, ref, serr, gerr


def _chain(labels):
    return gr.make(len(labels) + 1, [(i, c, i + 1) for i, c in enumerate(labels)], [len(labels)])


def _peaky(rng, T, V, labs, lens):
    """peaky along a random alignment of labs[b] (a line whose labelling does not fit gets noise alone)"""
    fit = [l if cr.need(l) <= n else [] for l, n in zip(labs, lens)]
    return cr.build_logits(rng, T, len(labs), V, fit, lens, PEAKY).numpy()


# --------------------------------------------------------------------------------------------------------------------- chains
_CHAIN_L = [0, 1, 31, 32, 33, 20]
_CHAIN_LENS = [70, 69, 70, 68, 70, 66]


@pytest.mark.parametrize("regime", ["peaky", "dense"])
@pytest.mark.parametrize("kind", ["random", "equal", "abab"])
def test_chains_against_fp64_and_the_nbest_kernel(kind, regime):
    """L = 0, 1, 31, 32, 33 (and 20) labels, ragged lens; 33 equal labels take 65 of the line's 70 frames.  The same inputs through
    vocr_ctc_nbest_grad with n = 1: the two agree within the sum of their tolerances, and this kernel's error stays within 10x the
    other's."""
    T, B, V = 70, 6, 40
    rng = np.random.default_rng([1, ["random", "equal", "abab"].index(kind), regime == "dense"])
    labs = [cr.make_labels(rng, V, L, kind) for L in _CHAIN_L]
    assert all(cr.need(l) <= n for l, n in zip(labs, _CHAIN_LENS))
    x = _peaky(rng, T, V, labs, _CHAIN_LENS) if regime == "peaky" else dense_logits(rng, T, B, V, 3.0)
    family = "chains_" + regime
    name = "chains_%s_%s" % (kind, regime)
    (xd, ld, gp, wd, cd, wt), logp, grad, ref, serr, gerr = _check(name, family, x, _CHAIN_LENS, [_chain(l) for l in labs], range(B), seed=1)
    M = max(len(l) for l in labs)
    lab = np.zeros((B, 1, M), dtype=np.int32)
    for b, l in enumerate(labs):
        lab[b, 0, :len(l)] = l
    ll = torch.tensor([[len(l)] for l in labs], dtype=torch.int32).cuda()
    nb_p, nb_g = _ops().ctc_nbest(xd, ld, torch.from_numpy(lab).cuda(), ll, None, wt.reshape(B, 1))
    n_serr, n_gerr = _errors(name + "/nbest", xd, _CHAIN_LENS, nb_p[:, 0], nb_g, ref)
    d_s = float(((logp - nb_p[:, 0]).abs().cpu().double().numpy() / np.maximum(np.abs(ref["logp"]), 1.0)).max())
    d_g = max(float((grad[:, b] - nb_g[:, b]).abs().max()) / float(np.abs(ref["grad"][:, b]).max()) for b in range(B))
    print("grammar-grad-errors %-22s vocr_ctc_nbest_grad on the same inputs: score %.1e  grad %.1e;  between the two kernels: score %.1e  "
          "grad %.1e" % (name, n_serr, n_gerr, d_s, d_g))
    assert n_serr <= TOL["nbest_chain"][0] and n_gerr <= TOL["nbest_chain"][1], (name, n_serr, n_gerr)
    assert d_s <= TOL[family][0] + TOL["nbest_chain"][0] and d_g <= TOL[family][1] + TOL["nbest_chain"][1], (name, d_s, d_g)
    assert serr <= 10 * n_serr and gerr <= 10 * n_gerr, (name, serr, n_serr, gerr, n_gerr)


# --------------------------------------------------------------------------------------------------------------------- degree
def _hub(D, V):
    """0 -(classes 1..D)-> 1..D -(mixed classes)-> hub H -(classes 1..D)-> leaves: H has D incoming arcs in groups of several
    sizes, H and 0 have D outgoing arcs.  H and the leaves accept."""
    H = D + 1
    arcs = [(0, c, c) for c in range(1, D + 1)]
    arcs += [(i, 1 + (i * 7) % 5 + (0 if i % 3 else 20), H) for i in range(1, D + 1)]
    arcs += [(H, c, H + c) for c in range(1, D + 1)]
    return gr.make(H + D + 1, arcs, range(H, H + D + 1), V=V)


@pytest.mark.parametrize("regime", ["peaky", "dense"])
def test_hub_states_of_63_64_65_arcs(regime):
    T, V = 12, 70
    autos = [_hub(D, V) for D in (63, 64, 65)]
    assert [gr.max_in_degree(a) for a in autos] == [63, 64, 65]
    assert [int(np.bincount(a["src"]).max()) for a in autos] == [63, 64, 65]
    rng = np.random.default_rng([2, regime == "dense"])
    which = [0, 1, 2, 2, 1, 0]
    lens = [12, 12, 12, 11, 9, 12]
    if regime == "peaky":
        labs = []                                                  # 0 -i-> i -> H -j-> a leaf
        for k in which:
            i = int(rng.integers(1, 60))
            labs.append([i, int(autos[k]["cls"][np.nonzero(autos[k]["src"] == i)[0][0]]), int(rng.integers(1, 60))])
        x = _peaky(rng, T, V, labs, lens)
    else:
        x = dense_logits(rng, T, len(which), V, 3.0)
    _check("degree_" + regime, "degree", x, lens, autos, which, seed=2, need_finite=6)


# ------------------------------------------------------------------------------------------------------------------ templates
def _alphabet(V):
    import vistaocr_amd as va
    return va.Alphabet(["<ctc-blank>"] + ["u%04x" % (0x61 + i) for i in range(V - 1)])


def _template_cases(AL):
    from vistaocr_amd import Grammar
    A, G = Grammar.ANY, Grammar.GAP
    # (items, a labelling it accepts)
    return [
        ([1, 2, G, 3, 4], [1, 2, 9, 9, 5, 3, 4]),
        ([G, 5, 6, 7], [8, 5, 5, 6, 7]),
        ([5, 6, 7, G], [5, 6, 7, 7, 1]),
        ([G], [3, 1, 4, 1, 5]),
        ([A], [11]),
        ([1, {2, 3, 4}, A, [5, 6]], [1, 3, 1, 6]),
        ([2, G, 2], [2, 2]),
        ([2, 2, G, 2, 2], [2, 2, 7, 2, 2, 2]),
        ([G, 1, G, 2, G], [1, 2]),
    ]


@pytest.mark.parametrize("regime", ["peaky", "dense"])
def test_templates(regime):
    from vistaocr_amd import Grammar
    T, V = 40, 30
    AL = _alphabet(V)
    cases = _template_cases(AL)
    grammars = [Grammar.from_template(AL, items) for items, _ in cases]
    for g, (_, lab) in zip(grammars, cases):
        assert g.accepts(lab)
    autos = [gr.from_grammar(g) for g in grammars]
    B = len(cases)
    lens = [40, 39, 40, 37, 40, 40, 40, 33, 40]
    rng = np.random.default_rng([3, regime == "dense"])
    x = _peaky(rng, T, V, [lab for _, lab in cases], lens) if regime == "peaky" else dense_logits(rng, T, B, V, 3.0)
    _check("templates_" + regime, "templates", x, lens, autos, range(B), seed=3, need_finite=B)


# ---------------------------------------------------------------------------------------------------------------------- cells
def _tree(V, N):
    """A deterministic two-level tree of exactly N = S + E cells (the leaves and the inner states accept; an odd cell is one unreachable
    state): in-degree 1 everywhere."""
    n, extra = divmod(N - (2 * V - 1), 2)
    assert 0 <= n <= (V - 1) ** 2
    arcs = [(0, c, c) for c in range(1, V)]
    for i in range(n):
        arcs.append((1 + i // (V - 1), 1 + i % (V - 1), V + i))
    a = gr.make(V + n + extra, arcs, range(1, V + n), V=V)
    assert a["S"] + len(a["src"]) == N
    return a


@pytest.mark.parametrize("N", [2048, 2049, 5296, 5297, 8192])
def test_trees_across_the_thread_and_staging_limits(N):
    """one peaky and one dense line against the same automaton"""
    T, V = 16, 70
    a = _tree(V, N)
    rng = np.random.default_rng([4, N])
    x = dense_logits(rng, T, 2, V, 3.0)
    x[:, 0] = _peaky(rng, T, V, [[3, 5]], [16])[:, 0]
    _check("cells_%d" % N, "cells", x, [16, 13], [a], [0, 0], seed=4, need_finite=2)


# ------------------------------------------------------------------------------------------------------- lens, which, classes, nfa
def test_lens_0_1_2_T_and_a_start_state_that_accepts():
    T, V = 9, 6
    star = gr.make(2, [(0, 1, 1), (1, 2, 0)], [0], V=V)            # (ab)*: the start accepts
    chain = _chain([1, 2])
    rng = np.random.default_rng(5)
    lens = [0, 1, 2, T, 0, 1, 2, T]
    which = [0, 0, 0, 0, 1, 1, 1, 1]
    x = dense_logits(rng, T, 8, V, 2.0)
    _, logp, grad, ref, _, _ = _check("lens", "lens", x, lens, [star, chain], which, seed=5, need_finite=6)
    got = logp.cpu().numpy()
    assert got[0] == 0.0 and got[4] == NEG and got[5] == NEG and np.isfinite(got[[1, 2, 3, 6, 7]]).all()
    assert float(grad[:, [0, 4, 5]].abs().max()) == 0.0


def test_which_pairs_a_line_with_its_automaton_and_poisons_only_its_own_lines():
    """shared automata; which = -1 and = G; an automaton whose arcs are not sorted"""
    T, V = 20, 12
    rng = np.random.default_rng(6)
    good0, good1 = _chain([3, 3, 5]), gr.make(3, [(0, 1, 1), (0, 2, 2), (1, 4, 2), (2, 4, 2)], [2], V=V)
    bad = _chain([4, 6, 2])
    bad = dict(bad, src=bad["src"][::-1].copy(), cls=bad["cls"][::-1].copy(), dst=bad["dst"][::-1].copy())
    assert not gr.valid(bad, V, ar.classes_of(V), 4, 4)
    autos = [good0, bad, good1]
    which = [0, 1, 2, -1, 3, 0, 2, 1]
    lens = [20, 20, 19, 20, 20, 17, 20, 11]
    x = dense_logits(rng, T, 8, V, 2.0)
    x[:, :3] = _peaky(rng, T, V, [[3, 3, 5], [4, 6, 2], [1, 4]], lens[:3])
    (xd, ld, gp, wd, cd, wt), logp, grad, ref, _, _ = _check("which", "which", x, lens, autos, which, seed=6, need_finite=4)
    assert [bool(v) for v in np.isfinite(logp.cpu().numpy())] == [True, False, True, False, False, True, True, False]
    # the good lines have the bits of a call that holds them alone, with their automata alone
    keep = [0, 2, 5, 6]
    sub = torch.tensor(keep).cuda()
    re_which = torch.tensor([0, 1, 0, 1], dtype=torch.int32).cuda()
    gp2 = _pack([good0, good1], gp["max_states"], gp["max_arcs"])
    l2, g2 = _raw(xd[:, sub].contiguous(), ld[sub].contiguous(), gp2, re_which, None, wt[sub].contiguous())
    assert torch.equal(l2, logp[sub]) and torch.equal(g2, grad[:, sub])


@pytest.mark.parametrize("regime", ["peaky", "dense"])
def test_symbol_classes_and_columns_at_minus_infinity(regime):
    """CANON9; an arc class given as a non-canonical member (2 for class 1, 6 for class 4); one member of the 3-class at -inf
    everywhere, one of the 2-class on a line, a whole class (both members) on another; a line whose only route needs a dead class"""
    T, V = 30, 12
    canon = CANON9 + list(range(9, V))
    cls = ar.classes_of(V, canon)
    a0 = gr.make(4, [(0, 2, 1), (1, 6, 2), (2, 3, 3), (2, 9, 3)], [3], V=V, canon=canon)
    a1 = gr.make(3, [(0, 1, 1), (1, 7, 1), (1, 4, 2), (0, 10, 2)], [2], V=V, canon=canon)
    a2 = _chain([7, 1, 8])
    rng = np.random.default_rng([7, regime == "dense"])
    lens = [30, 29, 30, 22, 30]
    which = [0, 1, 0, 1, 2]
    if regime == "peaky":
        x = _peaky(rng, T, V, [[1, 4, 3], [1, 7, 4], [1, 4, 9], [10], [7, 1, 8]], lens)
    else:
        x = dense_logits(rng, T, 5, V, 3.0)
    x[:, :, 5] = NEG
    x[:, 0, 2] = NEG
    x[:, 1, 9] = NEG
    x[:, 3, 1] = NEG
    x[:, 3, 2] = NEG                                               # class 1 is dead on line 3: its automaton is left with 0 -10-> 2
    x[:, 4, 1] = NEG
    x[:, 4, 2] = NEG                                               # ... and line 4's chain has no path
    _, logp, grad, ref, _, _ = _check("classes_" + regime, "classes", x, lens, [a0, a1, a2], which, canon, seed=7, need_finite=4)
    assert ref["logp"][4] == NEG and np.isfinite(ref["logp"][:4]).all()
    assert int(cls[2]) == 1 and int(cls[6]) == 4


def test_a_non_deterministic_automaton():
    """two arcs with the same (src, class) to different states, (dst, class) groups of more than one arc: the gradient of the sum over
    (frame path, automaton path) pairs"""
    T, V = 18, 8
    arcs = [(0, 1, 1), (0, 1, 2), (1, 2, 3), (2, 2, 3), (2, 3, 3), (1, 3, 3), (3, 1, 3), (0, 2, 3), (3, 4, 0)]
    a = gr.make(4, arcs, [3], V=V)
    rng = np.random.default_rng(8)
    x = dense_logits(rng, T, 3, V, 2.0)
    x[:, 0] = _peaky(rng, T, V, [[1, 2, 1, 4, 2]], [18])[:, 0]
    _check("nfa", "nfa", x, [18, 17, 5], [a], [0, 0, 0], seed=8, need_finite=3)


# ----------------------------------------------------------------------------------------------------------------------- bits
def test_bits_runs_scores_entry_and_batch_permutation():
    from vistaocr_amd import Grammar
    ops = _ops()
    T, V, B = 24, 30, 6
    AL = _alphabet(V)
    grammars = [Grammar.from_template(AL, [1, 2, Grammar.GAP, 3]), Grammar.from_labels(AL, [4, 4, 5]),
                Grammar.from_regex(AL, "ab*(c|d)+"), Grammar.from_template(AL, [Grammar.GAP, 7, Grammar.ANY])]
    autos = [gr.from_grammar(g) for g in grammars]
    gp = _pack(autos)
    rng = np.random.default_rng(9)
    which = [0, 1, 2, 3, 0, 2]
    lens = [24, 23, 24, 20, 11, 24]
    x = dense_logits(rng, T, B, V, 3.0)
    xd, ld, wd, _, wt = _dev(x, lens, which, None, _weights(rng, B))
    logp, grad = _raw(xd, ld, gp, wd, None, wt)
    logp2, grad2 = _raw(xd, ld, gp, wd, None, wt)
    assert torch.equal(logp, logp2) and torch.equal(grad, grad2)
    logp3, none = _raw(xd, ld, gp, wd, None, None)                 # scores only
    assert none is None and torch.equal(logp3, logp)
    l4, g4 = ops.ctc_grammar_grad(xd, lens, gp, wd, None, wt)      # the Python entry: its own uninitialised buffers
    assert torch.equal(l4, logp) and torch.equal(g4, grad)
    table = ops.ctc_grammar_scores(xd, ld, gp, None, False)[0]     # [B, G]
    assert torch.equal(table[torch.arange(B), wd.long()], logp)
    assert bool(torch.isfinite(logp).all())
    # a line's rows depend on that line and its automaton alone: the batch permuted, the other lines' grammars swapped
    perm = [3, 5, 0, 4, 1, 2]
    pt = torch.tensor(perm).cuda()
    lp, gpm = _raw(xd[:, pt].contiguous(), ld[pt].contiguous(), gp, wd[pt].contiguous(), None, wt[pt].contiguous())
    assert torch.equal(lp, logp[pt]) and torch.equal(gpm, grad[:, pt])
    for b in range(B):
        other = wd.clone()
        other[:] = (wd + 1) % len(autos)
        other[b] = wd[b]
        lo, go = _raw(xd, ld, gp, other, None, wt)
        assert torch.equal(lo[b], logp[b]) and torch.equal(go[:, b], grad[:, b]), b


# ------------------------------------------------------------------------------------------------------------------ criterion
def _run(crit, x, flat, act, ll, scale=1.0):
    xd = x.cuda().requires_grad_(True)
    loss = crit(xd, flat, act, ll)
    assert tuple(loss.shape) == (1,)
    (scale * loss).backward()
    return float(loss.detach()), xd.grad.cpu().double().numpy()


def _criterion_case(regime, feasible_only):
    """mix64 of tests/ctc_ref.py (T 60, B 4, V 96, up to 31 labels); one of its lines has no alignment"""
    x, _, _, act, labs = cr.build_case("mix64", regime)
    keep = [b for b in range(len(labs)) if not feasible_only or cr.need(labs[b]) <= act[b]]
    labs, act = [labs[b] for b in keep], [int(act[b]) for b in keep]
    flat = torch.tensor([v for l in labs for v in l], dtype=torch.int32)
    return (x[:, keep].contiguous(), flat, torch.tensor(act, dtype=torch.int32), torch.tensor([len(l) for l in labs], dtype=torch.int32),
            labs, act)


# mix64 in profiles/ctc_fp64_errors.txt: max abs error of nll per line, of dlogits per element, (dense_3, peaky_8_1)
CTC_RECORDED = {cr.DENSE: (3.22e-05, 5.31e-05), cr.PEAKY8: (3.84e-06, 2.02e-06)}


@pytest.mark.parametrize("regime", [cr.DENSE, cr.PEAKY8])
def test_exact_criterion_is_the_ctc_loss(regime):
    """loss and logits gradient against CTCLoss, another kernel, within the sum of the two kernels' errors against fp64; with the line
    that cannot be aligned both give +inf, and this criterion gives that line zero rows"""
    import vistaocr_amd as va
    AL = _alphabet(96)
    x, flat, act, ll, labs, lens = _criterion_case(regime, True)
    ref = gg.run(x.numpy(), lens, [_chain(l) for l in labs], range(len(labs)), None, -np.ones(len(labs)))
    e_nll, e_grad = CTC_RECORDED[regime]
    tol_s, tol_g = TOL["criterion"]
    crit = va.GrammarCTCLoss.exact(AL)
    ctc, own = _run(va.CTCLoss(), x, flat, act, ll), _run(crit, x, flat, act, ll)
    lnp = ref["logp"]
    serr = float((np.abs(crit.last_logp.cpu().double().numpy() - lnp) / np.maximum(np.abs(lnp), 1.0)).max())
    gerr = max(float(np.abs(own[1][:, b] - ref["grad"][:, b]).max()) / float(np.abs(ref["grad"][:, b]).max()) for b in range(len(labs)))
    d_loss = abs(ctc[0] - own[0])
    bar_loss = float((e_nll + tol_s * np.maximum(np.abs(lnp), 1.0)).sum()) + 4 * cr.U * float(np.abs(lnp).sum())
    worst = max(float(np.abs(ctc[1][:, b] - own[1][:, b]).max()) / (e_grad + tol_g * float(np.abs(ref["grad"][:, b]).max()))
                for b in range(len(labs)))
    print("grammar-grad-errors criterion exact %-9s  score %.1e  grad %.1e  loss %.6f / CTCLoss %.6f  diff %.2e / bar %.2e  grad diff / bar "
          "%.3f" % (regime[0], serr, gerr, own[0], ctc[0], d_loss, bar_loss, worst))
    assert serr <= tol_s and gerr <= tol_g
    assert d_loss <= bar_loss and worst <= 1.0
    assert tuple(crit.last_logp.shape) == (len(labs),) and crit.last_logp.is_cuda
    x, flat, act, ll, labs, lens = _criterion_case(regime, False)
    ctc, own = _run(va.CTCLoss(), x, flat, act, ll), _run(va.GrammarCTCLoss.exact(AL), x, flat, act, ll)
    assert ctc[0] == float("inf") and own[0] == float("inf")
    assert float(np.abs(own[1][:, 0]).max()) == 0.0 and float(np.abs(own[1][:, 1:]).max()) > 0 and np.isfinite(own[1]).all()


def _gapped_batch(rng, T, V, gap, any_char):
    labs = [[1, 2, gap, 3, 4], [gap, 5, 6], [7, any_char, 8, gap], [1, 2, gap, 3, 4], [9, 9, 10]]
    said = [[1, 2, 11, 12, 3, 4], [13, 5, 6], [7, 14, 8], [1, 2, 3, 4], [9, 9, 10]]
    lens = [T, T - 1, T, T - 5, T]
    return labs, said, lens


@pytest.mark.parametrize("regime", ["peaky", "dense"])
def test_with_gaps_against_fp64_scaled_and_chunked(regime):
    """the gapped criterion against the restatement on the grammars it builds; dloss = 2.5 scales the saved gradient; a lattice limit
    that forces one, two and three lines per call gives the bits of the single call"""
    import vistaocr_amd as va
    T, V = 40, 30
    AL = _alphabet(V)
    gap, any_char = V - 1, V - 2
    rng = np.random.default_rng([10, regime == "dense"])
    labs, said, lens = _gapped_batch(rng, T, V, gap, any_char)
    x = torch.from_numpy(_peaky(rng, T, V, said, lens) if regime == "peaky" else dense_logits(rng, T, len(labs), V, 3.0))
    flat = torch.tensor([v for l in labs for v in l], dtype=torch.int32)
    act, ll = torch.tensor(lens, dtype=torch.int32), torch.tensor([len(l) for l in labs], dtype=torch.int32)
    crit = va.GrammarCTCLoss.with_gaps(AL, gap, any_char)
    loss, grad = _run(crit, x, flat, act, ll, 2.5)
    grammars, which = crit.batch_grammars(flat.tolist(), ll.tolist())
    assert which == [0, 1, 2, 0, 3] and crit.cache_misses == 4
    for g in grammars:                                             # the reserved labels are on no arc
        assert gap not in g.arc_cls.tolist() and any_char not in g.arc_cls.tolist()
    ref = gg.run(x.numpy(), lens, [gr.from_grammar(g) for g in grammars], which, None, -np.ones(len(labs)))
    assert np.isfinite(ref["logp"]).all()
    lnp = ref["logp"]
    serr = float((np.abs(crit.last_logp.cpu().double().numpy() - lnp) / np.maximum(np.abs(lnp), 1.0)).max())
    gerr = max(float(np.abs(grad[:, b] - 2.5 * ref["grad"][:, b]).max()) / (2.5 * float(np.abs(ref["grad"][:, b]).max()))
               for b in range(len(labs)))
    print("grammar-grad-errors criterion gaps  %-9s  score %.1e  grad %.1e  loss %.6f want %.6f" % (regime, serr, gerr, loss, -lnp.sum()))
    tol_s, tol_g = TOL["criterion"]
    assert serr <= tol_s and gerr <= tol_g
    assert abs(loss + lnp.sum()) <= tol_s * float(np.maximum(np.abs(lnp), 1.0).sum()) + 4 * cr.U * abs(lnp.sum())
    one = _ops().grammar_lattice_bytes(T, 1, max(g.n_states for g in grammars), max(g.n_arcs for g in grammars))
    for per in (1, 2, 3):
        cut = va.GrammarCTCLoss.with_gaps(AL, gap, any_char, max_lattice_bytes=per * one)
        loss2, grad2 = _run(cut, x, flat, act, ll, 2.5)
        assert loss2 == loss and np.array_equal(grad2, grad) and torch.equal(cut.last_logp, crit.last_logp), per
    with pytest.raises(ValueError, match="exceed the limit"):
        va.GrammarCTCLoss.with_gaps(AL, gap, any_char, max_lattice_bytes=one - 1)(x.cuda(), flat, act, ll)
    # GrammarMatcher.line_log_prob: the same numbers with autograd per line
    m = va.GrammarMatcher(AL)
    xd = x.cuda().requires_grad_(True)
    lp = m.line_log_prob(xd, lens, grammars, which)
    assert torch.equal(lp.detach(), crit.last_logp)
    (-2.5 * lp).sum().backward()
    assert np.array_equal(xd.grad.cpu().double().numpy(), grad)
    lp_cut = m.line_log_prob(xd, lens, grammars, which, max_lattice_bytes=2 * one)
    assert torch.equal(lp_cut.detach(), lp.detach())
    with torch.no_grad():
        assert torch.equal(m.line_log_prob(xd, lens, grammars, which), lp.detach())


def _tiny_model(AL):
    import vistaocr_amd as va
    torch.manual_seed(0)
    model = va.CnnOcrModel(alphabet=AL, verbose=False, input_line_height=30, rds_line_height=30, lstm_input_dim=32, num_lstm_layers=1,
                           num_lstm_hidden_units=32, p_lstm_dropout=0.0, num_in_channels=1)
    model.train()
    return model


def test_three_training_steps_with_gapped_targets():
    import vistaocr_amd as va
    ops = _ops()
    AL = va.english_alphabet()
    gap = AL.char_to_idx["u002a"]                                  # '*' stands for "anything"
    model = _tiny_model(AL)
    opt = va.make_optimizer(model, lr=1e-3)
    crit = va.GrammarCTCLoss.with_gaps(AL, "*")
    g = torch.Generator().manual_seed(5)
    nb, width, L = 4, 200, 5
    targets = torch.randint(1, 60, (nb, L), generator=g).to(torch.int32)
    targets[:, 2] = gap
    targets[1, 0] = gap
    batch = (torch.rand(nb, 1, 30, width, generator=g), targets.reshape(-1), torch.full((nb,), width, dtype=torch.int32),
             torch.full((nb,), L, dtype=torch.int32), {})
    before = torch.cat([p.detach().reshape(-1).clone() for p in model.parameters()])
    for _ in range(3):
        value = va.train(batch, model, crit, opt)
        assert isinstance(value, float) and np.isfinite(value)
    after = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert bool(torch.isfinite(after).all()) and float((after - before).abs().max()) > 0
    assert bool(torch.isfinite(crit.last_logp).all()) and crit.cache_misses == 4 and crit.cache_hits == 8
    ops.check_health_sync(torch.device("cuda", torch.cuda.current_device()))
