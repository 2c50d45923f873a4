"""GPU: the weighted grammars' three kernels - vocr_ctc_grammar_scores_weighted, vocr_ctc_grammar_grad_weighted (csrc/ctc_grammar.hip,
the WT instantiations) and vocr_ctc_grammar_beam_search_weighted (csrc/ctc_beam.hip, WEIGHTED) - and their Python surface against the
fp64 restatements of tests/wgrammar_ref.py (held to brute force and central differences in tests/test_wgrammar_cpu.py), on the pinned
inputs of tests/wgrammar_cases.py.

Bars (tests/wgrammar_cases.py says where they come from): sweep scores within the DERIVED bound; gradients and beam scores within 4 x
the recorded error; and, whatever the recorded error says, within 10 x what the existing UNWEIGHTED entry shows on the same logits and
automaton, measured in the same test.  Every case prints its figures before it asserts (-s; profiles/ctc_wgrammar_errors.txt keeps a
run's output).  Shapes: T = 12 and B <= 4 for the sweeps, B = 8 for the beam cases (so that one undecided line in eight may be
dropped), the smallest automata that reach each branch of the host plan."""
import numpy as np
import pytest
import torch

from tests import align_ref as ar
from tests import beam_cases as bc
from tests import grammar_beam_cases as gc
from tests import grammar_beam_ref as gbr
from tests import grammar_grad_ref as gg
from tests import grammar_ref as gr
from tests import wgrammar_cases as wc
from tests import wgrammar_ref as wr

pytestmark = pytest.mark.gpu
NEG = -np.inf
NAN = float("nan")
F32, I32 = torch.float32, torch.int32


def _ops():
    from vistaocr_amd import ops
    return ops


def _grad_errors(*a, **k):
    from tests.test_grammar_grad_gpu import _errors
    return _errors(*a, **k)


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def _pack(automata, max_states=None, max_arcs=None, weights=True):
    cat = lambda k, dt: _t(np.concatenate([np.asarray(a[k]) for a in automata]), dt)
    gp = {"state_off": _t(np.cumsum([0] + [a["S"] for a in automata]), np.int32),
          "arc_off": _t(np.cumsum([0] + [len(a["src"]) for a in automata]), np.int32),
          "src": cat("src", np.int32), "cls": cat("cls", np.int32), "dst": cat("dst", np.int32), "accept": cat("accept", np.int32),
          "max_states": max(a["S"] for a in automata) if max_states is None else max_states,
          "max_arcs": max(len(a["src"]) for a in automata) if max_arcs is None else max_arcs}
    if weights:
        gp["arc_logw"], gp["final_logw"] = cat("w", np.float32), cat("fw", np.float32)
    return gp


def _dev(x, lens, canon=None):
    return (_t(x, np.float32), torch.tensor([int(v) for v in lens], dtype=I32).cuda(), None if canon is None else _t(canon, np.int32))


def _weights(B, seed):
    from tests.test_grammar_grad_gpu import _weights as w
    return w(np.random.default_rng([23, seed]), B)


# ---- the C entries themselves, every output and the workspace NaN- or poison-filled first
def _raw_scores(xd, ld, gp, cd, aw, fw):
    from vistaocr_amd import _lib
    p = _ops()._p
    T, B, V = xd.shape
    G = gp["state_off"].numel() - 1
    nbytes = _lib.load().vocr_ctc_grammar_weighted_workspace_bytes(T, B, V, G, gp["max_states"], gp["max_arcs"], 1)
    ws = torch.full((nbytes // 4,), NAN, dtype=F32, device="cuda")
    logp, best = torch.full((B, G), NAN, dtype=F32, device="cuda"), torch.full((B, G), NAN, dtype=F32, device="cuda")
    lab, ln = torch.full((B, G, T), -7, dtype=I32, device="cuda"), torch.full((B, G), -7, dtype=I32, device="cuda")
    _lib.call("vocr_ctc_grammar_scores_weighted", p(xd), p(ld), T, B, V, p(cd), p(gp["state_off"]), p(gp["arc_off"]), G, p(gp["src"]),
              p(gp["cls"]), p(gp["dst"]), p(gp["accept"]), p(aw), p(fw), gp["max_states"], gp["max_arcs"], p(logp), p(best), p(lab), p(ln), T,
              p(ws), nbytes, _ops()._stream())
    return logp, best, lab, ln


def _raw_grad(xd, ld, gp, wd, cd, wt, aw, fw):
    from vistaocr_amd import _lib
    p = _ops()._p
    T, B, V = xd.shape
    G = gp["state_off"].numel() - 1
    nbytes = _lib.load().vocr_ctc_grammar_grad_weighted_workspace_bytes(T, B, V, G, gp["max_states"], gp["max_arcs"], 1)
    ws = torch.full((nbytes // 4,), NAN, dtype=F32, device="cuda")
    logp, dl = torch.full((B,), NAN, dtype=F32, device="cuda"), torch.full((T, B, V), NAN, dtype=F32, device="cuda")
    _lib.call("vocr_ctc_grammar_grad_weighted", p(xd), p(ld), T, B, V, p(cd), p(gp["state_off"]), p(gp["arc_off"]), G, p(gp["src"]),
              p(gp["cls"]), p(gp["dst"]), p(gp["accept"]), p(aw), p(fw), gp["max_states"], gp["max_arcs"], p(wd), p(wt), p(logp), p(dl),
              p(ws), nbytes, _ops()._stream())
    return logp, dl


def _raw_beam(xd, ld, dp, which, cd, K, nbest, lm, alpha, gw, beta, logw, fin, want_g=True):
    from vistaocr_amd import _lib
    ops = _ops()
    p = ops._p
    T, B, V = xd.shape
    nbytes = _lib.load().vocr_ctc_grammar_beam_workspace_bytes(T, B, V, K, nbest)
    ws = torch.full((nbytes // 4,), NAN, dtype=F32, device="cuda")
    lab, ln = torch.full((B, nbest, T), -7, dtype=I32, device="cuda"), torch.full((B, nbest), -7, dtype=I32, device="cuda")
    sc = torch.full((B, nbest, 3), NAN, dtype=F32, device="cuda")
    og = torch.full((B, nbest), NAN, dtype=F32, device="cuda") if want_g else None
    G = dp["state_off"].numel() - 1
    _lib.call("vocr_ctc_grammar_beam_search_weighted", p(xd), p(ld), T, B, V, p(cd), K, nbest, p(dp["state_off"]), p(dp["next"]),
              p(dp["dist"]), p(logw), p(fin), G, p(which), *ops._char_lm_args("test", lm, V), float(alpha), float(gw), float(beta),
              float("-inf"), p(lab), p(ln), p(sc), p(og), p(ws), nbytes, ops._stream())
    return lab, ln, sc, og


def _same(a, b):
    from tests.ctc_guarded import same_bits
    return same_bits(a, b)


# ===================================================================================================== 1. NULL weights
def test_null_weights_are_the_unweighted_entries_bit_for_bit():
    """Each weighted entry with both tables NULL returns the bits of its unweighted entry; zero-filled tables the same labels and
    scores within the sweep bound."""
    ops = _ops()
    c = wc.sweep_case("slack")
    xd, ld, cd = _dev(c.x, c.lens, c.canon)
    gp = _pack(c.automata, c.max_states, c.max_arcs, weights=False)
    want = ops.ctc_grammar_scores(xd, ld.tolist(), gp, cd, True)
    got = _raw_scores(xd, ld, gp, cd, None, None)
    assert all(_same(g, w) for g, w in zip(got, want))
    E, S = gp["src"].numel(), gp["accept"].numel()
    zero = _raw_scores(xd, ld, gp, cd, torch.zeros(E, device="cuda"), torch.zeros(S, device="cuda"))
    assert _same(zero[2], want[2]) and _same(zero[3], want[3])
    T, B, _ = c.x.shape
    for z, w in ((zero[0], want[0]), (zero[1], want[1])):
        z, w = z.cpu().double().numpy(), w.cpu().double().numpy()
        fin = w != NEG
        assert np.array_equal(z == NEG, ~fin)
        D = np.array([gr.max_in_degree(a) for a in c.automata])[None, :]
        N = np.array([a["S"] + len(a["src"]) for a in c.automata])[None, :]
        assert (np.abs(z - w)[fin] <= np.broadcast_to(2 * wc.bound(T, np.where(fin, w, 0.0), D, N, 0.0), w.shape)[fin]).all()
    G = len(c.automata)
    which = torch.tensor([b % G for b in range(B)], dtype=I32).cuda()
    wt = _t(_weights(B, 1), np.float32)
    want = ops.ctc_grammar_grad(xd, ld, gp, which, cd, wt)
    got = _raw_grad(xd, ld, gp, which, cd, wt, None, None)
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    zero = _raw_grad(xd, ld, gp, which, cd, wt, torch.zeros(E, device="cuda"), torch.zeros(S, device="cuda"))
    assert _same(zero[0], _raw_scores(xd, ld, gp, cd, torch.zeros(E, device="cuda"), torch.zeros(S, device="cuda"))[0][torch.arange(B), which.long()])
    # the beam search
    bcase = gc.case("dense_K16_lm")
    xb, lb, _ = _dev(bcase.x[:, :4], bcase.lens[:4])
    from vistaocr_amd.grammar import pack_dense_grammars
    dp = pack_dense_grammars(bcase.grammars, "cuda")
    lm = bcase.lm.to("cuda")
    want = ops.ctc_grammar_beam_search(xb, bcase.lens[:4], dp, None, None, 16, 4, lm, bcase.alpha, bcase.beta)
    wh = torch.zeros(4, dtype=I32, device="cuda")
    got = _raw_beam(xb, lb, dp, wh, None, 16, 4, lm, bcase.alpha, 1.0, bcase.beta, None, None)
    assert all(_same(g, w) for g, w in zip(got[:3], want)) and not got[3].any()
    states = dp["dist"].numel()
    zero = _raw_beam(xb, lb, dp, wh, None, 16, 4, lm, bcase.alpha, 1.0, bcase.beta, torch.zeros(states, 13, device="cuda"),
                     torch.zeros(states, device="cuda"))
    assert all(_same(g, w) for g, w in zip(zero[:3], want)) and not zero[3].any()      # + 0 * x changes no bit


# ===================================================================================================== 2. tiny, against brute force
def test_tiny_automaton_against_brute_force():
    ops = _ops()
    a, x = wc.tiny_automaton(), wc.tiny_logits()
    xd, ld, cd = _dev(x, wc.TINY_LENS, wc.TINY_CANON)
    gp = _pack([a])
    logp, best, lab, ln = [o.cpu().numpy() for o in ops.ctc_grammar_scores(xd, wc.TINY_LENS, gp, cd, True)]
    cls = ar.classes_of(4, wc.TINY_CANON)
    W = wr.accumulated_weight(a, 5)
    worst = 0.0
    for b, n in enumerate(wc.TINY_LENS):
        lnz, top, _ = wr.brute_force(x[:n, b], a, wc.TINY_CANON)
        bnd = wc.bound(5, np.array([lnz, top]), gr.max_in_degree(a), a["S"] + len(a["src"]), W)
        d = np.abs(np.array([logp[b, 0], best[b, 0]], dtype=np.float64) - [lnz, top])
        worst = max(worst, float((d / bnd).max()))
        y = lab[b, 0, :ln[b, 0]].tolist()
        assert ln[b, 0] >= 0 and gr.accepts(a, y, cls) and not lab[b, 0, ln[b, 0]:].any(), (b, y)
        # the labelling is the best path's: its Viterbi score plus the best automaton path's weight is the maximum
        if n:
            vit = float(ops.ctc_align(xd[:, b:b + 1], [n], torch.from_numpy(lab[b:b + 1, 0]).cuda(), torch.from_numpy(ln[b:b + 1, 0]).cuda(),
                                      cd)[0][0, 0])
            assert abs(vit + wr.path_weights(a, y, cls)[1] - top) <= 2 * bnd[1], (b, vit, top)
    print("wgrammar-errors tiny: largest fraction of the bound %.3f" % worst)
    assert worst <= 1.0
    assert logp[1, 0] == best[1, 0] == np.float32(a["fw"][0]) and ln[1, 0] == 0       # no frame: the start state's final weight


# ===================================================================================================== 3. sweep seams, scores
@pytest.mark.parametrize("name", wc.sweep_names())
def test_sweep_scores_against_fp64(name):
    ops = _ops()
    c = wc.sweep_case(name)
    T, B, V = c.x.shape
    xd, ld, cd = _dev(c.x, c.lens, c.canon)
    gp = _pack(c.automata, c.max_states, c.max_arcs)
    assert name != "slack" or (gp["max_states"] > max(a["S"] for a in c.automata) and gp["max_arcs"] > max(len(a["src"]) for a in c.automata))
    logp, best, lab, ln = [o.cpu().numpy() for o in ops.ctc_grammar_scores(xd, c.lens, gp, cd, True)]
    ref = wr.search(c.x, c.lens, c.automata, c.canon)
    cls = ar.classes_of(V, c.canon)
    D = np.array([gr.max_in_degree(a) for a in c.automata])[None, :]
    N = np.array([a["S"] + len(a["src"]) for a in c.automata])[None, :]
    Tb = np.clip(np.asarray(c.lens), 0, T)[:, None]
    W = np.array([[wr.accumulated_weight(a, int(t)) for a in c.automata] for t in Tb[:, 0]])
    frac, worst, finite = 0.0, 0.0, 0
    for what, g, r in (("logp", logp, ref["logp"]), ("best", best, ref["best"])):
        assert not np.isnan(g).any() and not (g == np.inf).any(), (name, what)
        assert np.array_equal(g == NEG, r == NEG), (name, what)
        fin = r != NEG
        finite += int(fin.sum())
        d = np.abs(g.astype(np.float64) - np.where(fin, r, 0.0))[fin]
        bnd = np.broadcast_to(wc.bound(Tb, np.where(fin, r, 0.0), D, N, W), r.shape)[fin]
        worst, frac = max(worst, float(d.max())), max(frac, float((d / bnd).max()))
    dead = ref["best"] == NEG
    assert (ln[dead] == -1).all() and (ln[~dead] >= 0).all()
    for b, g in np.argwhere(~dead):
        assert gr.accepts(c.automata[g], lab[b, g, :ln[b, g]], cls) and not lab[b, g, ln[b, g]:].any(), (name, b, g)
    print("wgrammar-errors scores %-10s family %-8s cells %4d staging %d  finite %d  largest |fp32 - fp64| %.3g  fraction of the bound %.3f"
          % (name, c.family, int(N.max()), wc.staging(gp["max_states"], gp["max_arcs"]), finite, worst, frac))
    assert finite >= 2 and frac <= 1.0, (name, worst, frac)


# ===================================================================================================== 4. the gradient
def _grad_case(name, family, x, lens, automata, which, canon=None, max_states=None, max_arcs=None, seed=0):
    """the weighted entry against fp64, the unweighted entry on the same logits and automata against its fp64, and the cap"""
    ops = _ops()
    T, B, V = x.shape
    w = _weights(B, seed)
    xd, ld, cd = _dev(x, lens, canon)
    wd, wt = torch.tensor([int(k) for k in which], dtype=I32).cuda(), _t(w, np.float32)
    gp = _pack(automata, max_states, max_arcs)
    logp, grad = _raw_grad(xd, ld, gp, wd, cd, wt, gp["arc_logw"], gp["final_logw"])
    ref = wr.run(x, lens, automata, which, canon, w.astype(np.float64))
    serr, gerr = _grad_errors(name, xd, lens, logp, grad, ref, w)
    rows = float(grad.double().sum(dim=2).abs().max())                   # every frame row sums to 0: every weight counted exactly once
    sc = ops.ctc_grammar_scores(xd, lens, gp, cd, False)[0]
    for b, k in enumerate(which):
        if 0 <= k < len(automata):
            assert _same(logp[b], sc[b, k]), (name, b)                       # the bits of the scores entry
    gu = _pack(automata, max_states, max_arcs, weights=False)
    ulogp, ugrad = ops.ctc_grammar_grad(xd, ld, gu, wd, cd, wt)
    userr, ugerr = _grad_errors(name + "/unweighted", xd, lens, ulogp, ugrad, gg.run(x, lens, automata, which, canon, w.astype(np.float64),
                                                                                     max_states, max_arcs), w)
    bar_s, bar_g = wc.bars(wc.GRAD_RECORDED[family])
    print("wgrammar-errors grad %-12s family %-8s T %2d B %d V %3d cells <= %4d  score %.1e  grad %.1e  row sums %.1e   unweighted: score "
          "%.1e  grad %.1e" % (name, family, T, B, V, gp["max_states"] + gp["max_arcs"], serr, gerr, rows, userr, ugerr))
    assert rows <= 64 * V * wc.U * float(np.abs(w).max()), (name, rows)      # V terms of at most |w| each, rounded
    assert serr <= 10 * userr and gerr <= 10 * ugerr, (name, serr, userr, gerr, ugerr)
    assert serr <= bar_s and gerr <= bar_g, (name, serr, gerr, bar_s, bar_g)
    assert max(serr, gerr) <= wc.CEILING
    return (xd, ld, cd, gp, wd, wt), logp, grad, ref


@pytest.mark.parametrize("name", wc.sweep_names())
def test_gradient_against_fp64(name):
    c = wc.sweep_case(name)
    B, G = c.x.shape[1], len(c.automata)
    _grad_case(name, c.family, c.x, c.lens, c.automata, [b % G for b in range(B)], c.canon, c.max_states, c.max_arcs, seed=len(name))


def test_gradient_of_the_tiny_automaton():
    a, x = wc.tiny_automaton(), wc.tiny_logits()
    # (not TINY_LENS' line of one frame: without weights every labelling of one frame is accepted, P = 1 and the gradient is exactly 0)
    _grad_case("tiny", "tiny", x, [5, 0, 2, 4], [a], [0, 0, 0, 0], wc.TINY_CANON, seed=3)


def test_a_weighted_chain_shifts_the_score_and_keeps_the_gradient():
    """A chain has one automaton path: ln Z = ln P + the sum of its weights, and the gradient is the unweighted chain's."""
    ops = _ops()
    rng = np.random.default_rng(41)
    T, B, V = 12, 4, 9
    labs = [[1, 2, 2, 3], [5], [], [8, 7, 8]]
    x = wc.bd.dense_logits(rng, T, B, V, sigma=2.0)
    lens = [12, 12, 7, 5]
    chains = [wc.random_weights(rng, gr.make(len(l) + 1, [(i, c, i + 1) for i, c in enumerate(l)], [len(l)])) for l in labs]
    xd, ld, _ = _dev(x, lens)
    wd, wt = torch.arange(B, dtype=I32).cuda(), _t(_weights(B, 5), np.float32)
    gp, gu = _pack(chains), _pack(chains, weights=False)
    logp, grad = ops.ctc_grammar_grad(xd, ld, gp, wd, None, wt)
    ulogp, ugrad = ops.ctc_grammar_grad(xd, ld, gu, wd, None, wt)
    shift = np.array([a["w"].sum() + a["fw"][-1] for a in chains])
    tol_s, tol_g = wc.bars(wc.GRAD_RECORDED["tiny"])
    from tests.test_grammar_grad_gpu import TOL
    d = np.abs(logp.cpu().double().numpy() - (ulogp.cpu().double().numpy() + shift))
    scale = np.maximum(np.abs(ulogp.cpu().double().numpy() + shift), 1.0)
    print("wgrammar-errors chain: score %.1e  grad %.1e" % (float((d / scale).max()), float((grad - ugrad).abs().max())))
    assert (d / scale <= tol_s + TOL["chains_dense"][0]).all()
    for b in range(B):
        top = float(ugrad[:, b].abs().max())
        assert float((grad[:, b] - ugrad[:, b]).abs().max()) <= (tol_g + TOL["chains_dense"][1]) * top, b


def test_two_weighted_alternatives_mix_their_probabilities():
    """Weights ln p and ln (1 - p) on two alternatives: Z = p P(l1) + (1 - p) P(l2), with P from ops.ctc_align's forward scores."""
    ops = _ops()
    from vistaocr_amd.grammar import Grammar, pack_grammars
    al = gc.field_alphabet()
    p = 0.8
    g = Grammar.from_words(al, ["10", "1a"], [np.log(p), np.log(1 - p)])
    x = wc.bd.dense_logits(np.random.default_rng(43), 12, 3, 13, sigma=2.0)
    xd, ld, _ = _dev(x, [12, 8, 2])
    lnz = ops.ctc_grammar_scores(xd, [12, 8, 2], pack_grammars([g], "cuda"), None, False)[0][:, 0].cpu().double().numpy()
    i = lambda ch: al.char_to_idx["u%04x" % ord(ch)]
    lab = torch.tensor([[[i("1"), i("0")], [i("1"), i("a")]]] * 3, dtype=I32).cuda()
    P = ops.ctc_align(xd, [12, 8, 2], lab, torch.full((3, 2), 2, dtype=I32).cuda())[0][..., 1].cpu().double().numpy()
    want = np.logaddexp(np.log(p) + P[:, 0], np.log(1 - p) + P[:, 1])
    print("wgrammar-errors alternatives: %s" % np.abs(lnz - want))
    assert (np.abs(lnz - want) <= 2 * wc.bound(12, want, 2, g.n_states + g.n_arcs, 3.0)).all(), (lnz, want)


def test_which_and_weights_per_line_and_chunked_lattices():
    """Four automata (one unweighted in a weighted pack), which in any order, one index outside [0, G); GrammarMatcher.line_log_prob
    on weighted grammars, cut into chunks of 1, 2 and 3 lines: the bits of one call."""
    import vistaocr_amd as va
    from vistaocr_amd.grammar import Grammar, GrammarMatcher
    al = gc.field_alphabet()
    grammars = [wc.field_words()[0], Grammar.from_regex(al, r"\d+-?\d*"), wc.field_ngram(),
                Grammar.from_dfa(al, [{"1": 0, "a": 1}, {"-": 0}], [True, False], arc_weights=[{"1": 0.5, "a": -1.0}, {"-": 0.25}],
                                 final_weights=[-0.5, 0.0])]
    automata = [wr.from_grammar(g) for g in grammars]
    which = [2, 0, 3, 1]
    x = wc.bd.dense_logits(np.random.default_rng(45), 12, 4, 13, sigma=2.0)
    lens = [12, 9, 12, 6]
    _grad_case("which", "slack", x, lens, automata, which, seed=7)
    _grad_case("which_out", "slack", x, lens, automata, [2, 9, -1, 1], seed=8)
    m = GrammarMatcher(al)
    xd = _t(x, np.float32).requires_grad_(True)
    up = _t(_weights(4, 9), np.float32)
    outs = []
    one = _ops().grammar_lattice_bytes(12, 1, max(g.n_states for g in grammars), max(g.n_arcs for g in grammars))
    for per in (None, 1, 2, 3):
        xd.grad = None
        lp = m.line_log_prob(xd, lens, grammars, which, max_lattice_bytes=None if per is None else per * one)
        (lp * up).sum().backward()
        outs.append((lp.detach().clone(), xd.grad.clone()))
    assert all(_same(o[0], outs[0][0]) and _same(o[1], outs[0][1]) for o in outs[1:])
    ref = wr.run(x, lens, automata, which, None, up.cpu().double().numpy())
    serr, gerr = _grad_errors("line_log_prob", xd.detach(), lens, outs[0][0], outs[0][1], ref, up.cpu().numpy())
    bar_s, bar_g = wc.bars(wc.GRAD_RECORDED["slack"])
    assert serr <= bar_s and gerr <= bar_g, (serr, gerr)
    hits = m.match(xd.detach(), lens, grammars)
    assert np.allclose(hits.logp[np.arange(4), which], outs[0][0].cpu().numpy(), rtol=0, atol=0)


# ===================================================================================================== 5. the beam search
def _beam(c, gw=None):
    from vistaocr_amd.grammar import pack_dense_grammars
    xd, ld, cd = _dev(c.x, c.lens, c.canon)
    dp = pack_dense_grammars(c.grammars, "cuda")
    out = _ops().ctc_grammar_beam_search(xd, c.lens, dp, c.which, cd, c.K, c.nbest, c.lm.to("cuda") if c.lm is not None else None, c.alpha,
                                         c.beta, None, c.gw if gw is None else gw, True)
    return [o.cpu().numpy() for o in out], (xd, ld, cd, dp)


def _unweighted_beam_error(c):
    """the existing entry on the same logits and automata (their weights dropped) against tests/grammar_beam_ref.py: the largest
    |total - fp64| and |acoustic - fp64| over the decided lines"""
    from vistaocr_amd.grammar import pack_dense_grammars
    xd, ld, cd = _dev(c.x, c.lens, c.canon)
    dp = {k: v for k, v in pack_dense_grammars(c.grammars, "cuda").items() if k not in ("logw", "final")}
    lab, ln, sc = [o.cpu().numpy() for o in _ops().ctc_grammar_beam_search(xd, c.lens, dp, c.which, cd, c.K, c.nbest,
                                                                          c.lm.to("cuda") if c.lm is not None else None, c.alpha, c.beta)]
    err = np.zeros(2)
    for b in range(c.x.shape[1]):
        g = c.grammars[0 if c.which is None else c.which[b]]
        hyps, gap = gbr.beam_search(c.x[:, b], c.lens[b], g.dense_tables(), c.K, nbest=c.nbest, canon=c.canon, lm=c.lm, alpha=c.alpha,
                                    beta=c.beta)
        if gap < wc.TAU:
            continue
        for q, h in enumerate(hyps):
            if lab[b, q, :ln[b, q]].tolist() == h[0]:
                err = np.maximum(err, np.abs(sc[b, q, :2].astype(np.float64) - np.asarray(h[1:3])))
    return err


@pytest.mark.parametrize("name", ["brute", "dense", "dense_lm", "trie"])
def test_beam_against_fp64(name):
    """brute: the beam holds every prefix, so the restatement is the brute force (tests/test_wgrammar_cpu.py).  dense: a weighted
    lexicon, a boost and an unweighted grammar through which, ragged lens, without and with the trigram.  trie: 3000 weighted words,
    beyond the sweep kernels' 8192 cells, with the 5-gram."""
    c = wc.beam_case(name)
    uerr = _unweighted_beam_error(c)
    print("wgrammar-beam-errors %-12s the unweighted entry on the same logits and automata: total %.2e acoustic %.2e" % (name, *uerr))
    (lab, ln, sc, og), _ = _beam(c)
    err = wc.beam_compare(name, c, wc.beam_reference(name), lab, ln, sc, og)
    assert (err[:2] <= 10 * uerr).all(), (name, err, uerr)


@pytest.mark.parametrize("K", [4, 16, 128])
def test_ngram_as_a_grammar_is_the_lm_search(K):
    """Grammar.from_ngram(lm) under the weighted grammar search with NO LM and grammar_weight = alpha against vocr_ctc_beam_search with
    that LM and lm_weight = alpha: identical labels and lengths on the decided lines, totals within the bar."""
    name = "ngram_K%d" % K
    c = wc.beam_case(name)
    ref = wc.beam_reference(name)
    (lab, ln, sc, og), (xd, ld, cd, dp) = _beam(c)
    lm = gc.field_lm()
    wl, wn, ws = [o.cpu().numpy() for o in _ops().ctc_beam_search(xd, c.lens, None, K, c.nbest, lm.to("cuda"), c.gw, c.beta)]
    lines = wc.decided(ref)
    assert len(lines) == 8
    assert np.array_equal(lab[lines], wl[lines]) and np.array_equal(ln[lines], wn[lines]), name
    bar = wc.bars(wc.BEAM_RECORDED["ngram"])
    d_tot = float(np.abs(sc[lines, :, 0].astype(np.float64) - ws[lines, :, 0]).max())
    d_lm = float(np.abs(og[lines].astype(np.float64) - ws[lines, :, 2]).max())          # the grammar's weight IS the LM score
    lm_err = np.zeros(2)
    for b in lines:
        for q, h in enumerate(ref[b].hyps):
            lm_err = np.maximum(lm_err, np.abs(ws[b, q, :2].astype(np.float64) - np.asarray(h[1:3])))
    print("wgrammar-beam-errors %-12s against vocr_ctc_beam_search with the LM: total %.2e  grammar - lm %.2e;  that entry against fp64: "
          "total %.2e acoustic %.2e" % (name, d_tot, d_lm, *lm_err))
    err = wc.beam_compare(name, c, ref, lab, ln, sc, og)
    assert d_tot <= 2 * bar[0] and d_lm <= 2 * bar[3], (name, d_tot, d_lm, bar)
    assert (err[:2] <= 10 * lm_err).all(), (name, err, lm_err)


@pytest.mark.parametrize("name", ["boost", "boost_lm"])
def test_a_boost_changes_the_reading(name):
    """The constructed line reads `qzx`; the boost of `qvx` makes that the 1-best - without and with the 6-gram."""
    c = wc.beam_case(name)
    al, _ = bc.english()
    want = [al.char_to_idx["u%04x" % ord(ch)] for ch in wc.BOOST_PHRASE]
    (lab, ln, sc, og), _ = _beam(c, gw=0.0)
    assert lab[0, 0, :ln[0, 0]].tolist() != want and og[0, 0] == 0.0
    (lab, ln, sc, og), _ = _beam(c)
    assert lab[0, 0, :ln[0, 0]].tolist() == want and og[0, 0] == 3.0
    wc.beam_compare(name, c, wc.beam_reference(name), lab, ln, sc, og)


def test_which_out_of_range_and_a_poisoned_table_give_no_hypothesis():
    from vistaocr_amd.grammar import pack_dense_grammars
    c = wc.beam_case("dense")
    xd, ld, _ = _dev(c.x[:, :4], c.lens[:4])
    dp = pack_dense_grammars(c.grammars, "cuda")
    which = torch.tensor([0, 3, -1, 1], dtype=I32).cuda()
    lab, ln, sc, og = _raw_beam(xd, ld, dp, which, None, 16, 4, None, 0.0, 0.7, 0.3, dp["logw"], dp["final"])
    for b in (1, 2):
        assert not np.isfinite(sc[b, :, 0].cpu().numpy()).any() and not ln[b].any() and not lab[b].any() and not og[b].any()
    assert np.isfinite(float(sc[0, 0, 0])) and np.isfinite(float(sc[3, 0, 0]))
    bad = dict(dp)
    bad["next"] = torch.full_like(dp["next"], 1 << 30)
    lab, ln, sc, og = _raw_beam(xd, ld, bad, which, None, 16, 4, None, 0.0, 0.7, 0.3, dp["logw"], dp["final"])
    assert not torch.isnan(sc).any() and not torch.isnan(og).any() and int(ln.min()) >= 0
    nanw = torch.full_like(dp["logw"], NAN)                                     # a weight that is not finite is no arc
    lab, ln, sc, og = _raw_beam(xd, ld, dp, which, None, 16, 4, None, 0.0, 0.7, 0.3, nanw, dp["final"])
    assert not torch.isnan(sc).any() and not torch.isnan(og).any() and not ln.any()


def test_an_automaton_with_a_bad_weight_poisons_its_own_column():
    ops = _ops()
    c = wc.sweep_case("slack")
    xd, ld, cd = _dev(c.x, c.lens, c.canon)
    gp = _pack(c.automata, c.max_states, c.max_arcs)
    good = ops.ctc_grammar_scores(xd, c.lens, gp, cd, True)
    a_off = np.cumsum([0] + [len(a["src"]) for a in c.automata])
    s_off = np.cumsum([0] + [a["S"] for a in c.automata])
    for bad, where in ((NAN, "arc"), (float("inf"), "arc"), (float("-inf"), "final")):
        gb = dict(gp)
        if where == "arc":
            gb["arc_logw"] = gp["arc_logw"].clone()
            gb["arc_logw"][int(a_off[1])] = bad
        else:
            acc = int(np.nonzero(c.automata[1]["accept"])[0][0])
            gb["final_logw"] = gp["final_logw"].clone()
            gb["final_logw"][int(s_off[1]) + acc] = bad
        got = ops.ctc_grammar_scores(xd, c.lens, gb, cd, True)
        assert (got[0][:, 1] == NEG).all() and (got[1][:, 1] == NEG).all() and (got[3][:, 1] == -1).all() and not got[2][:, 1].any()
        for k in (0, 2):
            assert all(_same(g[:, k], w[:, k]) for g, w in zip(got, good))
        B = c.x.shape[1]
        lp, dl = ops.ctc_grammar_grad(xd, ld, gb, torch.ones(B, dtype=I32).cuda(), cd, torch.ones(B, device="cuda"))
        assert (lp == NEG).all() and not dl.any()
    gb = dict(gp)                                                              # a final weight on a state that does not accept is not read
    dead = [s for s in range(c.automata[1]["S"]) if not c.automata[1]["accept"][s]]
    if dead:
        gb["final_logw"] = gp["final_logw"].clone()
        gb["final_logw"][int(s_off[1]) + dead[0]] = NAN
        assert all(_same(g, w) for g, w in zip(ops.ctc_grammar_scores(xd, c.lens, gb, cd, True), good))


# ===================================================================================================== 6. the surface
def test_grammar_ctc_loss_with_weighted_templates():
    """to_grammar returns a weighted automaton - at every position the transcript's symbol (ln 0.8) or its neighbour (ln 0.2): the loss
    is -sum ln Z of the restatement and its backward the restatement's gradient."""
    import vistaocr_amd as va
    from vistaocr_amd.grammar import Grammar
    al = gc.field_alphabet()

    def to_grammar(labels):
        trans = [{v: k + 1, v % 12 + 1: k + 1} for k, v in enumerate(labels)] + [{}]
        tw = [{v: float(np.log(0.8)), v % 12 + 1: float(np.log(0.2))} for v in labels] + [{}]
        return Grammar.from_dfa(al, trans, [False] * len(labels) + [True], arc_weights=tw, final_weights=[0.0] * (len(labels) + 1))

    labs = [[1, 2, 11, 3], [5, 5], [12], [7, 8, 9]]
    x = wc.bd.dense_logits(np.random.default_rng(61), 12, 4, 13, sigma=2.0)
    lens = [12, 10, 3, 12]
    crit = va.GrammarCTCLoss(al, to_grammar)
    xd = _t(x, np.float32).requires_grad_(True)
    loss = crit(xd, torch.tensor([v for l in labs for v in l]), torch.tensor(lens), torch.tensor([len(l) for l in labs]))
    (2.0 * loss).sum().backward()
    automata = [wr.from_grammar(to_grammar(tuple(l))) for l in labs]
    ref = wr.run(x, lens, automata, range(4), None, -2.0 * np.ones(4))
    serr, gerr = _grad_errors("criterion", xd.detach(), lens, crit.last_logp, xd.grad, ref, -2.0 * np.ones(4))
    bar_s, bar_g = wc.bars(wc.GRAD_RECORDED["surface"])
    print("wgrammar-errors grad %-12s family %-8s score %.1e  grad %.1e   loss %.6f  -sum ln Z %.6f" % ("criterion", "surface", serr, gerr,
                                                                                                      float(loss.detach()), -ref["logp"].sum()))
    assert serr <= bar_s and gerr <= bar_g, (serr, gerr)
    assert abs(float(loss.detach()) + ref["logp"].sum()) <= bar_s * float(np.maximum(np.abs(ref["logp"]), 1.0).sum()) + 4 * wc.U * abs(ref["logp"].sum())


def test_grammar_beam_decoder_with_a_grammar_weight():
    import vistaocr_amd as va
    c = wc.beam_case("dense")
    ref = wc.beam_reference("dense")
    al = gc.field_alphabet()
    dec = va.GrammarBeamDecoder(al, c.grammars, beam=c.K, nbest=c.nbest, insertion_bonus=c.beta, grammar_weight=c.gw)
    xd = _t(c.x, np.float32)
    lines = wc.decided(ref)
    idx = al.idx_to_char
    from vistaocr_amd.textutils import uxxxx_to_utf8
    text = lambda y: uxxxx_to_utf8(" ".join(idx[v] for v in y)) if y else ""
    got = dec.decode(xd, c.lens, which=c.which)
    plain = dec.decode_nbest(xd, c.lens, which=c.which)
    full = dec.decode_nbest(xd, c.lens, which=c.which, grammar_scores=True)
    hyps, ali = dec.decode_aligned(xd, c.lens, which=c.which)
    bar = wc.bars(wc.BEAM_RECORDED["dense"])
    for b in lines:
        want = ref[b].hyps
        assert got[b] == hyps[b] == (text(want[0][0]) if want else ""), (b, got[b], want[:1])
        assert [h[0] for h in plain[b]] == [h[0] for h in full[b]] == [h[0] for h in want], b
        assert all(len(h[1]) == 3 for h in plain[b]) and all(len(h[1]) == 4 for h in full[b])
        for h, w in zip(full[b], want):
            assert abs(h[1][0] - w[1]) <= bar[0] and abs(h[1][3] - w[4]) <= bar[3], (b, h, w)
            assert h[1][3] == np.float32(c.grammars[c.which[b]].weight_of(h[0])) or abs(h[1][3] - c.grammars[c.which[b]].weight_of(h[0])) < 1e-5
        assert (ali[b] is None) == (not want)
    off = va.GrammarBeamDecoder(al, c.grammars, beam=c.K, nbest=c.nbest, insertion_bonus=c.beta, grammar_weight=0.0)
    zero = wc.beam_references(c, gw=0.0)
    res = off.decode_nbest(xd, c.lens, which=c.which)
    for b in wc.decided(zero):
        assert [h[0] for h in res[b]] == [h[0] for h in zero[b].hyps], b
    with pytest.raises(ValueError):
        va.GrammarBeamDecoder(al, c.grammars, grammar_weight=float("nan"))
