"""GPU: vocr_ctc_entropy (vistaocr_amd/csrc/ctc_entropy.hip), EntropyRegularizedCTCLoss and CtcAligner.entropy against the fp64
restatement of tests/entropy_ref.py.  Every element of every output is compared: -inf exactly where the restatement has it and never a
NaN, rows past `lens` and the rows of a line without a score exactly 0, the rest within the family's tolerance.

THE TOLERANCES are not derived: they are 4x the largest error each case family showed on an MI355X, rounded up to one digit
(profiles/ctc_entropy_errors.txt lists the measured maxima; results are bit-identical from run to run, so the margin is for other
inputs of the same family, not for noise).  Scores: max(|ln P - ref|, |H - ref|) / max(|ln P| + H, 1).  Gradient: per line,
max |g - ref| / (the line's largest |ref|), for coefficients (w_ctc, w_ent) of both signs drawn per line.  Every case prints its figures
before it asserts ("entropy-errors ...").

What the shapes are for (the constants are the kernels'): the paired sweep keeps labellings of up to 31 labels in registers and
prefetches PF = 8 frames there, beyond that it keeps both rows in LDS in 64-position chunks and stages TB = 8 frames (L = 31, 32, 33:
S = 63, 65, 67 across the one-wave limit; L = 63, 64, 65: S = 127, 129, 131 across a chunk seam; lens 1, 2, 8, 9, 10, 17 and 65, 66,
73, 74 at the two depths); the gradient kernel works on tiles of TT = 16 frames with the positions in SG = 4 groups."""
import math

import numpy as np
import pytest
import torch

from tests import ctc_ref as cr
from tests import entropy_ref as er
from tests import nbest_ref as nr
from tests.beam_data import dense_logits

pytestmark = pytest.mark.gpu
NAN = float("nan")
NEG = float("-inf")
PEAKY, DENSE = ("peaky", 8.0, 1.0), ("beam_dense", 3.0)
CANON9 = [0, 1, 1, 3, 4, 4, 4, 7, 8]          # classes of 2 ({1, 2}) and 3 ({4, 5, 6}) members; V >= 9

# family: (scores, gradient) = 4x the maxima of profiles/ctc_entropy_errors.txt, rounded up to one digit
TOL = {
    "seam_peaky": (7e-6, 3e-4),               # profiles/ctc_entropy_errors.txt: 1.7e-06, 5.4e-05
    "seam_dense": (2e-6, 4e-3),               # profiles/ctc_entropy_errors.txt: 4.5e-07, 8.1e-04
    "lens": (1e-5, 3e-4),                     # profiles/ctc_entropy_errors.txt: 2.5e-06, 5.6e-05
    "stage": (4e-7, 6e-4),                    # profiles/ctc_entropy_errors.txt: 8.8e-08, 1.5e-04
    "tight": (6e-6, 3e-4),                    # profiles/ctc_entropy_errors.txt: 1.5e-06, 6.1e-05 (dH alone)
    "V": (5e-6, 2e-4),                        # profiles/ctc_entropy_errors.txt: 1.1e-06, 4.1e-05
    "ragged": (1e-5, 9e-5),                   # profiles/ctc_entropy_errors.txt: 2.4e-06, 2.1e-05
    "classes": (3e-6, 2e-4),                  # profiles/ctc_entropy_errors.txt: 6.8e-07, 4.2e-05
    "certain": (4e-7, 4e-5),                  # profiles/ctc_entropy_errors.txt: 8.2e-08, 9.2e-06
    "long": (4e-6, 7e-3),                     # profiles/ctc_entropy_errors.txt: 8.3e-07, 1.6e-03
    "uniform": (3e-6, 0.0),                   # profiles/ctc_entropy_errors.txt: 6.6e-07 (scores only)
    "criterion": (4e-6, 2e-4),                # profiles/ctc_entropy_errors.txt: 8.1e-07, 3.8e-05
}

_L_LONG = [100, 97, 104, 90, 110, 99, 101, 95] * 4
# name, family, T, B, V, label counts, kinds, lens ("full", "tight" or a list), regime, canon, specials
CASES = [
    ("seam_peaky", "seam_peaky", 140, 8, 40, [0, 1, 31, 32, 33, 63, 64, 65], "random", [140, 139, 140, 138, 140, 137, 140, 140], PEAKY, None, ()),
    ("seam_dense", "seam_dense", 140, 8, 40, [0, 1, 31, 32, 33, 63, 64, 65], "random", [140, 139, 140, 138, 140, 137, 140, 140], DENSE, None, ()),
    ("seam_patterns", "seam_peaky", 140, 6, 30, [31, 32, 33, 63, 64, 65], ["equal", "abab", "equal", "abab", "abab", "equal"], "full", PEAKY, None, ()),
    ("lens_peaky", "lens", 17, 7, 12, [1, 1, 3, 4, 4, 6, 5], "random", [1, 2, 8, 9, 10, 17, 16], PEAKY, None, ()),
    ("lens_dense", "lens", 17, 7, 12, [1, 2, 3, 4, 4, 6, 5], "random", [1, 2, 8, 9, 10, 17, 16], DENSE, None, ()),
    ("stage", "stage", 74, 4, 20, [33, 33, 34, 40], "random", [65, 66, 73, 74], DENSE, None, ()),
    ("tight", "tight", 130, 5, 20, [5, 31, 33, 12, 64], "random", "tight", DENSE, None, ()),
    ("tight_equal", "tight", 130, 3, 20, [5, 33, 65], "equal", "tight", PEAKY, None, ()),
    ("V2", "V", 24, 3, 2, [5, 1, 0], "equal", [24, 17, 9], DENSE, None, ()),
    ("V96", "V", 40, 3, 96, [10, 7, 0], "random", [40, 33, 8], PEAKY, None, ()),
    ("V256", "V", 20, 2, 256, [6, 4], "random", [20, 13], DENSE, None, ()),
    ("ragged", "ragged", 40, 7, 15, [6, 5, 3, 30, 4, 2, 3], ["random", "random", "random", "equal", "random", "random", "random"],
     [40, 25, 0, 33, 12, 5, 30], PEAKY, None, ("bad",)),
    ("classes_peaky", "classes", 40, 3, 12, [8, 6, 3], "random", [40, 31, 17], PEAKY, "c9", ("member", "neginf")),
    ("classes_dense", "classes", 40, 3, 12, [8, 6, 33], "random", [40, 31, 40], DENSE, "c9", ("member", "neginf")),
    ("certain", "certain", 12, 3, 6, [3, 3, 2], ["abab", "abab", "equal"], [12, 12, 9], DENSE, None, ("certain",)),
    ("long", "long", 294, 32, 96, _L_LONG, "random", [294 - 2 * i for i in range(32)], "both", None, ()),
]


def build_case(name):
    """dict(x fp32 [T,B,V], lens, labs[b] (list), canon (list or None), coeff float64 [B,2] (fp32 values), M): data only"""
    spec = [c for c in CASES if c[0] == name][0]
    _, family, T, B, V, ls, kinds, lens, regime, canon, specials = spec
    rng = np.random.default_rng([16, [c[0] for c in CASES].index(name)])
    kinds = [kinds] * B if isinstance(kinds, str) else kinds
    canon = CANON9 + list(range(9, V)) if canon == "c9" else None
    cls = er.classes_of(V, canon)
    labs = [cr.make_labels(rng, V, ls[b], kinds[b]) for b in range(B)]
    if "member" in specials:                                  # a label given as the non-canonical member of its class
        labs[0][0], labs[1][-1] = 2, 6
    if lens == "full":
        lens = [T] * B
    elif lens == "tight":                                     # exactly one feasible path
        lens = [er.need(l, cls) for l in labs]
    lens = [int(v) for v in lens]
    assert max(lens) <= T
    fit = [l if er.need(l, cls) <= lens[b] else [] for b, l in enumerate(labs)]
    if regime == "both":                                      # even lines peaky, odd lines dense
        x = cr.build_logits(rng, T, B, V, fit, lens, PEAKY)
        x[:, 1::2] = torch.from_numpy(dense_logits(rng, T, B, V, 3.0))[:, 1::2]
    elif regime[0] == "beam_dense":
        x = torch.from_numpy(dense_logits(rng, T, B, V, regime[1]))
    else:
        x = cr.build_logits(rng, T, B, V, fit, lens, regime)
    if "bad" in specials:                                     # line 4: a label outside (0, V)
        labs[4] = [V] + labs[4][1:]
    if "neginf" in specials:                                  # one member of the 3-class at -inf everywhere, one of the 2-class on a line,
        x[:, :, 5] = NEG                                      # a whole other class on line 1
        x[:, 0, 2] = NEG
        x[:, 1, 9] = NEG
        labs[1] = [v if v != 9 else 10 for v in labs[1]]
    if "certain" in specials:
        a, b2 = labs[0][0], labs[0][1]                        # line 0: frames whose only finite column is the path's: u = 0 exactly
        for t, col in ((0, a), (5, 0), (11, a if len(labs[0]) % 2 else b2)):
            keep = x[t, 0, col].clone()
            x[t, 0, :] = NEG
            x[t, 0, col] = keep
        path = [labs[1][0]] * 4 + [labs[1][1]] * 3 + [0] * 2 + [labs[1][2]] * 3        # line 1: every frame certain, P = 1 and H = 0
        for t, col in enumerate(path):
            x[t, 1, :] = NEG
            x[t, 1, col] = 1.5
    co = rng.normal(0, 1, (B, 2))
    co = (np.sign(co) * (0.5 + np.abs(co))).astype(np.float32).astype(np.float64)
    return dict(name=name, family=family, x=x, lens=lens, labs=labs, canon=canon, coeff=co, M=max(max(len(l) for l in labs), 1),
                T=T, B=B, V=V, cls=cls)


_refs = {}


def _reference(name):
    """the case and its fp64 answer (ln P [B], H [B], grad [T,B,V] at the case's coefficients), computed once"""
    if name not in _refs:
        k = build_case(name)
        _refs[name] = (k, er.entropy(k["x"].numpy(), k["lens"], k["labs"], k["canon"], k["coeff"], k["M"]))
    return _refs[name]


def _pack(labs, width, dev="cuda"):
    lab = np.zeros((len(labs), max(width, 1)), dtype=np.int32)
    ln = np.zeros(len(labs), dtype=np.int32)
    for b, l in enumerate(labs):
        ln[b] = len(l)
        lab[b, :min(len(l), lab.shape[1])] = l[:lab.shape[1]]
    return torch.from_numpy(lab).to(dev), torch.from_numpy(ln).to(dev)


def _raw(x, lens, labels, label_lens, M, canon=None, coeff=None):
    """the C entry point itself, every buffer NaN-filled first; returns device tensors (ctc [B], entropy [B], dlogits [T,B,V] or None)"""
    from vistaocr_amd import _lib, ops
    T, B, V = x.shape
    nbytes = _lib.load().vocr_ctc_entropy_workspace_bytes(T, B, V, M, 0 if coeff is None else 1)
    assert nbytes > 0
    ws = torch.full(((nbytes + 3) // 4,), NAN, dtype=torch.float32, device=x.device)
    ctc = torch.full((B,), NAN, dtype=torch.float32, device=x.device)
    ent = torch.full((B,), NAN, dtype=torch.float32, device=x.device)
    dl = torch.full((T, B, V), NAN, dtype=torch.float32, device=x.device) if coeff is not None else None
    p = ops._p
    _lib.call("vocr_ctc_entropy", p(x), p(lens), T, B, V, p(canon), p(labels), p(label_lens), int(labels.shape[1]), M, p(coeff), p(ctc),
              p(ent), p(dl), p(ws), ws.numel() * 4, ops._stream())
    return ctc, ent, dl


def _device_case(k, dev="cuda"):
    labels, label_lens = _pack(k["labs"], k["M"], dev)
    canon = None if k["canon"] is None else torch.tensor(k["canon"], dtype=torch.int32, device=dev)
    return (k["x"].to(dev), torch.tensor(k["lens"], dtype=torch.int32, device=dev), labels, label_lens, canon,
            torch.from_numpy(k["coeff"].astype(np.float32)).to(dev))


def _errors(name, T, lens, ctc, ent, grad, ref):
    """the exact parts asserted; returns (score error, gradient error) in the units of TOL"""
    lnp, H, g = ref
    got_p, got_h = ctc.cpu().double().numpy(), ent.cpu().double().numpy()
    assert not np.isnan(got_p).any() and np.isfinite(got_h).all() and (got_h >= 0).all(), (name, got_p, got_h)
    fin = np.isfinite(lnp)
    assert ((got_p == NEG) == ~fin).all() and (np.isfinite(got_p) == fin).all(), (name, got_p, lnp)
    assert (got_h[~fin] == 0).all(), name
    serr = 0.0
    if fin.any():
        scale = np.maximum(np.abs(lnp[fin]) + H[fin], 1.0)
        serr = float((np.maximum(np.abs(got_p[fin] - lnp[fin]), np.abs(got_h[fin] - H[fin])) / scale).max())
    gerr = 0.0
    if grad is not None:
        got_g = grad.cpu().double().numpy()
        assert np.isfinite(got_g).all(), name
        for b, ln in enumerate(lens):
            ln = min(max(ln, 0), T)
            assert float(np.abs(got_g[ln:, b]).max() if ln < T else 0.0) == 0.0, (name, b)
            top = float(np.abs(g[:, b]).max())
            if not fin[b] or top == 0.0:
                assert float(np.abs(got_g[:, b]).max()) == 0.0, (name, b)
            else:
                gerr = max(gerr, float(np.abs(got_g[:, b] - g[:, b]).max()) / top)
    return serr, gerr


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_scores_and_gradient_against_fp64(name):
    from vistaocr_amd import ops
    k, ref = _reference(name)
    x, lens, labels, label_lens, canon, coeff = _device_case(k)
    ctc, ent, grad = _raw(x, lens, labels, label_lens, k["M"], canon, coeff)
    serr, gerr = _errors(name, k["T"], k["lens"], ctc, ent, grad, ref)
    fin = np.isfinite(ref[0])
    extra = 0.0
    if k["family"] == "tight":
        # one feasible path: H = 0 and dH = 0.  The entropy's gradient alone, coefficients (0, 1), against the scale of ln P's
        assert all(er.count_paths(n, l, k["cls"]) == 1 for n, l in zip(k["lens"], k["labs"]))
        zero_one = torch.tensor([[0.0, 1.0]] * k["B"], device="cuda")
        _, _, gh = _raw(x, lens, labels, label_lens, k["M"], canon, zero_one)
        _, _, gp = er.entropy(k["x"].numpy(), k["lens"], k["labs"], k["canon"], [[1.0, 0.0]] * k["B"], k["M"])
        for b in range(k["B"]):
            extra = max(extra, float(gh[:, b].abs().max()) / float(np.abs(gp[:, b]).max()))
        assert float(np.abs(ref[1]).max()) < 1e-9                      # the restatement's own rounding at |ln P| of some hundreds
    print("entropy-errors %-14s family %-10s T %3d B %2d V %3d longest %3d  scorable %2d / %2d  max |lnP| %8.3f max H %7.3f  score %.1e  "
          "grad %.1e  dH alone %.1e" % (name, k["family"], k["T"], k["B"], k["V"], k["M"], int(fin.sum()), fin.size,
                                        float(np.abs(ref[0][fin]).max()) if fin.any() else 0.0, float(ref[1].max()), serr, gerr, extra))
    tol_s, tol_g = TOL[k["family"]]
    assert serr <= tol_s and gerr <= tol_g and extra <= tol_g, (name, serr, gerr, extra)
    # bit-identical: a second run, the scores-only call, the Python entry (its own uninitialised buffers)
    ctc2, ent2, grad2 = _raw(x, lens, labels, label_lens, k["M"], canon, coeff)
    assert torch.equal(ctc, ctc2) and torch.equal(ent, ent2) and torch.equal(grad, grad2), name
    c3, e3, none = _raw(x, lens, labels, label_lens, k["M"], canon, None)
    assert none is None and torch.equal(c3, ctc) and torch.equal(e3, ent), name
    c4, e4, g4 = ops.ctc_entropy(x, k["lens"], labels, label_lens, canon, coeff)
    assert torch.equal(c4, ctc) and torch.equal(e4, ent) and torch.equal(g4, grad), name
    # the same bits as the n-best entry's score, with and without weights
    assert torch.equal(ops.ctc_nbest(x, lens, labels, label_lens, canon)[0], ctc), name
    assert torch.equal(ops.ctc_nbest(x, lens, labels, label_lens, canon, torch.ones(k["B"], device="cuda"))[0], ctc), name


def test_case_list_covers_what_it_claims():
    longest = {c[0]: c[5] for c in CASES}
    assert set(longest["seam_peaky"]) == {0, 1, 31, 32, 33, 63, 64, 65} == set(longest["seam_dense"])
    lens = {v for c in CASES for v in build_case(c[0])["lens"]}
    assert lens >= {0, 1, 2, 8, 9, 10, 17, 65, 66, 73, 74}
    assert {c[4] for c in CASES} >= {2, 96, 256}
    k, ref = _reference("ragged")
    assert [bool(v) for v in np.isfinite(ref[0])] == [True, True, False, False, False, True, True]      # lens 0, no fit, a bad label
    k, ref = _reference("certain")
    _, clp = er.class_logprobs(k["x"][:, 1].numpy(), k["cls"])
    assert (clp.max(1)[:12] == 0.0).all() and ref[0][1] == 0.0 and ref[1][1] == 0.0
    k, ref = _reference("long")
    assert k["T"] == 294 and k["B"] == 32 and k["V"] == 96 and min(len(l) for l in k["labs"]) >= 90 and np.isfinite(ref[0]).all()
    k, ref = _reference("classes_peaky")
    assert k["labs"][0][0] == 2 and k["cls"][2] == 1 and np.isfinite(ref[0]).all()


def test_uniform_logits_closed_form():
    """every feasible path is equally likely: H = ln(count) and ln P = H - len * ln V, the count an integer recursion"""
    T, V = 70, 11
    labs = [[], [3], [1, 2, 3, 3, 1], [4] * 20, list(range(1, 11)) * 3 + [1, 2, 3], [5, 6] * 17]
    lens = [9, 70, 40, 60, 70, 69]
    x = torch.full((T, len(labs), V), 0.25)
    labels, label_lens = _pack(labs, 34)
    ctc, ent, _ = _raw(x.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda"), labels, label_lens, 34)
    worst = 0.0
    for b, (lab, n) in enumerate(zip(labs, lens)):
        h = math.log(er.count_paths(n, lab))
        p = h - n * math.log(V)
        worst = max(worst, max(abs(float(ctc[b]) - p), abs(float(ent[b]) - h)) / max(abs(p) + h, 1.0))
    print("entropy-errors uniform        family uniform    T %3d B %2d V %3d  score %.1e" % (T, len(labs), V, worst))
    assert worst <= TOL["uniform"][0]


@pytest.mark.parametrize("name", ["seam_dense", "ragged", "classes_peaky", "stage"])
def test_a_line_does_not_depend_on_its_batch(name):
    k, _ = _reference(name)
    x, lens, labels, label_lens, canon, coeff = _device_case(k)
    ctc, ent, grad = _raw(x, lens, labels, label_lens, k["M"], canon, coeff)
    for b in range(k["B"]):
        c1, e1, g1 = _raw(x[:, b:b + 1].contiguous(), lens[b:b + 1].contiguous(), labels[b:b + 1].contiguous(),
                          label_lens[b:b + 1].contiguous(), k["M"], canon, coeff[b:b + 1].contiguous())
        assert torch.equal(c1[0], ctc[b]) and torch.equal(e1[0], ent[b]) and torch.equal(g1[:, 0], grad[:, b]), (name, b)


@pytest.mark.parametrize("name", ["seam_peaky", "seam_dense", "classes_dense", "lens_dense"])
def test_gradient_is_linear_in_the_coefficients(name):
    """(1, 0) is vocr_ctc_nbest_grad's gradient at weight 1, within that suite's bar against fp64; (0, 1) sums to 0 over every frame; the
    case's own coefficients give the combination.  Every run is within tol * (its line's scale) of fp64, where the three are exactly
    linear, so the bars add; a row sum adds the bars of its nonzero columns.  The scale of a line is its largest |g|, and for the
    (0, 1) run not less than that of the (1, 0) run: on a line with one feasible path (L = 0 is one) dH is 0 and what the kernel returns
    is rounding of the size the tight family records against d ln P (profiles/ctc_entropy_errors.txt, "dH alone")."""
    k, _ = _reference(name)
    x, lens, labels, label_lens, canon, coeff = _device_case(k)
    B, T = k["B"], k["T"]
    tol = TOL[k["family"]][1]
    one = torch.tensor([[1.0, 0.0]] * B, device="cuda")
    two = torch.tensor([[0.0, 1.0]] * B, device="cuda")
    g10, g01, g = (_raw(x, lens, labels, label_lens, k["M"], canon, c)[2].cpu().double() for c in (one, two, coeff))
    own = nr.Reference(k["x"], k["lens"], [[l] for l in k["labs"]], k["canon"], np.ones((B, 1)), k["M"])
    frac = cr.ratio(g10, own.grad, own.grad_bar)
    nb = _ops().ctc_nbest(x, lens, labels, label_lens, canon, torch.ones(B, device="cuda"))[1].cpu().double()
    both = cr.ratio(nb, own.grad, own.grad_bar)
    worst_sum = worst_lin = 0.0
    for b in range(B):
        top10, top01, top = float(g10[:, b].abs().max()), float(g01[:, b].abs().max()), float(g[:, b].abs().max())
        wc, we = float(coeff[b, 0]), float(coeff[b, 1])
        scale01 = max(top01, top10)
        if top01 > 0:
            cols = int((g01[:, b] != 0).any(0).sum())
            worst_sum = max(worst_sum, float(g01[:, b].sum(1).abs().max()) / (cols * tol * scale01))
        bar = tol * (abs(wc) * top10 + abs(we) * scale01 + top)
        if bar > 0:
            worst_lin = max(worst_lin, float((g[:, b] - (wc * g10[:, b] + we * g01[:, b])).abs().max()) / bar)
        else:
            assert float(g[:, b].abs().max()) == 0.0
    print("entropy-errors %-14s (1, 0) against fp64 / nbest bar %.3f (vocr_ctc_nbest_grad itself %.3f)  (0, 1) row sums / bar %.3f  "
          "linearity / bar %.3f" % (name, frac, both, worst_sum, worst_lin))
    assert frac <= 1.0 and worst_sum <= 1.0 and worst_lin <= 1.0


def _ops():
    from vistaocr_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------- the criterion
def _criterion_case(regime, feasible_only):
    """mix64 of tests/ctc_ref.py (T 60, B 4, V 96, up to 31 labels), whose CTC errors profiles/ctc_fp64_errors.txt records; one of its
    lines has no alignment, `feasible_only` leaves it out.  (x, flat targets, act_lens, label_lens, labs, lens)"""
    x, _, _, act, labs = cr.build_case("mix64", regime)
    keep = [b for b in range(len(labs)) if not feasible_only or cr.need(labs[b]) <= act[b]]
    assert len(keep) == (3 if feasible_only else 4)
    labs, act = [labs[b] for b in keep], [int(act[b]) for b in keep]
    flat = torch.tensor([v for l in labs for v in l], dtype=torch.int32)
    return (x[:, keep].contiguous(), flat, torch.tensor(act, dtype=torch.int32), torch.tensor([len(l) for l in labs], dtype=torch.int32),
            labs, act)


# mix64 in profiles/ctc_fp64_errors.txt: max abs error of nll per line, of dlogits per element, (dense_3, peaky_8_1)
CTC_RECORDED = {cr.DENSE: (3.22e-05, 5.31e-05), cr.PEAKY8: (3.84e-06, 2.02e-06)}


def _run(crit, x, flat, act, ll, scale=1.0):
    xd = x.cuda().requires_grad_(True)
    loss = crit(xd, flat, act, ll)
    assert tuple(loss.shape) == (1,)
    (scale * loss).backward()
    return float(loss.detach()), xd.grad.cpu().double().numpy()


@pytest.mark.parametrize("regime", [cr.DENSE, cr.PEAKY8])
def test_criterion_at_beta_0_is_the_ctc_loss(regime):
    """loss and gradient against CTCLoss, another kernel, within the sum of the two kernels' recorded fp64 errors; with the line that
    cannot be aligned in the batch both give +inf (and CTCLoss gives that line its softmax rows, this criterion zeros)"""
    import vistaocr_amd as va
    x, flat, act, ll, labs, lens = _criterion_case(regime, True)
    lnp, H, g = er.entropy(x.numpy(), lens, labs, None, [[-1.0, 0.0]] * len(labs))
    assert np.isfinite(lnp).all()
    e_nll, e_grad = CTC_RECORDED[regime]
    tol_s, tol_g = TOL["criterion"]
    ctc, own = _run(va.CTCLoss(), x, flat, act, ll), _run(va.EntropyRegularizedCTCLoss(0.0), x, flat, act, ll)
    d_loss = abs(ctc[0] - own[0])
    bar_loss = float((e_nll + tol_s * np.maximum(np.abs(lnp) + H, 1.0)).sum()) + 4 * cr.U * float(np.abs(lnp).sum())
    worst = 0.0
    for b in range(len(labs)):
        worst = max(worst, float(np.abs(ctc[1][:, b] - own[1][:, b]).max()) / (e_grad + tol_g * float(np.abs(g[:, b]).max())))
    print("entropy-errors criterion beta 0 %-9s  loss %.6f / CTCLoss %.6f  diff %.2e / bar %.2e  grad diff / bar %.3f"
          % (regime[0], own[0], ctc[0], d_loss, bar_loss, worst))
    assert d_loss <= bar_loss and worst <= 1.0
    x, flat, act, ll, labs, lens = _criterion_case(regime, False)
    ctc, own = _run(va.CTCLoss(), x, flat, act, ll), _run(va.EntropyRegularizedCTCLoss(0.0), x, flat, act, ll)
    assert ctc[0] == float("inf") and own[0] == float("inf")
    assert float(np.abs(own[1][:, 0]).max()) == 0.0 and float(np.abs(own[1][:, 1:]).max()) > 0 and np.isfinite(own[1]).all()


@pytest.mark.parametrize("regime", [cr.DENSE, cr.PEAKY8])
def test_criterion_at_beta_is_nll_minus_beta_entropy(regime):
    import vistaocr_amd as va
    beta = 0.25
    x, flat, act, ll, labs, lens = _criterion_case(regime, True)
    lnp, H, g = er.entropy(x.numpy(), lens, labs, None, [[-1.0, -beta]] * len(labs))
    crit = va.EntropyRegularizedCTCLoss(beta)
    got, gg = _run(crit, x, flat, act, ll, 2.0)                     # the saved gradient is scaled in the backward
    tol_s, tol_g = TOL["criterion"]
    nll, ent = crit.last_nll.cpu().double().numpy(), crit.last_entropy.cpu().double().numpy()
    assert tuple(crit.last_nll.shape) == (len(labs),) == tuple(crit.last_entropy.shape) and crit.last_nll.is_cuda
    scale = np.maximum(np.abs(lnp) + H, 1.0)
    serr = float((np.maximum(np.abs(nll + lnp), np.abs(ent - H)) / scale).max())
    want = float((-lnp - beta * H).sum())
    gerr = max(float(np.abs(gg[:, b] - 2.0 * g[:, b]).max()) / (2.0 * float(np.abs(g[:, b]).max())) for b in range(len(labs)))
    print("entropy-errors criterion beta %.2f %-9s  score %.1e  grad %.1e  loss %.6f want %.6f" % (beta, regime[0], serr, gerr, got, want))
    assert serr <= tol_s and gerr <= tol_g
    assert abs(got - want) <= (1 + beta) * tol_s * float(scale.sum()) + 4 * cr.U * abs(want)


def _tiny_model(AL):
    import vistaocr_amd as va
    torch.manual_seed(0)
    model = va.CnnOcrModel(alphabet=AL, verbose=False, input_line_height=30, rds_line_height=30, lstm_input_dim=32, num_lstm_layers=1,
                           num_lstm_hidden_units=32, p_lstm_dropout=0.0, num_in_channels=1)
    model.train()
    return model


def _batch(AL, seed=5):
    g = torch.Generator().manual_seed(seed)
    nb, width, L = 4, 200, 5
    return (torch.rand(nb, 1, 30, width, generator=g), torch.randint(1, len(AL), (nb * L,), generator=g).to(torch.int32),
            torch.full((nb,), width, dtype=torch.int32), torch.full((nb,), L, dtype=torch.int32), {})


@pytest.mark.parametrize("step", ["train", "train_async"])
def test_training_step_with_the_criterion(step):
    import vistaocr_amd as va
    from vistaocr_amd import ops
    AL = va.english_alphabet()
    model = _tiny_model(AL)
    opt = va.make_optimizer(model, lr=1e-3)
    crit = va.EntropyRegularizedCTCLoss(0.2)
    before = torch.cat([p.detach().reshape(-1).clone() for p in model.parameters()])
    out = (va.train if step == "train" else va.train_async)(_batch(AL), model, crit, opt)
    value = out if step == "train" else float(out.reshape(-1)[0].cpu())
    assert isinstance(value, float) and np.isfinite(value)
    after = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert bool(torch.isfinite(after).all()) and float((after - before).abs().max()) > 0
    assert bool(torch.isfinite(crit.last_nll).all()) and bool((crit.last_entropy > 0).all())
    ops.check_health_sync(torch.device("cuda", torch.cuda.current_device()))


def test_fit_accepts_the_criterion(tmp_path):
    import os
    import vistaocr_amd as va
    from vistaocr_amd.loop import fit
    AL = va.english_alphabet()
    model = _tiny_model(AL)
    opt = va.make_optimizer(model, lr=1e-3)
    hist = fit(model, va.EntropyRegularizedCTCLoss(0.1), opt, [_batch(AL, 1), _batch(AL, 2)], None, va.train,
               os.path.join(str(tmp_path), "run"), batch_size=4, snapshot_every_n_iterations=1000)
    assert len(hist["loss"]) == 2 and all(np.isfinite(v) for v in hist["loss"])


def test_python_entries_shapes_and_errors():
    import vistaocr_amd as va
    from vistaocr_amd import ops
    k, ref = _reference("lens_peaky")
    x, lens, labels, label_lens, canon, coeff = _device_case(k)
    with pytest.raises(RuntimeError, match="coeff"):
        ops.ctc_entropy(x, lens, labels, label_lens, None, coeff[:, :1].contiguous())
    with pytest.raises(RuntimeError, match="coeff"):
        ops.ctc_entropy(x, lens, labels, label_lens, None, coeff.double())
    with pytest.raises(RuntimeError, match="labels must be"):
        ops.ctc_entropy(x, lens, labels.unsqueeze(1), label_lens.unsqueeze(1))
    with pytest.raises(RuntimeError, match="lengths"):
        ops.ctc_entropy(x, lens[:3], labels, label_lens)
    with pytest.raises(ValueError, match="beta"):
        va.EntropyRegularizedCTCLoss(-1.0)
    crit = va.EntropyRegularizedCTCLoss(0.1)
    flat = torch.tensor([v for l in k["labs"] for v in l], dtype=torch.int32)
    ll = torch.tensor([len(l) for l in k["labs"]], dtype=torch.int32)
    act = torch.tensor(k["lens"], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="one entry per batch element"):
        crit(x, flat, act[:3], ll)
    with pytest.raises(RuntimeError, match="sum\\(label_lens\\)"):
        crit(x, flat[:-1], act, ll)
    with pytest.raises(RuntimeError, match="exceeds the time dimension"):
        crit(x, flat, act + 1, ll)
    loss = crit(x, flat, act, ll)                                    # the flat targets are unpacked to the kernel's rows
    want = float((-ref[0] - 0.1 * ref[1]).sum())
    assert abs(float(loss) - want) <= 1e-5 * abs(want)


def test_aligner_entropy_returns_the_kernels_numbers():
    import vistaocr_amd as va
    from vistaocr_amd import ops
    AL = va.english_alphabet()
    V = len(AL)
    rng = np.random.default_rng(4)
    T, lens = 30, [30, 21, 4]
    x = torch.from_numpy(dense_logits(rng, T, 3, V, 3.0)).cuda()
    canon = torch.tensor(AL.canonical_indices(), dtype=torch.int32, device="cuda")
    cls = er.classes_of(V, AL.canonical_indices())
    labs = [[int(v) for v in rng.integers(1, V, 6) if cls[int(v)] != 0], [int(v) for v in rng.integers(1, V, 3) if cls[int(v)] != 0],
            [5, 5, 5, 5, 5]]                                         # the last one does not fit its 4 frames
    got = va.CtcAligner(AL).entropy(x, lens, labs)
    labels, label_lens = _pack(labs, 6)
    ctc, ent, _ = ops.ctc_entropy(x, lens, labels, label_lens, canon)
    assert len(got) == 3 and got[2] == (NEG, 0.0, 0.0)
    for b in range(3):
        assert got[b][0] == float(ctc[b]) and got[b][1] == float(ent[b]) and got[b][2] == float(ent[b]) / lens[b]
    strings = [" ".join(AL.idx_to_char[v] for v in l) for l in labs]
    assert va.CtcAligner(AL).entropy(x, torch.tensor(lens), strings) == got
