"""CPU: the restatement of tests/nbest_ref.py (weighted n-best CTC scores and gradient, the risk on top of it) held to brute-force path
enumeration with autograd and to tests/ctc_ref.py; the bars of tests/test_nbest_gpu.py held to the project's rule (an fp32 run of the
kernel's formulas within a quarter of every gradient bar, and inside the project's eps_line for the scores, on the whole GPU case list;
every mutant at least 10x over a bar); and the argument validation of the new entry points, which needs no GPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ctc_ref as cr
from tests import nbest_cases as nc
from tests import nbest_ref as nr


@pytest.fixture(scope="module", autouse=True)
def _cpu_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)


def _brute(x, lens, hyps, cls, w):
    """scores and the gradient of sum w_q ln P_q over the scorable hypotheses, by enumeration and autograd"""
    xx = x.clone().requires_grad_(True)
    B, n = len(hyps), len(hyps[0])
    sc = np.full((B, n), -np.inf)
    tot = torch.zeros((), dtype=torch.float64)
    for b in range(B):
        for q, h in enumerate(hyps[b]):
            if not nr.hyp_ok(h, x.shape[2], cls, x.shape[0]):
                continue
            s = nr.brute_force(xx[:, b], lens[b], h, cls)
            if s is not None and bool(torch.isfinite(s)):
                sc[b, q] = float(s.detach())
                tot = tot + w[b, q] * s
    tot.backward()
    return sc, xx.grad


@pytest.mark.parametrize("canon", [None, [0, 1, 1, 3, 3], [0, 1, 2, 2, 2]])
def test_restatement_equals_brute_force(canon):
    """all V^T paths, T <= 6, V = 5, classes of 2 and 3 members, weights of both signs, a -inf column, ragged lines, hypotheses that do
    not fit or are bad"""
    rng = np.random.default_rng(5)
    T, B, V = 6, 3, 5
    x = torch.from_numpy(rng.normal(0, 2, (T, B, V)))
    x[2, 0, 2] = -np.inf
    x[:, 1, 4] = -np.inf
    lens = [6, 5, 3]
    hyps = [[[1], [3, 1], [2, 4], [1, 3, 1], None, [1, 1, 1, 1]],
            [[4, 1], [3], [], [1, 2], [0, 1], [3, 3]],
            [[1, 3], [2], [3, 1, 3], [5], [], [1, 1]]]
    w = rng.normal(0, 1.5, (B, 6))
    cls = nr.classes_of(V, canon)
    sc, g = _brute(x, lens, hyps, cls, w)
    got_sc, got_g = nr.nbest(x, lens, hyps, canon, w)
    fin = np.isfinite(sc)
    assert (np.isfinite(got_sc.numpy()) == fin).all(), (sc, got_sc)
    assert fin.sum() >= 10 and (~fin).sum() >= 3
    assert np.abs(got_sc.numpy()[fin] - sc[fin]).max() < 1e-13
    assert float((got_g - g).abs().max()) < 1e-13
    assert float(got_g[5:, 1].abs().max()) == 0 and float(got_g[3:, 2].abs().max()) == 0
    if canon is not None:                                           # the members of a class share its occupancy by their softmax share
        assert float(g.abs().max()) > 1e-3


def test_restatement_equals_ctc_ref_at_n1():
    for name, regime in (("act_edges", cr.PEAKY8), ("patterns64", cr.DENSE), ("tight64", cr.DENSE), ("mix128", cr.PEAKY8)):
        x, flat, ll, act, labs = cr.build_case(name, regime)
        nll, grad, _, _ = cr.ctc(x, flat, ll, act)
        sc, g = nr.nbest(x, act, [[l] for l in labs], None, -np.ones((len(labs), 1)))
        fin = torch.isfinite(nll)
        assert bool((torch.isfinite(sc[:, 0]) == fin).all())
        assert float((sc[:, 0] + nll)[fin].abs().max()) < 1e-10
        # ctc_ref gives an infeasible line its softmax row; a hypothesis without a score contributes nothing here
        assert float((g - grad)[:, fin].abs().max()) < 1e-12 and float(g[:, ~fin].abs().max() if (~fin).any() else 0) == 0
        ref, own = cr.Reference(x, flat, ll, act), nr.Reference(x, act, [[l] for l in labs], None, -np.ones((len(labs), 1)))
        both = (ref.grad_bar > 0) & fin.view(1, -1, 1)
        # the same derivation: the n = 1 bar is ctc_ref's plus the accumulation term R = U (K + 5) (y + occ), K <= 64 positions of a class
        # here, against C_GRAD y (e_lp + 2 U) >= 18 U y: at most 1 + 69 / 18 times ctc_ref's
        r = own.grad_bar[both] / ref.grad_bar[both]
        assert 1.0 <= float(r.min()) and float(r.max()) < 1 + 69 / 18, (name, float(r.min()), float(r.max()))


def test_risk_terms_and_gradient_by_autograd():
    """the coefficients c_q = p_q (W_q - risk) are the derivative of the risk with respect to the scores, and the risk's logit gradient is
    the weighted n-best gradient at c (brute force again)"""
    rng = np.random.default_rng(9)
    T, B, V = 5, 2, 4
    x = torch.from_numpy(rng.normal(0, 1.5, (T, B, V)))
    hyps = [[[1], [2, 1], [3], [1, 1, 1, 1]], [[2], [2, 3], [1], []]]
    errors = np.array([[0, 1, 1, 3], [1, 0, 2, 1]], dtype=np.float64)
    filled = np.array([[1, 1, 1, 1], [1, 1, 0, 1]], dtype=bool)
    cls = nr.classes_of(V, None)
    xx = x.clone().requires_grad_(True)
    total = torch.zeros((), dtype=torch.float64)
    for b in range(B):
        s = [nr.brute_force(xx[:, b], T, h, cls) for h in hyps[b]]
        keep = [q for q in range(4) if filled[b, q] and s[q] is not None]
        p = torch.softmax(torch.stack([s[q] for q in keep]), 0)
        total = total + (p * torch.tensor([errors[b, q] for q in keep])).sum()
    total.backward()
    risk, bar, c, g, gbar, scores, member = nr.risk_reference(x, [T, T], hyps, None, errors, filled)
    assert member.tolist() == [[True, True, True, False], [True, True, False, True]]
    assert abs(risk.sum() - float(total.detach())) < 1e-12 and np.abs(c.sum(1)).max() < 1e-15
    assert float((g - xx.grad).abs().max()) < 1e-13
    assert (bar > 0).all() and float(gbar.min()) > 0


def test_product_risk_terms_on_the_cpu():
    """risk.risk_terms is plain torch: on CPU tensors it gives the restatement's risk and coefficients, empty lists included"""
    from vistaocr_amd import risk as rk
    rng = np.random.default_rng(2)
    scores = rng.normal(-20, 5, (5, 6))
    errors = rng.integers(0, 7, (5, 6)).astype(np.float64)
    member = rng.random((5, 6)) < 0.7
    member[3] = False
    scores[~member] = np.where(rng.random((~member).sum()) < 0.5, -np.inf, scores[~member])
    risk, c, p, _ = nr.risk_terms(scores, errors, member)
    got = rk.risk_terms(torch.from_numpy(errors), torch.from_numpy(scores), torch.from_numpy(member))
    assert np.abs(got[0].numpy() - risk).max() < 1e-12 and np.abs(got[1].numpy() - c).max() < 1e-12 and np.abs(got[2].numpy() - p).max() < 1e-12
    assert risk[3] == 0 and np.abs(c[3]).max() == 0 and np.abs(c.sum(1)).max() < 1e-14 and not np.isnan(got[1].numpy()).any()
    got32 = rk.risk_terms(torch.from_numpy(errors).float(), torch.from_numpy(scores).float(), torch.from_numpy(member))
    assert not bool(torch.isnan(got32[1]).any()) and np.abs(got32[0].numpy() - risk).max() < 1e-4


_cache = {}


def _reference(name):
    if name not in _cache:
        k = nc.build_case(name)
        _cache[name] = (k, nr.Reference(k["x"], k["lens"], k["hyps"], k["canon"], k["w"], k["M"]))
    return _cache[name]


@pytest.mark.parametrize("name", [c[0] for c in nc.CASES])
def test_fp32_formulas_stay_within_a_quarter_of_the_bars(name):
    k, ref = _reference(name)
    s32, g32 = nr.nbest(k["x"], k["lens"], k["hyps"], k["canon"], k["w"], k["M"], dtype=torch.float32)
    fin = torch.isfinite(ref.scores)
    assert bool((torch.isfinite(s32) == fin).all()) and not bool(torch.isnan(s32).any()) and not bool(torch.isnan(g32).any())
    assert not bool(torch.isnan(ref.grad).any()) and bool(torch.isfinite(ref.grad).all())
    sfrac = 0.0
    if bool(fin.any()):
        sfrac = float(((s32.double() - ref.scores).abs()[fin] / torch.from_numpy(nr.eps_line(k["T"], ref.scores[fin].numpy()))).max())
    gfrac = cr.ratio(g32, ref.grad, ref.grad_bar)
    print("nbest-cpu %-14s fp32 formulas: score diff / eps_line %.3f  grad diff / bar %.3f" % (name, sfrac, gfrac))
    assert gfrac <= 0.25, (name, gfrac)
    assert sfrac <= 1.0, (name, sfrac)          # eps_line is the project's bar for the sweep, not derived here: 4 U at T = 1


@pytest.mark.parametrize("mutant", nr.MUTANTS)
def test_every_mutant_misses_a_bar_by_10x(mutant):
    """no_share: the member share p(v) / P(class) dropped; no_wsum: the - y sum(w) term dropped; inf_kept: a hypothesis without a score
    still counted in sum(w)"""
    worst = {}
    for name in nc.MUTANT_CASES:
        k, ref = _reference(name)
        _, g = nr.nbest(k["x"], k["lens"], k["hyps"], k["canon"], k["w"], k["M"], mutant=mutant)
        worst[name] = cr.ratio(g, ref.grad, ref.grad_bar)
    print("nbest-cpu mutant %-9s misses by %s" % (mutant, {k: "%.3g" % v for k, v in worst.items()}))
    assert max(worst.values()) >= 10.0, worst


def test_case_list_covers_what_it_claims():
    """the shapes the GPU file relies on are really in the list: both lattice regimes and the seam, the edges of lens, the specials"""
    longest = {c[0]: max(max((len(h) for h in row if h is not None), default=0) for row in nc.build_case(c[0])["hyps"]) for c in nc.CASES}
    assert longest["seam31"] == 31 and longest["seam32"] == 32 and longest["seam33"] == 33 and longest["long_peaky"] >= 100
    assert {c[3] for c in nc.CASES} >= {2, 5, 96, 166, 256} and {c[4] for c in nc.CASES} >= {1, 3, 128}
    assert {c[1] for c in nc.CASES} >= {1, nr.TT - 1, nr.TT, nr.TT + 1, 2 * nr.TT + 1, 294}
    lens = {v for c in nc.CASES for v in nc.build_case(c[0])["lens"]}
    assert lens >= {0, 1, nr.PF - 1, nr.PF, nr.PF + 1, nr.PF + 2, 8 * nr.TB, 8 * nr.TB + 1, 8 * nr.TB + 2}
    k = nc.build_case("tight")
    assert all(cr.need(row[0]) == ln for row, ln in zip(k["hyps"], k["lens"]))
    sc = _reference("specials")[1].scores
    assert int((~torch.isfinite(sc)).sum()) >= 4
    assert not bool(torch.isfinite(_reference("dead_frame")[1].scores[0]).any())


def test_argument_validation_without_gpu():
    from vistaocr_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    ws = lib.vocr_ctc_nbest_workspace_bytes
    clp = 294 * 32 * 96 * 4
    assert ws(294, 32, 96, 16, 100) == clp + 32 * 16 * 8 * 294 * 201
    assert ws(294, 32, 96, 16, 100) == lib.vocr_ctc_edit_workspace_bytes(294, 32, 96, 16, 100)
    assert ws(294, 32, 1, 16, 100) == 0 and ws(294, 32, 257, 16, 100) == 0 and ws(294, 32, 96, 0, 100) == 0 and ws(294, 32, 96, 129, 100) == 0
    assert ws(294, 32, 96, 16, 295) == 0 and ws(294, 32, 96, 16, -1) == 0 and ws(0, 32, 96, 16, 0) == 0
    assert ws(294, 32, 96, 128, 294) == 0                          # 2.8 GiB of lattices
    assert ws(1 << 20, 1 << 10, 96, 2, 0) == 0                     # t * b * n = 2^31

    def go(logits=one, lens=one, t=20, b=2, v=10, canon=None, labels=one, label_lens=one, n=3, stride=5, m=5, weights=one, out=one,
           dlogits=one, wsp=one, nbytes=1 << 30):
        return lib.vocr_ctc_nbest_grad(logits, lens, t, b, v, canon, labels, label_lens, n, stride, m, weights, out, dlogits, wsp, nbytes, None)

    for kw in (dict(logits=None), dict(lens=None), dict(labels=None), dict(label_lens=None), dict(out=None), dict(wsp=None)):
        assert go(**kw) == -1 and b"vocr_ctc_nbest_grad: null pointer" in lib.vocr_last_error(), kw
    assert go(dlogits=None) == -1 and b"weights and dlogits go together" in lib.vocr_last_error()
    assert go(weights=None) == -1 and b"weights and dlogits go together" in lib.vocr_last_error()
    assert go(v=1) == -1 and go(v=257) == -1 and b"2 <= v <= 256" in lib.vocr_last_error()
    assert go(n=0) == -1 and go(n=129) == -1 and b"1 <= n <= 128" in lib.vocr_last_error()
    assert go(m=21, stride=21) == -1 and b"max_label_len" in lib.vocr_last_error()
    assert go(m=5, stride=4) == -1 and go(m=-1) == -1 and go(t=0) == -1 and go(b=0) == -1
    assert go(t=294, b=32, v=96, n=128, stride=294, m=294) == -1 and b"unsupported shape" in lib.vocr_last_error()
    need = ws(20, 2, 10, 3, 5)
    assert go(nbytes=need - 1) == -1 and b"workspace too small" in lib.vocr_last_error()
    # a scores-only call needs the class log-probabilities alone, and checks for them
    assert go(weights=None, dlogits=None, nbytes=20 * 2 * 10 * 4 - 1) == -1 and b"workspace too small" in lib.vocr_last_error()
