"""CPU: the fp64 restatement of tests/entropy_ref.py (ln P, the alignment entropy H and their closed-form gradient) held to the
enumeration of every class path, to central differences and to the closed form on uniform logits; and the argument validation of
vocr_ctc_entropy / vocr_ctc_entropy_workspace_bytes, which needs no GPU."""
import ctypes
import itertools
import math

import numpy as np
import pytest

from tests import entropy_ref as er

CANON_PAIR = [0, 1, 1, 3]                 # columns 1 and 2 are one class


@pytest.mark.parametrize("canon", [None, CANON_PAIR])
def test_restatement_equals_enumeration_of_all_paths(canon):
    """all paths at T <= 6, V = 4: repeated labels, a two-member class (a label given as its non-canonical member), L = 0, a labelling
    that does not fit, one that meets a -inf class, ragged lengths"""
    rng = np.random.default_rng(11)
    T, V = 6, 4
    cls = er.classes_of(V, canon)
    x = rng.normal(0, 2, (T, 8, V))
    x[:, 6, 3] = -np.inf
    x[2, 7, 1] = -np.inf
    labs = [[1], [1, 3], [1, 1], [3, 1, 3], [], [3, 3, 3, 3], [3, 1], [2, 3, 2]]
    lens = [6, 5, 6, 6, 4, 6, 6, 6]
    seen_inf = 0
    for b, (lab, n) in enumerate(zip(labs, lens)):
        want_p, want_h = er.brute_force(x[:, b], n, lab, cls)
        r = er.line(x[:, b], n, lab, cls)
        if not np.isfinite(want_p):
            seen_inf += 1
            assert r["lnp"] == -np.inf and r["H"] == 0.0 and float(np.abs(r["grad"]).max()) == 0.0, b
            continue
        assert abs(r["lnp"] - want_p) < 1e-13 and abs(r["H"] - want_h) < 1e-12, (b, r["lnp"], want_p, r["H"], want_h)
        assert r["H"] >= 0.0
    assert seen_inf == 2                                             # four equal labels need 7 frames; class 3 is -inf on line 6
    assert er.line(x[:, 4], 4, [], cls)["H"] < 1e-13                 # L = 0: one path
    assert er.line(x[:, 0], 0, [], cls)["lnp"] == 0.0 and er.line(x[:, 0], 0, [1], cls)["lnp"] == -np.inf
    assert er.line(x[:, 0], 6, [0], cls)["lnp"] == -np.inf and er.line(x[:, 0], 6, [4], cls)["lnp"] == -np.inf


@pytest.mark.parametrize("canon", [None, CANON_PAIR])
def test_gradient_equals_central_differences(canon):
    """d(w_ctc ln P + w_ent H)/dlogits of the closed form against central differences of the restatement's own scores, element by element;
    a line with a -inf column and a ragged one among them; the entropy's gradient sums to 0 over every frame"""
    rng = np.random.default_rng(3)
    T, V = 7, 4
    cls = er.classes_of(V, canon)
    cases = [([1, 3], 7, None), ([1, 1], 7, None), ([2, 3, 2], 6, None), ([], 5, None), ([3], 7, 1), ([1, 3, 1, 3], 7, None)]
    eps = 1e-6
    for lab, n, dead in cases:
        x = rng.normal(0, 1.5, (T, V))
        if dead is not None:
            x[:, dead] = -np.inf
        for wc, we in ((1.0, 0.0), (0.0, 1.0), (-1.0, -0.3)):
            r = er.line(x, n, lab, cls, None, wc, we)
            assert np.isfinite(r["lnp"])
            num = np.zeros_like(x)
            for t in range(T):
                for v in range(V):
                    if not np.isfinite(x[t, v]):
                        continue
                    xp, xm = x.copy(), x.copy()
                    xp[t, v] += eps
                    xm[t, v] -= eps
                    rp, rm = er.line(xp, n, lab, cls), er.line(xm, n, lab, cls)
                    num[t, v] = (wc * (rp["lnp"] - rm["lnp"]) + we * (rp["ratio"] + rp["lnp"] - rm["ratio"] - rm["lnp"])) / (2 * eps)
            assert float(np.abs(r["grad"] - num).max()) < 2e-8, (lab, n, wc, we, float(np.abs(r["grad"] - num).max()))
            assert float(np.abs(r["grad"][n:]).max() if n < T else 0.0) == 0.0
        assert float(np.abs(r["dH"].sum(1)).max()) < 1e-13 and float(np.abs(r["dP"].sum(1)).max()) < 1e-13


def test_uniform_logits_closed_form():
    """every feasible path is equally likely: H = ln(count), ln P = H - len * ln V, the count from the integer recursion (checked
    against enumeration where that is possible)"""
    V = 5
    cls = er.classes_of(V, None)
    for lab, n in (([1], 4), ([1, 2], 5), ([2, 2], 6), ([1, 2, 1], 6)):
        feas = sum(1 for fr in itertools.product(range(V), repeat=n)
                   if [k for i, k in enumerate(fr) if k != 0 and (i == 0 or fr[i - 1] != k)] == lab)
        assert er.count_paths(n, lab) == feas, (lab, n)
    assert er.count_paths(3, [1, 1]) == 1 and er.count_paths(2, [1, 1]) == 0 and er.count_paths(0, []) == 1 and er.count_paths(7, []) == 1
    for lab, n, V in (([1, 2, 3, 3, 1], 40, 7), ([], 9, 3), ([4] * 20, 60, 96), (list(range(1, 60)), 294, 96)):
        x = np.full((n, V), 0.25)
        r = er.line(x, n, lab, er.classes_of(V, None))
        cnt = er.count_paths(n, lab)
        assert cnt >= 1
        assert abs(r["H"] - math.log(cnt)) < 1e-9 * max(1.0, math.log(cnt)), (lab[:3], n, r["H"], math.log(cnt))
        assert abs(r["lnp"] - (math.log(cnt) - n * math.log(V))) < 1e-9 * n


def test_need_and_tight_lines_have_zero_entropy():
    cls = er.classes_of(6, None)
    rng = np.random.default_rng(1)
    for lab in ([1, 1, 2], [3], [2, 2, 2, 2], [1, 2, 3]):
        n = er.need(lab)
        assert er.count_paths(n, lab) == 1 and er.count_paths(n - 1, lab) == 0
        r = er.line(rng.normal(0, 2, (n, 6)), n, lab, cls, None, 0.0, 1.0)
        assert abs(r["H"]) < 1e-12 and float(np.abs(r["grad"]).max()) < 1e-12


def test_argument_validation_without_gpu():
    from vistaocr_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "vocr_ctc_entropy") and hasattr(lib, "vocr_ctc_entropy_workspace_bytes")
    one = ctypes.c_void_p(16)
    ws = lib.vocr_ctc_entropy_workspace_bytes
    clp = 294 * 32 * 96 * 4
    assert ws(294, 32, 96, 100, 0) == clp
    assert ws(294, 32, 96, 100, 1) == clp + 32 * 16 * 294 * 201 > ws(294, 32, 96, 100, 0)
    assert ws(294, 32, 1, 100, 1) == 0 and ws(294, 32, 257, 100, 1) == 0 and ws(294, 32, 96, 295, 1) == 0 and ws(294, 32, 96, -1, 0) == 0
    assert ws(0, 32, 96, 0, 0) == 0 and ws(294, 0, 96, 10, 0) == 0
    assert ws(2000, 1, 96, 1663, 1) > 0 and ws(2000, 1, 96, 1664, 1) == 0 and ws(2000, 1, 96, 1664, 0) == 0      # the paired rows' LDS limit
    assert lib.vocr_ctc_nbest_workspace_bytes(2000, 1, 96, 1, 1664) > 0                                         # ... which is this entry's alone
    assert ws(2000, 400, 96, 1663, 1) == 0 and ws(2000, 400, 96, 1663, 0) == 0                                 # 42 GB of lattices

    def go(logits=one, lens=one, t=20, b=2, v=10, canon=None, labels=one, label_lens=one, stride=5, m=5, coeff=one, ctc=one, ent=one,
           dlogits=one, wsp=one, nbytes=1 << 30):
        return lib.vocr_ctc_entropy(logits, lens, t, b, v, canon, labels, label_lens, stride, m, coeff, ctc, ent, dlogits, wsp, nbytes, None)

    for kw in (dict(logits=None), dict(lens=None), dict(labels=None), dict(label_lens=None), dict(ctc=None), dict(ent=None), dict(wsp=None)):
        assert go(**kw) == -1 and b"vocr_ctc_entropy: null pointer" in lib.vocr_last_error(), kw
    assert go(dlogits=None) == -1 and b"vocr_ctc_entropy: coeff and dlogits go together" in lib.vocr_last_error()
    assert go(coeff=None) == -1 and b"vocr_ctc_entropy: coeff and dlogits go together" in lib.vocr_last_error()
    assert go(v=257) == -1 and b"vocr_ctc_entropy" in lib.vocr_last_error() and b"2 <= v <= 256" in lib.vocr_last_error()
    assert go(v=1) == -1 and go(t=0) == -1 and go(b=0) == -1 and go(m=-1) == -1 and go(m=5, stride=4) == -1
    assert go(m=21, stride=21) == -1 and b"max_label_len" in lib.vocr_last_error()
    assert go(t=2000, b=1, v=96, stride=1664, m=1664) == -1 and b"vocr_ctc_entropy: unsupported shape" in lib.vocr_last_error()
    need = ws(20, 2, 10, 5, 1)
    assert go(nbytes=need - 1) == -1 and b"vocr_ctc_entropy: workspace too small" in lib.vocr_last_error()
    assert go(coeff=None, dlogits=None, nbytes=ws(20, 2, 10, 5, 0) - 1) == -1 and b"workspace too small" in lib.vocr_last_error()


def test_criterion_refuses_bad_arguments_without_gpu():
    import torch
    import vistaocr_amd as va
    with pytest.raises(ValueError, match="beta"):
        va.EntropyRegularizedCTCLoss(-0.1)
    with pytest.raises(TypeError):
        va.EntropyRegularizedCTCLoss()
    crit = va.EntropyRegularizedCTCLoss(0.2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(torch.zeros(4, 1, 9), torch.tensor([1], dtype=torch.int32), torch.tensor([4], dtype=torch.int32),
             torch.tensor([1], dtype=torch.int32))
