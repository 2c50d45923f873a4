"""CPU: the CTC restatement of tests/ctc_ref.py against torch.nn.functional.ctc_loss in double precision and against the plain-C
restatement oracle/ctc_ref.c (also on the empty and infeasible lines, where torch yields NaN gradients), the closed form of a line with
one feasible path, and the bars of tests/test_ctc_fp64_gpu.py: both fp32 formulations within a quarter of every bar on the whole GPU case
list, every mutant (a CTC that is wrong on purpose) at least 10x over one."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ctc_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _cpu_threads():
    """the CPU references at no more than 16 threads (what a GPU host gives one command); the caller's count is restored afterwards"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def cref():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "libctc_ref.so"))
    lib.ctc_ref.restype = ctypes.c_int
    return lib


_refs = {}


def reference(name, regime):
    key = (name, regime)
    if key not in _refs:
        case = cr.build_case(name, regime)
        _refs[key] = (case, cr.Reference(*case[:4]))
    return _refs[key]


@pytest.mark.parametrize("name,regime", [("B1", cr.DENSE), ("V257", cr.PEAKY8), ("patterns64", cr.DENSE), ("mix128", cr.DENSE),
                                         ("tight64", cr.DENSE), ("mix_generic", cr.PEAKY8), ("V2", cr.DENSE)],
                         ids=lambda v: v if isinstance(v, str) else cr.regime_name(v))
def test_fp64_restatement_is_torch_ctc_loss(name, regime):
    """per line (reduction="none") and the autograd gradient, on the feasible lines with at least one frame"""
    x, flat, ll, act, _ = cr.build_case(name, regime)
    nll, grad, _, _ = cr.ctc(x, flat, ll, act)
    ok = [b for b in range(len(ll)) if act[b] > 0 and bool(torch.isfinite(nll[b]))]
    assert len(ok) >= max(1, len(ll) - 1)
    lr = x[:, ok].double().requires_grad_(True)
    labs = [flat[sum(ll[:b]):sum(ll[:b + 1])].long() for b in ok]
    ref = F.ctc_loss(F.log_softmax(lr, 2), torch.cat(labs) if labs else flat[:0].long(), torch.tensor([act[b] for b in ok]),
                     torch.tensor([ll[b] for b in ok]), blank=0, reduction="none")
    ref.sum().backward()
    assert float((nll[ok] - ref.detach()).abs().max()) <= 1e-10 * (1 + float(ref.detach().abs().max()))
    assert float((grad[:, ok] - lr.grad).abs().max()) <= 1e-10


@pytest.mark.parametrize("name,regime", [("act_edges", cr.DENSE), ("act_edges", cr.SAT), ("T1", cr.PEAKY8), ("V2", cr.PEAKY8), ("mix64", cr.DENSE),
                                         ("mix128", cr.PEAKY8), ("mix_generic", cr.DENSE), ("patterns128", cr.PEAKY8), ("V4096", cr.DENSE),
                                         ("tight_generic", cr.DENSE)],
                         ids=lambda v: v if isinstance(v, str) else cr.regime_name(v))
def test_fp64_restatement_is_the_c_oracle_everywhere(cref, name, regime):
    x, flat, ll, act, _ = cr.build_case(name, regime)
    T, B, V = x.shape
    nll, grad, alpha, beta = cr.ctc(x, flat, ll, act)
    xs = np.ascontiguousarray(x.numpy())
    c_nll = np.zeros(B, dtype=np.float64)
    c_grad = np.full((T, B, V), np.nan, dtype=np.float64)
    lab = np.ascontiguousarray(flat.numpy())
    rc = cref.ctc_ref(xs.ctypes.data_as(ctypes.c_void_p), lab.ctypes.data_as(ctypes.c_void_p),
                      np.asarray(ll, dtype=np.int32).ctypes.data_as(ctypes.c_void_p),
                      np.asarray(act, dtype=np.int32).ctypes.data_as(ctypes.c_void_p), T, B, V,
                      c_nll.ctypes.data_as(ctypes.c_void_p), c_grad.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    c_nll, c_grad = torch.from_numpy(c_nll), torch.from_numpy(c_grad)
    assert torch.equal(torch.isinf(nll), torch.isinf(c_nll))
    fin = torch.isfinite(nll)
    assert float((nll[fin] - c_nll[fin]).abs().max()) <= 1e-10 * (1 + float(nll[fin].abs().max()))
    assert not torch.isnan(grad).any() and torch.isfinite(grad).all()
    assert float((grad - c_grad).abs().max()) <= 1e-10
    for b in range(B):
        assert not grad[act[b]:, b].any()
        assert torch.isinf(alpha[act[b]:, b]).all() and torch.isinf(beta[act[b]:, b]).all()
        if act[b] == 0:
            assert float(nll[b]) == (0.0 if ll[b] == 0 else float("inf"))
        elif not bool(fin[b]):                                           # infeasible: zero occupancy, the gradient is the softmax row
            assert torch.allclose(grad[:act[b], b], torch.softmax(x[:act[b], b].double(), 1), rtol=0, atol=1e-15)


def test_both_fp64_formulations_agree():
    x, flat, ll, act, _ = cr.build_case("patterns128", cr.PEAKY8)
    a, b = cr.ctc(x, flat, ll, act, form="kernel"), cr.ctc(x, flat, ll, act, form="pairwise")
    assert float((a[0] - b[0]).abs().max()) <= 1e-11 and float((a[1] - b[1]).abs().max()) <= 1e-12


@pytest.mark.parametrize("name,regime", [("tight64", cr.DENSE), ("tight64", cr.SAT), ("tight128", cr.DENSE), ("tight_generic", cr.DENSE)],
                         ids=lambda v: v if isinstance(v, str) else cr.regime_name(v))
def test_tight_lines_have_the_closed_form(name, regime):
    (x, flat, ll, act, labs), ref = reference(name, regime)
    B = len(ll)
    for b in range(B // 2):
        assert act[b] == cr.need(labs[b])
        cn, cg = cr.tight_closed_form(x[:, b], labs[b], act[b])
        assert abs(float(ref.nll[b]) - float(cn)) <= 1e-10 * (1 + abs(float(cn)))
        assert float((ref.grad[:act[b], b] - cg).abs().max()) <= 1e-12
    for b in range(B // 2, B):
        assert act[b] == cr.need(labs[b]) + 1 and bool(torch.isfinite(ref.nll[b]))


def test_builders_produce_what_they_claim():
    # tight: exactly one path at need(lab) frames, more with one frame to spare, none with one too few
    for lab in ([1, 1, 2], [2, 1], [1, 1, 1], [3]):
        n = cr.need(lab)
        assert cr.count_paths(lab, n) == 1 and cr.count_paths(lab, n + 1) > 1 and cr.count_paths(lab, n - 1) == 0
    assert cr.need([1, 1, 2]) == 4 and cr.need([]) == 0 and cr.need([5, 6, 5]) == 3
    # a random alignment is a valid path of its labelling
    rng = np.random.default_rng(5)
    for lab, tb in (([4, 4, 2, 9], 5), ([4, 4, 2, 9], 30), ([], 3), ([7], 1), ([1, 2] * 10, 20)):
        p = cr.random_alignment(rng, lab, tb)
        out, prev = [], None
        for v in p:
            if v != prev and v != 0:
                out.append(v)
            prev = v
        assert len(p) == tb and out == lab
    assert cr.random_alignment(rng, [4, 4], 2) is None
    # label kinds
    assert len(set(cr.make_labels(rng, 96, 20, "equal"))) == 1
    ab = cr.make_labels(rng, 96, 31, "abab")
    assert len(set(ab)) == 2 and all(ab[i] != ab[i + 1] and ab[i] == ab[i + 2] for i in range(29))
    rl = cr.make_labels(rng, 166, 12, "random")
    assert rl[0] == rl[1] and 1 in rl and 165 in rl
    # the c4 batch crosses every seam value; the edge batch holds every act_len of the list
    assert {0, 7, 31, 32, 33, 62, 63} <= set(cr._L_C4) and 31 in cr._L_BENCH and max(cr._L_BENCH) == 31
    assert [0, 1, 2, 8, 9, 10, 16, 17] == sorted(set(cr.build_case("act_edges", cr.DENSE)[3]))
    ls = {l for spec in cr.GPU_CASES for l in spec[4]}
    assert {0, 1, 31, 32, 33, 63, 64, 65} <= ls and max(ls) > 128
    assert {2, 63, 64, 65, 257, 4096} <= {spec[3] for spec in cr.GPU_CASES}
    # peaky: trained-like.  The labelling's nll is at most its margin path's; with margin m and unit noise the mean cost of a frame
    # on that path is <= ln(1 + (V - 1) e^(1 - m)) (Jensen: E e^(n_i - n_0) = e).  The stated bound takes e^(2.5 - m), 4.5x that, for
    # the spread of the short lines: nll <= act_len ln(1 + (V - 1) e^(2.5 - m))
    for name, regime in (("c4_ragged", cr.PEAKY8), ("c4_ragged", cr.PEAKY15), ("bench_ragged", cr.PEAKY8), ("generic_long", cr.PEAKY8)):
        (x, flat, ll, act, labs), ref = reference(name, regime)
        V = x.shape[2]
        bound = torch.tensor(act, dtype=torch.float64) * float(np.log1p((V - 1) * np.exp(2.5 - regime[1])))
        assert bool(torch.isfinite(ref.nll).all()) and bool((ref.nll <= bound).all()), (name, regime)
    (x, flat, ll, act, labs), ref = reference("c4_ragged", cr.PEAKY15)
    assert float(ref.nll.max()) < 1.0


@pytest.mark.parametrize("name,regime", list(cr.all_cases()), ids=lambda v: v if isinstance(v, str) else cr.regime_name(v))
def test_both_fp32_formulations_use_a_quarter_of_every_bar(name, regime):
    (x, flat, ll, act, labs), ref = reference(name, regime)
    for form in ("kernel", "pairwise"):
        nll, grad, _, _ = cr.ctc(x, flat, ll, act, torch.float32, form=form)
        rn, rg = cr.ratio(nll, ref.nll, ref.nll_bar), cr.ratio(grad, ref.grad, ref.grad_bar)
        print("%-17s %-12s %-8s nll %.3f of its bar (max err %.2e), grad %.3f (%.2e)" % (
            name, cr.regime_name(regime), form, rn, cr.max_err(nll, ref.nll), rg, cr.max_err(grad, ref.grad)))
        assert rn <= 0.25 and rg <= 0.25, (form, rn, rg)
    _refs.pop((name, regime), None)                                     # the large cases are not needed again


@pytest.mark.parametrize("mutant", cr.MUTANTS)
def test_every_mutant_misses_a_bar_by_10x(mutant):
    worst = 0.0
    for name, regime in cr.MUTANT_CASES:
        (x, flat, ll, act, labs), ref = reference(name, regime)
        nll, grad, _, _ = cr.ctc(x, flat, ll, act, torch.float32, mutant=mutant)
        r = max(cr.ratio(nll, ref.nll, ref.nll_bar), cr.ratio(grad, ref.grad, ref.grad_bar))
        print("%-12s on %-12s %-10s: %.3g of a bar" % (mutant, name, cr.regime_name(regime), r))
        worst = max(worst, r)
    assert worst >= 10.0, "mutant %r stays within 10x of every bar" % mutant
    # the peaky step-length case is where the issue's subtle mutants must show
    if mutant in ("seam", "prefetch", "dup"):
        (x, flat, ll, act, labs), ref = reference("c4_ragged", cr.PEAKY8)
        nll, grad, _, _ = cr.ctc(x, flat, ll, act, torch.float32, mutant=mutant)
        assert max(cr.ratio(nll, ref.nll, ref.nll_bar), cr.ratio(grad, ref.grad, ref.grad_bar)) >= 10.0
