"""GPU: vocr_ctc_nbest_grad (vistaocr_amd/csrc/ctc_nbest.hip) against the fp64 restatement of tests/nbest_ref.py on the cases of
tests/nbest_cases.py.  Every element of both outputs is compared: -inf exactly where the restatement has it and never a NaN, rows past
`lens` exactly 0, finite scores within the project's eps_line(T, score) and finite gradient elements within the bars derived at the
head of tests/nbest_ref.py.  The entry point is called with a NaN-filled workspace and NaN-filled outputs.

What the shapes are for (the constants are those of the kernels): the lattice kernel keeps labellings of up to 31 labels in registers
(seam31 / seam32 / seam33: S = 63, 65, 67; long_*: ~100 labels at T = 294) and prefetches PF = 8 frames there (lens 7 .. 10), beyond it
stages TB = 8 frames per pass (lens 64, 65, 66); the gradient kernel works on tiles of TT = 16 frames (T = 1, 15, 16, 17, 33) with the
hypotheses in QG = 4 groups (n = 1, 3, 128); V = 2, 5, 96, 166, 256.  Each case prints the worst fraction of its bars
(profiles/ctc_nbest_errors.txt)."""
import numpy as np
import pytest
import torch

from tests import ctc_ref as cr
from tests import nbest_cases as nc
from tests import nbest_ref as nr

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _raw(x, lens, labels, label_lens, M, canon=None, w=None):
    """the C entry point itself, every buffer NaN-filled first; returns device tensors (scores [B,n], dlogits [T,B,V] or None)"""
    from vistaocr_amd import _lib, ops
    T, B, V = x.shape
    n, stride = int(labels.shape[1]), int(labels.shape[2])
    nbytes = _lib.load().vocr_ctc_nbest_workspace_bytes(T, B, V, n, M)
    assert nbytes > 0
    ws = torch.full(((nbytes + 3) // 4,), NAN, dtype=torch.float32, device=x.device)
    scores = torch.full((B, n), NAN, dtype=torch.float32, device=x.device)
    dl = torch.full((T, B, V), NAN, dtype=torch.float32, device=x.device) if w is not None else None
    p = ops._p
    _lib.call("vocr_ctc_nbest_grad", p(x), p(lens), T, B, V, p(canon), p(labels), p(label_lens), n, stride, M, p(w), p(scores), p(dl),
              p(ws), ws.numel() * 4, ops._stream())
    return scores, dl


def _device_case(k, dev="cuda"):
    labels, label_lens = nr.pack(k["hyps"], k["M"], dev)
    canon = None if k["canon"] is None else torch.tensor(k["canon"], dtype=torch.int32, device=dev)
    return (k["x"].to(dev), torch.tensor(k["lens"], dtype=torch.int32, device=dev), labels, label_lens, canon,
            torch.from_numpy(k["w"].astype(np.float32)).to(dev))


def _check(name, T, scores, grad, ref, lens):
    """every element of both outputs against the restatement; returns the worst fractions (score / eps_line, grad / bar)"""
    got_s, got_g = scores.cpu().double(), grad.cpu().double()
    assert not bool(torch.isnan(got_s).any()) and not bool(torch.isnan(got_g).any()), name
    fin = torch.isfinite(ref.scores)
    assert bool(((got_s == cr.NEG) == ~fin).all()) and bool((torch.isfinite(got_s) == fin).all()), (name, got_s, ref.scores)
    assert bool(torch.isfinite(got_g).all()), name
    for b, ln in enumerate(lens):
        assert float(got_g[min(max(ln, 0), T):, b].abs().max() if ln < T else 0.0) == 0.0, (name, b)
    sfrac = 0.0
    if bool(fin.any()):
        sfrac = float(((got_s - ref.scores).abs()[fin] / torch.from_numpy(nr.eps_line(T, ref.scores[fin].numpy()))).max())
    gfrac = cr.ratio(got_g, ref.grad, ref.grad_bar)
    return sfrac, gfrac


_refs = {}


def _reference(name):
    if name not in _refs:
        k = nc.build_case(name)
        _refs[name] = (k, nr.Reference(k["x"], k["lens"], k["hyps"], k["canon"], k["w"], k["M"]))
    return _refs[name]


@pytest.mark.parametrize("name", [c[0] for c in nc.CASES])
def test_scores_and_gradient_against_fp64(name):
    from vistaocr_amd import ops
    k, ref = _reference(name)
    x, lens, labels, label_lens, canon, w = _device_case(k)
    scores, grad = _raw(x, lens, labels, label_lens, k["M"], canon, w)
    sfrac, gfrac = _check(name, k["T"], scores, grad, ref, k["lens"])
    fin = torch.isfinite(ref.scores)
    print("nbest-errors %-14s T %3d B %d V %3d n %3d longest %3d  scorable %3d / %3d  score diff / eps_line %.3f  grad diff / bar %.3f"
          % (name, k["T"], k["B"], k["V"], k["n"], k["M"], int(fin.sum()), fin.numel(), sfrac, gfrac))
    assert sfrac <= 1.0 and gfrac <= 1.0, (name, sfrac, gfrac)
    # bit-identical: a second run, the scores-only call, the Python entry (its own uninitialised buffers)
    scores2, grad2 = _raw(x, lens, labels, label_lens, k["M"], canon, w)
    assert torch.equal(scores, scores2) and torch.equal(grad, grad2), name
    only, none = _raw(x, lens, labels, label_lens, k["M"], canon, None)
    assert none is None and torch.equal(only, scores), name
    s3, g3 = ops.ctc_nbest(x, k["lens"], labels, label_lens, canon, w)
    assert torch.equal(s3, scores) and torch.equal(g3, grad), name
    s4, g4 = ops.ctc_nbest(x, lens, labels, label_lens, canon)
    assert g4 is None and torch.equal(s4, scores), name
    # the same sweep as the edit scores (bit for bit); the alignment's forward score within both bounds
    assert torch.equal(ops.ctc_edit_scores(x, lens, labels, label_lens, canon)[0], scores), name
    al = ops.ctc_align(x, lens, labels, label_lens, canon)[0][:, :, 1].cpu().double()
    got = scores.cpu().double()
    assert bool((torch.isfinite(al) == torch.isfinite(got)).all()), name
    if bool(fin.any()):
        assert bool(((al - got).abs()[fin] <= 2 * torch.from_numpy(nr.eps_line(k["T"], ref.scores[fin].numpy()))).all()), name
    if name == "zero_weights":
        assert float(grad.abs().max()) == 0.0
    if k["w"].shape[1] > 1 and name in ("V5", "specials", "classes"):          # the duplicate of rank 0 holds rank 0's bits
        assert float(scores[0, 0]) == float(scores[0, k["n"] - 1])


@pytest.mark.parametrize("name", ["seam33", "classes", "specials", "T16", "n128"])
def test_a_line_does_not_depend_on_its_batch(name):
    k, _ = _reference(name)
    x, lens, labels, label_lens, canon, w = _device_case(k)
    scores, grad = _raw(x, lens, labels, label_lens, k["M"], canon, w)
    for b in range(k["B"]):
        s1, g1 = _raw(x[:, b:b + 1].contiguous(), lens[b:b + 1].contiguous(), labels[b:b + 1].contiguous(),
                      label_lens[b:b + 1].contiguous(), k["M"], canon, w[b:b + 1].contiguous())
        assert torch.equal(s1[0], scores[b]) and torch.equal(g1[:, 0], grad[:, b]), (name, b)


@pytest.mark.parametrize("name,regime", [("patterns128", cr.PEAKY8), ("act_edges", cr.PEAKY8), ("mix64", cr.DENSE), ("tight128", cr.DENSE)])
def test_n1_minus_one_agrees_with_the_ctc_loss(name, regime):
    """n = 1, w = -1, no classes: the gradient of the criterion's negative log-likelihood, from another kernel, within the sum of both
    bars; on the lines with one feasible path also the closed form"""
    from vistaocr_amd import _lib, ops
    x, flat, ll, act, labs = cr.build_case(name, regime)
    T, B, V = x.shape
    hyps = [[l] for l in labs]
    M = max(max(ll), 1)
    own = nr.Reference(x, act, hyps, None, -np.ones((B, 1)), M)
    other = cr.Reference(x, flat, ll, act)
    dev = "cuda"
    labels, label_lens = nr.pack(hyps, M, dev)
    xd = x.to(dev)
    lens = torch.tensor(act, dtype=torch.int32, device=dev)
    scores, grad = _raw(xd, lens, labels, label_lens, M, None, torch.full((B, 1), -1.0, device=dev))
    sfrac, gfrac = _check(name, T, scores, grad, own, act)
    off = np.concatenate([[0], np.cumsum(ll)[:-1]]).astype(np.int32)
    nll = torch.empty(B, 1, dtype=torch.float32, device=dev)
    dl = torch.empty_like(xd)
    ws = ops._ws(_lib.load().vocr_ctc_workspace_bytes(T, B, V, max(ll)), dev)
    p = ops._p
    fd, od, ld = flat.to(dev), torch.from_numpy(off).to(dev), torch.tensor(ll, dtype=torch.int32, device=dev)     # kept alive over the call
    _lib.call("vocr_ctc_loss_grad", p(xd), p(fd), p(od), p(ld), p(lens), p(nll), p(dl), p(ws), T, B, V, max(ll), ops._stream())
    feas = torch.isfinite(own.scores[:, 0])
    d = (grad.cpu().double() - dl.cpu().double()).abs()[:, feas]
    bar = (own.grad_bar + other.grad_bar)[:, feas]
    frac = float(torch.where(d == 0, torch.zeros_like(d), d / bar).max())
    print("nbest-errors %-14s n = 1, w = -1 against vocr_ctc_loss_grad: diff / (both bars) %.3f; against fp64: score %.3f grad %.3f"
          % (name, frac, sfrac, gfrac))
    assert sfrac <= 1.0 and gfrac <= 1.0 and frac <= 1.0
    assert bool(((scores[:, 0].cpu().double() + nll[:, 0].cpu().double()).abs()[feas]
                 <= 2 * torch.from_numpy(nr.eps_line(T, own.scores[:, 0][feas].numpy()))).all())
    for b in range(B):
        if labs[b] and cr.need(labs[b]) == act[b]:
            cn, cg = cr.tight_closed_form(x[:, b], labs[b], act[b])
            assert abs(float(scores[b, 0]) + float(cn)) <= nr.eps_line(T, float(cn))
            dd = (grad[:act[b], b].cpu().double() - cg).abs()
            assert bool((dd <= own.grad_bar[:act[b], b]).all()), (name, b)


def test_every_labelling_entry_reports_the_same_forward_score_bits():
    """ln P_ctc(labels | x) is the same expressions in the same order in ctc_label_sweep of ctc_lattice.h and in the alignment's sum
    row, so the alignment's scores[..., 1], the edit scores' ctc and the n-best ctc with and without weights hold the same bits.  One batch on the sweep's seams: T 72, B 4, V 7, n 6;
    columns 1 and 2 are one class and column 6 is -inf in every frame; lens 72, 17, 9 (the first frame apart, PF = TB = 8 frames a
    block: 9 ends on a block, 17 just past one) and 0; labellings of 0, 1, 31, 32, 33 and 36 labels on every line (S = 63, 65, 67
    around the one-wave limit; M = 36 gives the S > 64 instantiation its LDS rows).  On the 72-frame line four are feasible and two have
    no path: the 33 labels hold column 6, and the 32 EQUAL labels need 63 frames, which the 72 offer, so the run that is too long for
    its line is the same labelling on the lines of 17 and 9 frames, like every L > len there (no run of at most 36 labels exceeds 72
    frames: 2 * 36 - 1 = 71).  No NaN logits: the alignment guards its sum row against them by design."""
    from vistaocr_amd import ops
    T, B, V, n = 72, 4, 7, 6
    x = torch.randn(T, B, V, generator=torch.Generator().manual_seed(72))
    x[:, :, 6] = float("-inf")
    canon = torch.tensor([0, 1, 1, 3, 4, 5, 6], dtype=torch.int32, device="cuda")
    lens = [72, 17, 9, 0]
    hyp = [[], [3], [(1, 2, 3, 4, 5)[i % 5] for i in range(31)], [4] * 32,
           [(3, 5)[i % 2] for i in range(16)] + [6] + [(1, 4)[i % 2] for i in range(16)], [(5, 3, 1, 4, 2)[i % 5] for i in range(36)]]
    assert [len(h) for h in hyp] == [0, 1, 31, 32, 33, 36]
    labels, label_lens = nr.pack([hyp] * B, 36, "cuda")
    xd, ld = x.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")
    w = torch.linspace(-1.0, 1.0, B * n, device="cuda").reshape(B, n).contiguous()
    al = ops.ctc_align(xd, ld, labels, label_lens, canon)[0][:, :, 1].contiguous()
    ed = ops.ctc_edit_scores(xd, ld, labels, label_lens, canon)[0]
    nw = ops.ctc_nbest(xd, ld, labels, label_lens, canon, w)[0]
    no = ops.ctc_nbest(xd, ld, labels, label_lens, canon)[0]
    finite = torch.tensor([[1, 1, 1, 1, 0, 1], [1, 1, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]], dtype=torch.bool)
    for name, got in (("align", al), ("edit", ed), ("nbest, weights", nw), ("nbest, scores only", no)):
        got = got.cpu()
        assert tuple(got.shape) == (B, n) and not bool(torch.isnan(got).any()), name
        assert bool((torch.isfinite(got) == finite).all()) and bool((got[~finite] == cr.NEG).all()), (name, got)
        assert float(got[3, 0]) == 0.0, name                                      # no frames, no labels: probability 1
        assert torch.equal(got.view(torch.int32), al.cpu().view(torch.int32)), (name, got, al)


def test_python_entry_shapes_and_errors():
    from vistaocr_amd import ops
    k, ref = _reference("T17")
    x, lens, labels, label_lens, canon, w = _device_case(k)
    s2, g2 = ops.ctc_nbest(x, lens, labels[:, 0].contiguous(), label_lens[:, 0].contiguous(), None, w[:, 0].contiguous())
    assert tuple(s2.shape) == (k["B"],) and tuple(g2.shape) == tuple(x.shape)
    s3, _ = ops.ctc_nbest(x, lens, labels, label_lens)
    assert torch.equal(s2, s3[:, 0])
    with pytest.raises(RuntimeError, match="weights"):
        ops.ctc_nbest(x, lens, labels, label_lens, None, w[:, :2].contiguous())
    with pytest.raises(RuntimeError, match="weights"):
        ops.ctc_nbest(x, lens, labels, label_lens, None, w.double())
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.ctc_nbest(x, lens, labels.repeat(1, 50, 1), label_lens.repeat(1, 50))
