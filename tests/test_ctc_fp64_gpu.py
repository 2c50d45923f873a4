"""GPU: the CTC criterion of ctc.hip (log-softmax, the three alpha/beta launch paths, the gradient kernel) against the fp64 restatement of
tests/ctc_ref.py, per line and per gradient element, under the bars derived there (tests/test_ctc_ref_cpu.py holds those bars to having
teeth), and the greedy decode kernels against a plain host restatement, exactly.

vocr_ctc_loss_grad picks its alpha/beta launch path from max_label_len alone (it only sizes the workspace rows): <= 31 the register kernel
with one position per lane (ctc_alpha_beta_reg_kernel<1>), <= 63 the same with two (<2>), above that the LDS kernel
(ctc_alpha_beta_lds_kernel).  ctc.hip promises that all three give the same bits; every batch here runs through each path that admits it
and the results must be torch.equal.

Every case prints e_k (the kernel's max abs error against fp64), e_32 (the fp32 restatement's) and the fraction of the bar each used -
run with -s to see the table."""
import numpy as np
import pytest
import torch

from tests import ctc_ref as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _cpu_threads():
    """the CPU references at no more than 16 threads (what a GPU host gives one command); the caller's count is restored afterwards"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)


def _offsets(ll):
    return np.concatenate([[0], np.cumsum(ll)[:-1]]).astype(np.int32)


def _workspace(T, B, V, mll, fill=None):
    from vistaocr_amd import _lib
    nbytes = _lib.load().vocr_ctc_workspace_bytes(T, B, V, mll)
    assert nbytes > 0
    ws = torch.empty(nbytes // 4 + 4, dtype=torch.float32, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    return ws


def raw_ctc(x, flat, ll, act, mll, ws=None, fill=None):
    """vocr_ctc_loss_grad on the raw ABI: (nll [B], dlogits [T,B,V]) on the host.  `mll` picks the kernel; `ws`: a workspace to reuse
    (at least as large as this call needs), else a fresh one, filled with `fill` first if given."""
    from vistaocr_amd import _lib
    T, B, V = x.shape
    used = flat[:sum(ll)]
    assert flat.numel() >= 1 and (used.numel() == 0 or (int(used.min()) >= 1 and int(used.max()) < V))          # the ABI's contract
    assert max(ll) <= mll and max(act) <= T and min(act) >= 0 and len(ll) == B and len(act) == B
    need = _lib.load().vocr_ctc_workspace_bytes(T, B, V, mll)
    if ws is None:
        ws = _workspace(T, B, V, mll, fill)
    assert ws.numel() * 4 >= need
    xd = x.contiguous().cuda()
    dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in (flat.numpy(), _offsets(ll), ll, act)]
    nll = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
    dl = torch.full((T, B, V), float("nan"), dtype=torch.float32, device="cuda")
    _lib.call("vocr_ctc_loss_grad", xd.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
              nll.data_ptr(), dl.data_ptr(), ws.data_ptr(), T, B, V, int(mll), None)
    torch.cuda.synchronize()
    return nll.cpu(), dl.cpu()


def kernel_of(mll):
    return "64" if mll <= 31 else "128" if mll <= 63 else "generic"


def forced(lmax):
    """the max_label_len values that send a batch with longest labelling lmax through every kernel that admits it"""
    return [lmax] + [m for m in (40, 70) if kernel_of(m) != kernel_of(lmax) and m > lmax]


def check_exact(nll, grad, ref, act):
    """no NaN, +-inf where and only where the reference has it, rows t >= act_len exactly 0"""
    assert not torch.isnan(nll).any() and not torch.isnan(grad).any()
    assert torch.equal(torch.isinf(nll), torch.isinf(ref.nll)) and bool((nll[torch.isinf(nll)] > 0).all())
    assert torch.isfinite(grad).all()
    for b, tb in enumerate(act):
        assert not grad[tb:, b].any(), "line %d: gradient rows past act_len are not zero" % b
    empty = [b for b, tb in enumerate(act) if tb == 0]
    for b in empty:
        assert float(nll[b]) == float(ref.nll[b])


_HEADER = False


def report(name, regime, mll, x, ll, ref, nll, grad, n32, g32):
    global _HEADER
    if not _HEADER:
        print("\n%-17s %-12s %-7s %5s %3s %5s %4s %9s | %9s %9s %6s %6s | %9s %9s %6s %6s" % (
            "case", "regime", "kernel", "T", "B", "V", "Lmax", "max nll", "e_k nll", "e_32 nll", "k/bar", "32/bar", "e_k grad", "e_32 grad",
            "k/bar", "32/bar"))
        _HEADER = True
    fin = ref.nll[torch.isfinite(ref.nll)]
    rk_n, rk_g = cr.ratio(nll, ref.nll, ref.nll_bar), cr.ratio(grad, ref.grad, ref.grad_bar)
    r32_n, r32_g = cr.ratio(n32, ref.nll, ref.nll_bar), cr.ratio(g32, ref.grad, ref.grad_bar)
    print("%-17s %-12s %-7s %5d %3d %5d %4d %9.3f | %9.2e %9.2e %6.3f %6.3f | %9.2e %9.2e %6.3f %6.3f" % (
        name, cr.regime_name(regime), kernel_of(mll), *x.shape, max(ll), float(fin.max()) if fin.numel() else 0.0,
        cr.max_err(nll, ref.nll), cr.max_err(n32, ref.nll), rk_n, r32_n, cr.max_err(grad, ref.grad), cr.max_err(g32, ref.grad), rk_g, r32_g))
    return rk_n, rk_g


@pytest.mark.parametrize("name,regime", list(cr.all_cases()), ids=lambda v: v if isinstance(v, str) else cr.regime_name(v))
def test_loss_and_gradient_against_fp64(name, regime):
    x, flat, ll, act, labs = cr.build_case(name, regime)
    T, B, V = x.shape
    ref = cr.Reference(x, flat, ll, act)
    n32, g32, _, _ = cr.ctc(x, flat, ll, act, torch.float32)
    mlls = forced(max(ll))
    nll, grad = raw_ctc(x, flat, ll, act, mlls[0], fill=float("nan"))
    rk_n, rk_g = report(name, regime, mlls[0], x, ll, ref, nll, grad, n32, g32)
    check_exact(nll, grad, ref, act)
    assert rk_n <= 1.0, "per-line nll misses its bar: %.3g of it" % rk_n
    assert rk_g <= 1.0, "a gradient element misses its bar: %.3g of it" % rk_g
    if name.startswith("tight"):
        for b in range(B // 2):                                          # one feasible path: the closed form, no restatement involved
            assert act[b] == cr.need(labs[b])
            cn, cg = cr.tight_closed_form(x[:, b], labs[b], act[b])
            assert abs(float(nll[b]) - float(cn)) <= float(ref.nll_bar[b])
            assert bool(((grad[:act[b], b].double() - cg).abs() <= ref.grad_bar[:act[b], b]).all())
    # the same batch through the other kernels: the same bits (ctc.hip's claim), whatever an earlier call left in the workspace
    for m in mlls[1:]:
        n2, g2 = raw_ctc(x, flat, ll, act, m, fill=-3.0)
        assert torch.equal(n2, nll), "nll of the %s kernel differs from the %s kernel's" % (kernel_of(m), kernel_of(mlls[0]))
        assert torch.equal(g2, grad), "dlogits of the %s kernel differ from the %s kernel's" % (kernel_of(m), kernel_of(mlls[0]))


def test_every_kernel_is_reached():
    """the case list sends batches through all three kernels, natively and forced"""
    seen = set()
    for spec in cr.GPU_CASES:
        seen.update(kernel_of(m) for m in forced(max(spec[4])))
    assert seen == {"64", "128", "generic"}
    assert forced(31) == [31, 40, 70] and forced(32) == [32, 70] and forced(63) == [63, 70] and forced(64) == [64] and forced(0) == [0, 40, 70]


@pytest.mark.parametrize("name,before", [("bench_ragged", "c4_ragged"), ("mix_generic", "generic_long"), ("c4_ragged", "generic_long")])
def test_result_does_not_depend_on_the_workspace(name, before):
    """rows t >= act_len of the alpha / beta workspace are never written: a ragged case gives the same bits in a fresh workspace full of
    NaN, in a workspace that a different case (a larger one for the first two) has just used, and once more after another one"""
    x, flat, ll, act, _ = cr.build_case(name, cr.PEAKY8)
    T, B, V = x.shape
    mll = max(ll)
    big = cr.build_case(before, cr.DENSE)
    other = cr.build_case("patterns_generic", cr.DENSE)
    from vistaocr_amd import _lib
    lib = _lib.load()
    sizes = [lib.vocr_ctc_workspace_bytes(*c[0].shape, max(c[2])) for c in (big, other)] + [lib.vocr_ctc_workspace_bytes(T, B, V, mll)]
    ws = torch.empty(max(sizes) // 4 + 4, dtype=torch.float32, device="cuda")
    ws.fill_(float("inf"))
    first = raw_ctc(x, flat, ll, act, mll, fill=float("nan"))
    raw_ctc(big[0], big[1], big[2], big[3], max(big[2]), ws=ws)
    second = raw_ctc(x, flat, ll, act, mll, ws=ws)
    raw_ctc(other[0], other[1], other[2], other[3], max(other[2]), ws=ws)
    third = raw_ctc(x, flat, ll, act, mll, ws=ws)
    for got in (second, third):
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])
    assert min(act) < T
    for b, tb in enumerate(act):
        assert not first[1][tb:, b].any()


def colsum_order(v):
    """vocr_colsum of an [m, 1] column in fp32, in the kernel's fixed order (gemm.hip: row splits of <= 32 rows' worth of work, four waves
    striding the rows by 4 with two accumulators each, a pairwise join, the splits added in order)"""
    v = np.asarray(v, dtype=np.float32)
    m = len(v)
    splits = max(1, min(64, -(-m // 32)))
    rps = -(-m // splits)
    total = None
    for r0 in range(0, m, rps):
        r1 = min(m, r0 + rps)
        red = []
        for w in range(4):
            s0 = s1 = np.float32(0)
            i = r0 + w
            while i + 4 < r1:
                s0 = np.float32(s0 + v[i])
                s1 = np.float32(s1 + v[i + 4])
                i += 8
            if i < r1:
                s0 = np.float32(s0 + v[i])
            red.append(np.float32(s0 + s1))
        part = np.float32(np.float32(red[0] + red[1]) + np.float32(red[2] + red[3]))
        total = part if total is None else np.float32(total + part)
    return total


@pytest.mark.parametrize("name,regime", [("bench_ragged", cr.PEAKY8), ("c4_ragged", cr.PEAKY8), ("patterns_generic", cr.DENSE), ("V257", cr.DENSE),
                                         ("B70", cr.PEAKY8), ("empty_all", cr.DENSE)],
                         ids=lambda v: v if isinstance(v, str) else cr.regime_name(v))
def test_ctcloss_batch_sum_and_autograd_scaling(name, regime):
    """CTCLoss / ops.CtcFn: the batch sum is the fixed-order fp32 sum of the raw per-line values, an upstream gradient of 0.37 scales the
    raw gradient by one fp32 product (vocr_scale_dev), and two runs give the same bits"""
    from vistaocr_amd import CTCLoss
    x, flat, ll, act, _ = cr.build_case(name, regime)
    nll, grad = raw_ctc(x, flat, ll, act, max(ll))
    assert torch.isfinite(nll).all()
    runs = []
    for _ in range(2):
        lg = x.clone().cuda().requires_grad_(True)
        loss = CTCLoss()(lg, flat[:sum(ll)], torch.tensor(act, dtype=torch.int32), torch.tensor(ll, dtype=torch.int32))
        assert tuple(loss.shape) == (1,)
        (0.37 * loss).backward()
        runs.append((loss.detach().cpu(), lg.grad.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    loss, g = runs[0]
    assert np.float32(loss.numpy()[0]) == colsum_order(nll.numpy()), (float(loss), float(colsum_order(nll.numpy())))
    want = grad.double() * float(np.float32(0.37))
    assert bool(((g.double() - want).abs() <= cr.ulp32(want) + 2.0 ** -126).all())         # 2^-126: a flushed subnormal product


# ------------------------------------------------------------------------------------------------------------------ greedy decode
def host_collapse(idx, mx, lens, canon, thresh):
    """decode_without_lm's rules on host arrays: a blank resets, a maximum below the threshold (fp32 comparison) resets, repeats collapse
    by their canonical class, the emitted label is the argmax index itself; lens are clamped to T"""
    T, B = idx.shape
    thresh = np.float32(thresh)
    out = []
    for b in range(B):
        prev, row = -1, []
        for t in range(min(int(lens[b]), T)):
            k = int(idx[t, b])
            if k == 0 or np.float32(mx[t, b]) < thresh:
                prev = -1
                continue
            if int(canon[k]) == prev:
                continue
            row.append(k)
            prev = int(canon[k])
        out.append(row)
    return out


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("B", [1, 65])
def test_argmax_rows_exact(V, B):
    from vistaocr_amd import ops
    T = 23                                                                   # T * B = 23, 1495: not multiples of the 4 rows of a block
    rng = np.random.default_rng(V * 1000 + B)
    x = rng.normal(0, 1, (T, B, V)).astype(np.float32)
    x[1, 0, :] = 0.25                                                        # an all-equal row: index 0
    if V > 11:
        x[2, 0, 10] = x[2, 0, 11] = 5.0                                      # a tie across neighbouring lanes
        x[3, 0, 11] = x[3, 0, 10] = -0.0
        x[3, 0, :10] = -1.0
        x[3, 0, 12:] = -1.0                                                  # the maximum is -0.0 twice
    if V > 74:
        x[4, 0, 10] = x[4, 0, 74] = 5.0                                      # a tie inside one lane's stride (columns 10 and 74)
        x[5, 0, 74] = x[5, 0, 75] = x[5, 0, 200] = 6.0
    x[6, B - 1, V - 1] = 9.0                                                 # the last column of the last line
    idx, mx = ops.argmax_rows(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (T, B)
    assert np.array_equal(idx.cpu().numpy(), np.argmax(x, 2).astype(np.int32))          # numpy: the first maximum
    assert np.array_equal(mx.cpu().numpy(), np.max(x, 2))


@pytest.mark.parametrize("B", [1, 65, 130])
def test_greedy_collapse_exact(B):
    """one thread per line, 64 per block: B = 1, 65 and 130 end inside the first, second and third block"""
    from vistaocr_amd import ops
    T, V = 40, 96
    rng = np.random.default_rng(B)
    thresh = np.float32(3 * 1 / V)
    below, above = np.nextafter(thresh, np.float32(0)), np.nextafter(thresh, np.float32(1))
    # few classes, so that blanks, repeats and merged classes are frequent: canon merges 5 into 3 and 9 into 2
    canon = np.arange(V, dtype=np.int32)
    canon[5], canon[9] = 3, 2
    idx = rng.choice(np.array([0, 2, 3, 5, 9, V - 1], dtype=np.int32), size=(T, B))
    mx = rng.choice(np.array([thresh, below, above, 0.5, -1.0], dtype=np.float32), size=(T, B), p=[0.2, 0.2, 0.2, 0.3, 0.1])
    idx[:6, 0] = [3, 3, 5, 3, 0, 3]
    mx[:6, 0] = [thresh, above, 0.5, below, 0.5, thresh]                     # 3 (3 5 merged) | below: reset | blank | 3
    lens = rng.integers(0, T + 1, B).astype(np.int32)
    lens[0] = T
    lens[B - 1] = T + 7                                                      # greater than T: clamped
    if B > 3:
        lens[1], lens[2], lens[3] = 0, 1, T
    want = host_collapse(idx, mx, lens, canon, thresh)
    assert want[0][:2] == [3, 3]
    labels, counts = ops.greedy_collapse(torch.from_numpy(idx).cuda(), torch.from_numpy(mx).cuda(), torch.from_numpy(lens).cuda(),
                                         torch.from_numpy(canon).cuda(), thresh)
    torch.cuda.synchronize()
    labels, counts = labels.cpu().numpy(), counts.cpu().numpy()
    assert counts.tolist() == [len(r) for r in want]
    for b in range(B):
        assert labels[b, :counts[b]].tolist() == want[b], b
        assert not labels[b, counts[b]:].any()


def test_argmax_feeds_collapse_at_the_threshold():
    """end to end on logits: a frame maximum exactly at the threshold is kept, one fp32 ulp below it resets, one above is kept"""
    from vistaocr_amd import ops
    T, B, V = 9, 2, 64
    thresh = np.float32(3 * 1 / V)
    below, above = np.nextafter(thresh, np.float32(0)), np.nextafter(thresh, np.float32(1))
    x = np.full((T, B, V), -2.0, dtype=np.float32)
    seq = [(7, thresh), (7, below), (7, above), (0, 0.5), (7, thresh), (8, above), (8, below), (8, 0.5), (63, thresh)]
    for t, (k, v) in enumerate(seq):
        x[t, :, k] = v
    idx, mx = ops.argmax_rows(torch.from_numpy(x).cuda())
    lens = np.array([T, 5], dtype=np.int32)
    canon = np.arange(V, dtype=np.int32)
    labels, counts = ops.greedy_collapse(idx, mx, torch.from_numpy(lens).cuda(), torch.from_numpy(canon).cuda(), thresh)
    torch.cuda.synchronize()
    want = host_collapse(idx.cpu().numpy(), mx.cpu().numpy(), lens, canon, thresh)
    assert want == [[7, 7, 7, 8, 8, 63], [7, 7, 7]]
    got = [labels[b, :int(counts[b])].cpu().tolist() for b in range(B)]
    assert got == want
