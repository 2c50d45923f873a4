"""GPU: the CTC entry points that score KNOWN labellings and queries, each called on the C entry (_lib.call) in memory the test owns to
the byte (tests/guarded.py, tests/ctc_guarded.py): vocr_ctc_loss_grad, vocr_ctc_align, vocr_ctc_edit_scores, vocr_ctc_nbest_grad,
vocr_ctc_entropy, vocr_ctc_keyword_scores.  tests/test_ctc_guarded_search_gpu.py does the same for the two beam searches, the grammar
entries and vocr_edit_stats.

Every case holds, of ONE call:
  accuracy      the answer of that entry's own fp64 restatement at that entry's own suite's bar (imported, never copied);
  written       every element of every output holds what include/vocr.h names for it - outputs start poisoned (NaN; integers 0xA5A5A5A5)
                and none of it may survive, the elements no path reaches included (spans -1 and label scores 0 at p >= L, -inf at
                p >= L / q > L of the edit scores, zero gradient rows past lens and on unscorable lines, {-1, -1} spans of invalid queries);
  no stale read the workspace starts as NaN and so do the bands round logits, weights and coeff: no NaN may appear in any output;
  guards        both bands of every operand and output and the band behind a workspace of exactly *_workspace_bytes(...) bytes are bit
                for bit as they were; label and query rows hold V, one past the alphabet, in every slot past their own length and in
                every column past max_label_len (label_stride = max_label_len + 3 everywhere);
  repeatable    a second call into fresh poisoned buffers gives the same bits;
  wrapper       the ops.* wrapper the product calls returns the same bits (values only: it allocates its own buffers);
  refusal       entries that take workspace_bytes are called with a truly smaller workspace, 16 bytes short, and its true size: the call
                fails with VOCR_EINVAL, every output is still fully poisoned, the workspace and every band untouched.
vocr_ctc_loss_grad takes no workspace_bytes: no refusal case.

entry                     branch of the host plan                                           case that takes it
vocr_ctc_loss_grad        sp = 64: one register per lane (longest label 31)                 L31 (dlogits given), L31_nograd (dlogits NULL)
                          sp = 128: two registers (32)                                      L32
                          sp = 192: the LDS kernel (64)                                     L64, L64_nograd
                          label_lens 0 and act_lens < T in every batch; V = 2 / 256         all of them; V2, V256
                          asserted: the workspace is (T B V + 2 B T sp) floats, sp from the case
vocr_ctc_align            S <= 64 (no rows, back pointers in LDS)                           T15, T16, T17 (M <= 6), T1, V2, V256
                          S > 64, rows and back pointers in LDS                             seams (M = 36: sp = 128, T = 72)
                          back pointers in the workspace: rows 28176 B + 800 * 10 * 16 B    bp_ws (T = 800, 300 labels, B = n = 1, V = 4)
                          = 156176 B > the 147456 B budget
                          rows in the workspace too: 1664 labels > 1663                     rows_ws (T = 1700, 1664 labels, B = n = 1, V = 4)
                          n = 1 / n = 3; label_stride > max_label_len                       bp_ws, rows_ws / the others; every case
                          asserted: workspace bytes = clp, + B n T (sp / 64) 16, + B n rows_floats 4 - the header's three terms
vocr_ctc_edit_scores,     labellings of 31 / 32 / 33 labels in one batch (register / LDS    seams
vocr_ctc_nbest_grad,      sweep of ctc_lattice.h)
vocr_ctc_entropy          T = 15 / 16 / 17 (16-frame tiles of the gradient kernels), T = 1  T15, T16, T17, T1
                          line lengths 0, 1, 8, 9 in one batch (PF = TB = 8)                T15 (15, 0, 1, 8 and 9 in T16 / T17)
                          with and without the gradient operand; a scores-only call         every case runs both; asserted: the entropy's
                          reports and gets the smaller workspace                            want_grad = 0 size and the n-best scores-only
                                                                                            size are the class log-probabilities alone
                          a class with a -inf member (canon)                                T16
                          an invalid labelling / one that does not fit / L = 0 /            T15, T17, V256 / T16, lens of 0 and 1 / every
                          an unfilled rank (label_lens -1)                                  case / T17, T1
                          V = 2 / V = 256                                                   V2 / V256
vocr_ctc_keyword_scores   query lengths 1, 8, 9, 16, 17 in one call (4 / 2 / 1 per wave)    mixed
                          nq = 7: an integer section of (16 + 14) * 4 = 120 B, no           mixed, flags
                          multiple of 16
                          query_flags NULL / given with an anchored and a trimmed query     mixed / flags
                          an invalid query between valid ones                               mixed ([V] and a too long one), flags (a trimmed
                                                                                            query of one label)
                          V = 2 / V = 256, lens 0 and lens > T                              V2 / V256
Run with -s for the table (profiles/ctc_guarded_errors.txt keeps it)."""
import time

import numpy as np
import pytest
import torch

from tests import align_ref as ar
from tests import ctc_guarded as cg
from tests import ctc_ref as cr
from tests import entropy_ref as enr
from tests import guarded as gd
from tests import kws_ref as kr
from tests import nbest_ref as nr
from tests.beam_data import dense_logits

pytestmark = pytest.mark.gpu
NEG = float("-inf")
PEAKY, DENSE = ("peaky", 8.0, 1.0), ("beam_dense", 3.0)
CANON9 = [0, 1, 1, 3, 4, 4, 4, 7, 8]          # tests/nbest_cases.py: classes of 2 ({1, 2}) and 3 ({4, 5, 6}) members; V >= 9
I32, F32 = torch.int32, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _table():
    cg.T0[0] = time.time()
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)
    cg.print_table("ctc-guarded: known labellings and queries")


def _i32(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int32))


def _align16(n):
    return (n + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------------------- vocr_ctc_loss_grad
# name, T, V, label counts (B = 4: the longest, none, two short ones), act_lens, regime, with dlogits
LOSS_CASES = [
    ("L31", 72, 8, [31, 0, 5, 12], [72, 72, 40, 9], cr.PEAKY8, True),
    ("L31_nograd", 72, 8, [31, 0, 5, 12], [72, 72, 40, 9], cr.PEAKY8, False),
    ("L32", 72, 8, [32, 0, 5, 3], [72, 70, 1, 0], cr.DENSE, True),
    ("L64", 136, 6, [64, 0, 33, 7], [136, 135, 50, 17], cr.PEAKY8, True),         # line 2: 33 labels in 50 frames, line 3 fits
    ("L64_nograd", 136, 6, [64, 0, 33, 7], [136, 135, 50, 17], cr.DENSE, False),
    ("V2", 24, 2, [5, 0, 1, 2], [24, 17, 9, 2], cr.DENSE, True),                   # line 3: two equal labels need 3 frames: +inf
    ("V256", 20, 256, [6, 0, 4, 1], [20, 13, 20, 1], cr.PEAKY8, True),
]


@pytest.mark.parametrize("name", [c[0] for c in LOSS_CASES])
def test_ctc_loss_grad(name):
    from tests.test_ctc_fp64_gpu import check_exact
    from vistaocr_amd import _lib, ops
    _, T, V, ls, act, regime, with_grad = [c for c in LOSS_CASES if c[0] == name][0]
    B = len(ls)
    rng = np.random.default_rng([41, [c[0] for c in LOSS_CASES].index(name)])
    labs = [cr.make_labels(rng, V, L, "random") for L in ls]
    fit = [l if cr.need(l) <= act[b] else [] for b, l in enumerate(labs)]
    x = cr.build_logits(rng, T, B, V, fit, act, regime)
    flat = torch.tensor([v for l in labs for v in l], dtype=I32)
    off = np.concatenate([[0], np.cumsum(ls)[:-1]])
    mll = max(ls)
    sp = (2 * mll + 1 + 63) // 64 * 64
    assert sp == {31: 64, 32: 128, 64: 192}.get(mll, 64)
    nbytes = _lib.load().vocr_ctc_workspace_bytes(T, B, V, mll)
    assert nbytes == (T * B * V + 2 * B * T * sp) * 4                           # the kernel is picked from sp alone: the documented rows
    ins = dict(x=x, labels=(flat, V), off=(_i32(off), 0), ll=(_i32(ls), 0), act=(_i32(act), 0))
    outs = dict(nll=((B,), F32), dl=((T, B, V), F32) if with_grad else None)
    args = lambda p, ws, n: (p["x"], p["labels"], p["off"], p["ll"], p["act"], p["nll"], p["dl"], ws, T, B, V, mll, ops._stream())
    run = cg.guarded_runs("vocr_ctc_loss_grad", name, ins, outs, nbytes, args, takes_size=False)
    ref = cr.Reference(x, flat, ls, act)
    nll = run.out("nll").cpu()
    rn = cr.ratio(nll, ref.nll, ref.nll_bar)
    rg = 0.0
    if with_grad:
        grad = run.out("dl").cpu()
        check_exact(nll, grad, ref, act)
        rg = cr.ratio(grad, ref.grad, ref.grad_bar)
    else:
        assert not torch.isnan(nll).any() and torch.equal(torch.isinf(nll), torch.isinf(ref.nll))
    cg.row("vocr_ctc_loss_grad", name, "sp %d, dlogits %s" % (sp, "given" if with_grad else "NULL"), max(rn, rg), nbytes)
    assert rn <= 1.0 and rg <= 1.0, (name, rn, rg)
    # the wrapper: the criterion's batch sum and, through autograd at dloss = 1, the same gradient bits
    d = lambda a: a.to("cuda")
    xd = d(x).requires_grad_(True)
    loss = ops.CtcFn.apply(xd, d(flat), d(_i32(off)), d(_i32(ls)), d(_i32(act)), mll)
    assert cg.same_bits(loss.detach().reshape(-1), ops.colsum(run.out("nll").reshape(B, 1).clone()).reshape(-1)), name
    if with_grad and bool(torch.isfinite(ref.nll).all()):
        loss.backward()
        assert cg.same_bits(xd.grad, run.out("dl")), name


# ------------------------------------------------------------------------------------- the entries over labellings [B][n][label_stride]
def _labelling_case(name):
    """dict(x fp32 [T,B,V], lens, hyps[b][q] (label list or None), canon, M, w [B,n], T, B, V, n, family): data only.  Every line has a
    base labelling (rank 0) and n - 1 one-edit neighbours of it (tests/nbest_cases.py's recipe); `special` then replaces single ranks."""
    from tests.nbest_cases import _edit
    spec = [c for c in LABELLING_CASES if c[0] == name][0]
    _, T, V, n, ls, lens, regime, canon, special, family = spec
    B = len(ls)
    rng = np.random.default_rng([43, [c[0] for c in LABELLING_CASES].index(name)])
    canon = CANON9 + list(range(9, V)) if canon else None
    allowed = [v for v in range(1, V) if canon is None or canon[v] != 0]
    base = [cr.make_labels(rng, V, L, "random") for L in ls]
    if regime[0] == "beam_dense":
        x = torch.from_numpy(dense_logits(rng, T, B, V, regime[1]))
    else:
        x = cr.build_logits(rng, T, B, V, [l if cr.need(l) <= lens[b] else [] for b, l in enumerate(base)], lens, regime)
    hyps = [[list(base[b])] + [_edit(rng, base[b], allowed) for _ in range(n - 1)] for b in range(B)]
    hyps = [[h if len(h) <= T else list(base[b]) for h in row] for b, row in enumerate(hyps)]       # max_label_len <= T
    M = max(max(len(h) for h in row) for row in hyps)
    for (b, q), h in special.items():
        if h == "nofit":                                      # one repeated label: k of them take 2k - 1 frames, more than the line has
            h = [allowed[0]] * min(lens[b] // 2 + 2, T)
            assert 2 * len(h) - 1 > lens[b]
        elif h == "big":
            h = [V] + hyps[b][q][1:]
        hyps[b][q] = h
    M = max([M, 1] + [len(h) for row in hyps for h in row if h is not None])
    assert M <= T
    if canon is not None:                                     # one member of the 3-class at -inf everywhere, one of the 2-class on line 0
        x[:, :, 5] = NEG
        x[:, 0, 2] = NEG
    w = rng.normal(0, 1, (B, n)).astype(np.float32).astype(np.float64)
    return dict(name=name, x=x, lens=lens, hyps=hyps, canon=canon, M=M, w=w, T=T, B=B, V=V, n=n, family=family)


# name, T, V, n, base label counts, lens, regime, classes, {(line, rank): None | [labels] | "nofit" | "big"}, the entropy suite's family
LABELLING_CASES = [
    ("seams", 72, 8, 3, [31, 32, 33, 0], [72, 72, 72, 9], PEAKY, False, {(1, 2): [1, 2, 3] * 12}, "seam_peaky"),
    ("T15", 15, 12, 3, [4, 0, 1, 3], [15, 0, 1, 8], PEAKY, False, {(0, 1): "big", (2, 2): [0]}, "lens"),
    ("T16", 16, 12, 3, [4, 3, 2, 1], [16, 9, 8, 1], DENSE, True, {(1, 0): "nofit", (0, 2): []}, "classes"),
    ("T17", 17, 12, 3, [5, 3, 0, 2], [17, 0, 9, 16], DENSE, False, {(0, 1): None, (3, 0): "big", (2, 1): None}, "lens"),
    # T = 1: logits N(0, 0.5).  The edit and alignment suites' eps_line(T, score) = 4 T 2^-24 max(|score|, 1) is 2.4e-7 at T = 1, and
    # x - lse alone rounds at ulp32(|x| + |lse|) / 2 twice: within that bar while |x| + |lse| < 4, which N(0, 3) logits are not
    ("T1", 1, 5, 3, [1, 0, 1, 1], [1, 1, 1, 0], ("beam_dense", 0.5), False, {(0, 2): None, (2, 1): []}, "lens"),
    ("V2", 24, 2, 3, [5, 1, 0], [24, 17, 9], DENSE, False, {}, "V"),
    ("V256", 20, 256, 3, [6, 4], [20, 13], DENSE, False, {(1, 0): "big"}, "V"),
]
_cases = {}


def _case(name):
    if name not in _cases:
        k = _labelling_case(name)
        k["stride"] = k["M"] + 3
        k["labels"], k["label_lens"] = gd.pack_labels(k["hyps"], k["stride"], k["V"])
        k["lens_t"] = _i32(k["lens"])
        k["canon_t"] = None if k["canon"] is None else _i32(k["canon"])
        _cases[name] = k
    return _cases[name]


def _labelling_ins(k, **more):
    ins = dict(x=k["x"], lens=(k["lens_t"], 0), canon=None if k["canon_t"] is None else (k["canon_t"], 0),
               labels=(k["labels"], k["V"]), label_lens=(k["label_lens"], 0))
    ins.update(more)
    return ins


def _wrapper_args(k):
    d = lambda t: None if t is None else t.to("cuda")
    return d(k["x"]), d(k["lens_t"]), d(k["labels"][:, :, :k["M"]].contiguous()), d(k["label_lens"]), d(k["canon_t"])


def _clp_bytes(k):
    return _align16(k["T"] * k["B"] * k["V"] * 4)


LABELLING_NAMES = [c[0] for c in LABELLING_CASES]
ALIGN_LONG = {"bp_ws": (800, 300), "rows_ws": (1700, 1664)}


def _align_long_case(name):
    """B = n = 1, V = 4, one peaky line with its labelling 1 2 3 1 2 3 ...: a single wave over T frames"""
    T, L = ALIGN_LONG[name]
    rng = np.random.default_rng([47, L])
    lab = [1 + i % 3 for i in range(L)]
    x = cr.build_logits(rng, T, 1, 4, [lab], [T], PEAKY)
    k = dict(name=name, x=x, lens=[T], hyps=[[lab]], canon=None, M=L, T=T, B=1, V=4, n=1, stride=L + 3)
    k["labels"], k["label_lens"] = gd.pack_labels(k["hyps"], k["stride"], 4)
    k["lens_t"], k["canon_t"] = _i32([T]), None
    return k


@pytest.mark.parametrize("name", LABELLING_NAMES + sorted(ALIGN_LONG))
def test_ctc_align(name):
    from tests.test_align_gpu import _check_line
    from vistaocr_amd import _lib, ops
    k = _align_long_case(name) if name in ALIGN_LONG else _case(name)
    T, B, V, n, M, stride = k["T"], k["B"], k["V"], k["n"], k["M"], k["stride"]
    nbytes = _lib.load().vocr_ctc_align_workspace_bytes(T, B, V, n, M)
    sp = (2 * M + 1 + 63) // 64 * 64
    rows_floats = 0 if sp <= 64 else (2 * (sp + 2) + sp + 8 * sp + 3) // 4 * 4        # ctc_lattice.h: sweep_floats(sp, 2), 16-byte rounded
    bp = B * n * T * (sp // 64) * 16
    if name == "rows_ws":
        branch, want = "rows and back pointers in the workspace", _clp_bytes(k) + bp + B * n * rows_floats * 4
    elif name == "bp_ws":
        branch, want = "S > 64, rows in LDS, back pointers in the workspace", _clp_bytes(k) + bp
    else:
        branch, want = ("S > 64, rows and back pointers in LDS" if sp > 64 else "S <= 64"), _clp_bytes(k)
    assert nbytes == want, (name, nbytes, want)
    assert (sp > 64) == (name in ("seams", "bp_ws", "rows_ws"))
    outs = dict(scores=((B, n, 2), F32), spans=((B, n, M, 2), I32), label_scores=((B, n, M, 2), F32))
    args = lambda p, ws, nb: (p["x"], p["lens"], T, B, V, p["canon"], p["labels"], p["label_lens"], n, stride, M, p["scores"], p["spans"],
                              p["label_scores"], ws, nb, ops._stream())
    run = cg.guarded_runs("vocr_ctc_align", name, _labelling_ins(k), outs, nbytes, args)
    sc, sp_, ls = run.host("scores"), run.host("spans"), run.host("label_scores")
    xn = k["x"].numpy()
    used, frac = 0, 0.0
    for b in range(B):
        for q in range(n):
            h = k["hyps"][b][q]
            ok = h is not None and len(h) <= M
            ref = ar.align(xn[:, b], k["lens"][b], h, k["canon"]) if ok else ar._none()
            used += _check_line((sc[b, q], sp_[b, q], ls[b, q]), ref, len(h) if ok else 0, T, 1e-3, (name, b, q))
            if ref.spans is not None:
                frac = max(frac, abs(sc[b, q, 0] - ref.viterbi) / 1e-3, abs(sc[b, q, 1] - ref.ctc) / 1e-3)
    if name in ALIGN_LONG:
        assert used == 1, name                                                  # the reference decides the path: identical spans
    cg.row("vocr_ctc_align", name, branch, frac, nbytes)
    got = ops.ctc_align(*_wrapper_args(k))
    assert all(cg.same_bits(g, run.out(o)) for g, o in zip(got, ("scores", "spans", "label_scores"))), name


@pytest.mark.parametrize("name", LABELLING_NAMES)
def test_ctc_edit_scores(name):
    from tests.test_edit_gpu import _check, _expected
    from vistaocr_amd import _lib, ops
    k = _case(name)
    T, B, V, n, M, stride = k["T"], k["B"], k["V"], k["n"], k["M"], k["stride"]
    nbytes = _lib.load().vocr_ctc_edit_workspace_bytes(T, B, V, n, M)
    assert nbytes == _clp_bytes(k) + B * n * 8 * T * (2 * M + 1)               # the header's two terms: class log-probabilities, lattices
    outs = dict(ctc=((B, n), F32), sub=((B, n, M, V), F32), dele=((B, n, M), F32), ins=((B, n, M + 1, V), F32))
    args = lambda p, ws, nb: (p["x"], p["lens"], T, B, V, p["canon"], p["labels"], p["label_lens"], n, stride, M, p["ctc"], p["sub"],
                              p["dele"], p["ins"], ws, nb, ops._stream())
    run = cg.guarded_runs("vocr_ctc_edit_scores", name, _labelling_ins(k), outs, nbytes, args)
    got = [run.host(o) for o in ("ctc", "sub", "dele", "ins")]
    _, frac = _check(got, _expected(k["x"].numpy(), k["lens"], k["hyps"], k["canon"], M), T, "guarded " + name)
    cg.row("vocr_ctc_edit_scores", name, "longest S %d: %s sweep" % (2 * M + 1, "LDS" if 2 * M + 1 > 64 else "register"), frac, nbytes)
    wr = ops.ctc_edit_scores(*_wrapper_args(k))
    assert all(cg.same_bits(g, run.out(o)) for g, o in zip(wr, ("ctc", "sub", "dele", "ins"))), name


@pytest.mark.parametrize("name", LABELLING_NAMES)
def test_ctc_nbest_grad(name):
    from tests.test_nbest_gpu import _check
    from vistaocr_amd import _lib, ops
    k = _case(name)
    T, B, V, n, M, stride = k["T"], k["B"], k["V"], k["n"], k["M"], k["stride"]
    nbytes = _lib.load().vocr_ctc_nbest_workspace_bytes(T, B, V, n, M)
    assert nbytes == _clp_bytes(k) + B * n * 8 * T * (2 * M + 1)
    w = torch.from_numpy(k["w"].astype(np.float32))
    args = lambda p, ws, nb: (p["x"], p["lens"], T, B, V, p["canon"], p["labels"], p["label_lens"], n, stride, M, p.get("w"), p["ctc"],
                              p["dl"], ws, nb, ops._stream())
    run = cg.guarded_runs("vocr_ctc_nbest_grad", name, _labelling_ins(k, w=w), dict(ctc=((B, n), F32), dl=((T, B, V), F32)), nbytes, args)
    ref = nr.Reference(k["x"], k["lens"], k["hyps"], k["canon"], k["w"], M)
    sfrac, gfrac = _check(name, T, run.out("ctc"), run.out("dl"), ref, k["lens"])
    cg.row("vocr_ctc_nbest_grad", name, "with weights: class log-probabilities + lattices", max(sfrac, gfrac), nbytes)
    assert sfrac <= 1.0 and gfrac <= 1.0, (name, sfrac, gfrac)
    # scores only: the class log-probabilities alone are used, and checked for
    only = cg.guarded_runs("vocr_ctc_nbest_grad", name, _labelling_ins(k), dict(ctc=((B, n), F32), dl=None), _clp_bytes(k), args)
    assert cg.same_bits(only.out("ctc"), run.out("ctc")), name
    cg.row("vocr_ctc_nbest_grad", name, "scores only: class log-probabilities alone", sfrac, _clp_bytes(k))
    wa = _wrapper_args(k)
    s3, g3 = ops.ctc_nbest(*wa, w.to("cuda"))
    assert cg.same_bits(s3, run.out("ctc")) and cg.same_bits(g3, run.out("dl")), name
    s4, g4 = ops.ctc_nbest(*wa)
    assert g4 is None and cg.same_bits(s4, run.out("ctc")), name


@pytest.mark.parametrize("name", LABELLING_NAMES)
def test_ctc_entropy(name):
    from tests.test_entropy_gpu import TOL, _errors
    from vistaocr_amd import _lib, ops
    k = _case(name)
    T, B, V, M, stride = k["T"], k["B"], k["V"], k["M"], k["stride"]
    labs = [row[0] for row in k["hyps"]]                                        # rank 0 of every line: one labelling per line
    labels, label_lens = k["labels"][:, 0].contiguous(), k["label_lens"][:, 0].contiguous()
    coeff = np.stack([k["w"][:, 0], k["w"][:, 1]], 1)
    lib = _lib.load()
    nbytes, small = lib.vocr_ctc_entropy_workspace_bytes(T, B, V, M, 1), lib.vocr_ctc_entropy_workspace_bytes(T, B, V, M, 0)
    assert small == _clp_bytes(k) and nbytes == small + B * 16 * T * (2 * M + 1)      # the header's terms: the four lattices behind them
    ins = dict(x=k["x"], lens=(k["lens_t"], 0), canon=None if k["canon_t"] is None else (k["canon_t"], 0), labels=(labels, V),
               label_lens=(label_lens, 0))
    args = lambda p, ws, nb: (p["x"], p["lens"], T, B, V, p["canon"], p["labels"], p["label_lens"], stride, M, p.get("coeff"), p["ctc"],
                              p["ent"], p["dl"], ws, nb, ops._stream())
    outs = dict(ctc=((B,), F32), ent=((B,), F32), dl=((T, B, V), F32))
    run = cg.guarded_runs("vocr_ctc_entropy", name, dict(ins, coeff=torch.from_numpy(coeff.astype(np.float32))), outs, nbytes, args)
    ref = enr.entropy(k["x"].numpy(), k["lens"], labs, k["canon"], coeff, M)
    serr, gerr = _errors(name, T, k["lens"], run.out("ctc"), run.out("ent"), run.out("dl"), ref)
    tol_s, tol_g = TOL[k["family"]]
    cg.row("vocr_ctc_entropy", name, "with coeff (family %s)" % k["family"], max(serr / tol_s, gerr / tol_g), nbytes)
    assert serr <= tol_s and gerr <= tol_g, (name, k["family"], serr, gerr)
    only = cg.guarded_runs("vocr_ctc_entropy", name, ins, dict(outs, dl=None), small, args)
    assert cg.same_bits(only.out("ctc"), run.out("ctc")) and cg.same_bits(only.out("ent"), run.out("ent")), name
    cg.row("vocr_ctc_entropy", name, "scores only: the smaller workspace", serr / tol_s, small)
    d = lambda t: None if t is None else t.to("cuda")
    wa = (d(k["x"]), d(k["lens_t"]), d(labels[:, :M].contiguous()), d(label_lens), d(k["canon_t"]))
    c3, e3, g3 = ops.ctc_entropy(*wa, d(torch.from_numpy(coeff.astype(np.float32))))
    assert cg.same_bits(c3, run.out("ctc")) and cg.same_bits(e3, run.out("ent")) and cg.same_bits(g3, run.out("dl")), name
    c4, e4, g4 = ops.ctc_entropy(*wa)
    assert g4 is None and cg.same_bits(c4, run.out("ctc")) and cg.same_bits(e4, run.out("ent")), name


# ------------------------------------------------------------------------------------------------------ vocr_ctc_keyword_scores
def _kws_case(name):
    """(x numpy [T,B,V], lens, queries, flags or None, canon or None, max_query_len)"""
    from tests.test_kws_gpu import _lines, _queries_of_length
    if name in ("mixed", "flags"):
        T, V = 96, 12
        x = _lines(51, T, V, 2, 1)
        lens = [T, T - 7, 40]
        rng = np.random.default_rng(52)
        qs = [_queries_of_length(rng, x, lens, 2, V, L)[0] for L in (9, 1, 17, 8, 16)]
        assert [len(q) for q in qs] == [9, 1, 17, 8, 16]
        if name == "mixed":                                   # invalid between valid ones: a label V, and 18 labels where 17 is the limit
            qs = qs[:2] + [[V]] + qs[2:4] + [qs[2] + [1]] + qs[4:]
            return x, lens, qs, None, None, 17
        g0 = ar.greedy_labels(x[:, 0], T)
        qs = [g0[:9], qs[1], [3], g0[-8:], qs[3], qs[2], qs[4]]     # anchored at the start / a trimmed query of one label: invalid /
        return x, lens, qs, [1, 0, 4, 2, 12, 8, 3], None, 17        # anchored at the end / both trims / end trim / both anchors
    if name == "V2":
        x = np.random.default_rng(53).normal(0, 1, (12, 3, 2)).astype(np.float32)
        return x, [12, 0, 30], [[1], [1, 1], [1, 1, 1]], None, None, 3
    rng = np.random.default_rng(54)
    x = rng.normal(0, 1, (10, 2, 256)).astype(np.float32)
    x[:, :, 5] = NEG
    canon = CANON9 + list(range(9, 256))
    return x, [10, 99], [[255, 2], [4], [6, 1, 255], [200]], [0, 3, 0, 0], canon, 3


@pytest.mark.parametrize("name", ["mixed", "flags", "V2", "V256"])
def test_ctc_keyword_scores(name):
    from tests.test_kws_gpu import _check
    from vistaocr_amd import _lib, ops
    x, lens, qs, flags, canon, mq = _kws_case(name)
    T, B, V = x.shape
    nq, stride = len(qs), mq + 3
    queries, qlens = gd.pack_rows(qs, stride, V)
    nbytes = _lib.load().vocr_ctc_keyword_workspace_bytes(T, B, V, nq, mq)
    ints = (16 + 2 * nq) * 4
    assert nbytes == 2 * _align16(T * B * V * 4) + 2 * _align16(T * B * 4) + _align16(ints)
    if name in ("mixed", "flags"):
        assert nq == 7 and ints % 16 != 0
    ins = dict(x=torch.from_numpy(x), lens=(_i32(lens), 0), canon=None if canon is None else (_i32(canon), 0), queries=(queries, V),
               qlens=(qlens, 0), flags=None if flags is None else (_i32(flags), 0))
    outs = dict(lc=((B, nq), F32), best=((B, nq), F32), span=((B, nq, 2), I32))
    args = lambda p, ws, nb: (p["x"], p["lens"], T, B, V, p["canon"], p["queries"], p["qlens"], p["flags"], nq, stride, mq, p["lc"],
                              p["best"], p["span"], ws, nb, ops._stream())
    run = cg.guarded_runs("vocr_ctc_keyword_scores", name, ins, outs, nbytes, args)
    got = tuple(run.host(o) for o in ("lc", "best", "span"))
    ref = kr.search(x, lens, [q if len(q) <= mq else [0] for q in qs], flags, canon)      # longer than max_query_len: invalid
    _check("guarded kws " + name, x, lens, qs, flags, canon, got=got, ref=ref)
    fin = ref["log_count"] != -np.inf
    from tests.test_kws_gpu import bound
    frac = max([float((np.abs(g[f].astype(np.float64) - r[f]) / bound(T, r[f])).max()) for g, r, f in
                ((got[0], ref["log_count"], fin), (got[1], ref["best"], ref["best"] != -np.inf)) if f.any()] + [0.0])
    cg.row("vocr_ctc_keyword_scores", name, "nq %d, integer section %d B, flags %s" % (nq, ints, "NULL" if flags is None else "given"),
           frac, nbytes)
    dead = ~fin
    assert (got[2][dead] == -1).all(), name                                   # {-1, -1} for every pair without an occurrence
    d = lambda t: None if t is None else t.to("cuda")
    wr = ops.ctc_keyword_scores(d(torch.from_numpy(x)), lens, d(queries[:, :mq].contiguous()), d(qlens),
                                None if flags is None else d(_i32(flags)), None if canon is None else d(_i32(canon)))
    assert all(cg.same_bits(g, run.out(o)) for g, o in zip(wr, ("lc", "best", "span"))), name
