"""GPU: vocr_ctc_align (vistaocr_amd/csrc/ctc_align.hip) through ops.ctc_align, CtcAligner and the decoders' decode_aligned, against
brute force on exact cases, the fp64 restatement (tests/align_ref.py) on bench-shaped peaky and dense logits, the CTC loss kernel,
itself (determinism), and decode_dataset's word file.

Where spans are compared they must be IDENTICAL, on every line whose decision gap (align_ref) exceeds
    eps_line = 4 * T * 2^-24 * max(|viterbi_logp|, 1):
a linear worst-case bound on the fp32 rounding accumulated over T additions, on both competitors, with the log-softmax's share (the floor
of 1 covers the log-softmax's own rounding where the score is near 0).  "Greedy labels" are align_ref.greedy_labels: the plain argmax
collapse, so the test data does not depend on the code under test."""
import os

import numpy as np
import pytest
import torch

import vistaocr_amd as va
from tests import align_ref as ar
from tests import beam_data as bd
from tests.test_align_cpu import EXACT, exact_logits
from vistaocr_amd import _lib, ops
from vistaocr_amd.textutils import form_tokenized_words

pytestmark = pytest.mark.gpu

T1, B1, V1 = 294, 32, 96           # configs[1]'s logits shape


def eps_line(T, viterbi):
    return 4.0 * T * 2.0 ** -24 * max(abs(viterbi), 1.0)


def _run(x, lens, labels, canon=None):
    """x [T,B,V]; labels: per line a list of labellings (the n axis).  Returns host (scores [B,n,2], spans [B,n,M,2], label_scores)."""
    B, n = len(labels), max(len(h) for h in labels)
    M = max([len(l) for h in labels for l in h] + [1])
    lab = np.zeros((B, n, M), dtype=np.int32)
    ln = np.zeros((B, n), dtype=np.int32)
    for b, h in enumerate(labels):
        for q, l in enumerate(h):
            lab[b, q, :len(l)] = l
            ln[b, q] = len(l)
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda() if canon is not None else None
    out = ops.ctc_align(xd, lens, torch.from_numpy(lab).cuda(), torch.from_numpy(ln).cuda(), cd)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _check_line(got, ref, L, T, atol, label=""):
    """One (line, hypothesis): scores, padding, and - where the reference decides the path - identical spans and the label scores.
    Returns whether the spans were compared."""
    sc, sp, ls = got
    assert not np.isnan(sc).any() and not np.isnan(ls).any(), label
    assert np.all(sp[L:] == -1) and np.all(ls[L:] == 0), label
    if ref.spans is None:
        assert sc[0] == -np.inf and sc[1] == -np.inf and np.all(sp == -1) and np.all(ls == 0), (label, sc)
        return False
    assert abs(sc[0] - ref.viterbi) <= atol and abs(sc[1] - ref.ctc) <= atol, (label, sc, ref.viterbi, ref.ctc)
    if not ref.gap > eps_line(T, ref.viterbi):
        return False
    assert np.array_equal(sp[:L], ref.spans), (label, sp[:L].tolist(), ref.spans.tolist())
    assert np.allclose(ls[:L], ref.label_scores, atol=atol, rtol=0), label
    return True


def _compare(x, lens, labels, canon=None, atol=1e-3):
    sc, sp, ls = _run(x, lens, labels, canon)
    used = 0
    for b, h in enumerate(labels):
        for q, l in enumerate(h):
            ref = ar.align(x[:, b], lens[b], l, canon)
            used += _check_line((sc[b, q], sp[b, q], ls[b, q]), ref, len(l), x.shape[0], atol, (b, q))
    return used


@pytest.fixture(scope="module")
def english():
    al = va.english_alphabet()
    canon = np.array(al.canonical_indices())
    return al, canon, np.nonzero(canon == np.arange(len(al)))[0][1:]


@pytest.mark.parametrize("i", range(len(EXACT)))
def test_exact_against_brute_force(i):
    """The sizes of tests/test_align_cpu.py: spans equal the brute-force best path's, scores agree to 1e-5 |x| + 1e-6."""
    T, V, labels, canon = EXACT[i]
    x = exact_logits(i, T, V)
    best, spans, total, margin = ar.brute_force(x, labels, canon)
    sc, sp, ls = _run(x[:, None, :], [T], [[labels]], canon)
    print("exact case %d: got %s, brute force %r %r" % (i, sc[0, 0], best, total))
    if best == -np.inf:
        assert sc[0, 0, 0] == -np.inf and sc[0, 0, 1] == -np.inf and np.all(sp == -1) and np.all(ls == 0)
        return
    assert margin > 1e-4
    assert abs(sc[0, 0, 0] - best) <= 1e-5 * abs(best) + 1e-6
    assert abs(sc[0, 0, 1] - total) <= 1e-5 * abs(total) + 1e-6
    assert np.array_equal(sp[0, 0, :len(labels)], spans)


@pytest.mark.parametrize("p_char", [0.35, 0.10])
@pytest.mark.parametrize("seed", [7, 11])
def test_bench_shape_peaky(seed, p_char):
    """T = 294, B = 32, V = 96, greedy labels (L 43-67 at p_char 0.35: the S > 64 path; L 5-24 at 0.10: one wave per labelling).  The
    reference decides 32 of 32 lines in all four cases (eps_line 7.0e-5, smallest gap 2.5): >= 30 compared, identical spans on each."""
    x = bd.peaky_logits(np.random.default_rng(seed), T1, B1, V1, p_char=p_char)
    labels = [[ar.greedy_labels(x[:, b], T1)] for b in range(B1)]
    used = _compare(x, [T1] * B1, labels, atol=1e-3)
    print("peaky seed %d p_char %.2f: L %d-%d, %d of %d lines compared" % (seed, p_char, min(len(h[0]) for h in labels),
                                                                          max(len(h[0]) for h in labels), used, B1))
    assert used >= 30


@pytest.mark.parametrize("seed", [7, 11])
def test_dense_every_line_is_an_optimal_path(seed):
    """N(0,1) logits, T = 294, the first 60 greedy labels: scores near -1300, eps_line near 0.09, path identity undecidable (the
    reference decides 0-1 of 32 lines).  So on EVERY line the returned spans must describe a valid CTC path of the labelling whose fp64
    score is within eps_line of the fp64 optimum, and both returned scores must be within eps_line of the fp64 ones."""
    T = T1
    x = np.random.default_rng(seed).normal(0, 1, (T, B1, V1)).astype(np.float32)
    labels = [[ar.greedy_labels(x[:, b], T)[:60]] for b in range(B1)]
    sc, sp, ls = _run(x, [T] * B1, labels)
    worst = [0.0, 0.0, 0.0]
    for b in range(B1):
        lab = labels[b][0]
        ref = ar.align(x[:, b], T, lab)
        eps = eps_line(T, ref.viterbi)
        clp, cls = ar.class_logprobs(x[:, b])
        path = ar.path_from_spans(sp[b, 0], T, len(lab))
        assert path is not None and ar.path_is_valid(path, lab, cls), b
        score = ar.path_score(clp, lab, path)
        worst = [max(worst[0], ref.viterbi - score), max(worst[1], abs(sc[b, 0, 0] - score)), max(worst[2], abs(sc[b, 0, 1] - ref.ctc))]
        print("dense seed %d line %d: optimum %.6f path %.6f got %s ctc %.6f eps %.4f" % (seed, b, ref.viterbi, score, sc[b, 0], ref.ctc, eps))
        assert score >= ref.viterbi - eps, (b, score, ref.viterbi)
        assert abs(sc[b, 0, 0] - score) <= eps and abs(sc[b, 0, 1] - ref.ctc) <= eps, (b, sc[b, 0], score, ref.ctc)
    print("dense seed %d: largest optimum - path %.3g, |viterbi - path| %.3g, |ctc - fp64| %.3g" % ((seed,) + tuple(worst)))


@pytest.mark.parametrize("seed", [7, 11])
def test_dense_short_lines_decided(seed):
    """N(0,1) logits at T = 64 with the first 12 greedy labels: the reference decides 31 of 32 lines; >= 28 compared, identical spans."""
    T = 64
    x = np.random.default_rng(seed).normal(0, 1, (T, B1, V1)).astype(np.float32)
    labels = [[ar.greedy_labels(x[:, b], T)[:12]] for b in range(B1)]
    used = _compare(x, [T] * B1, labels, atol=1e-3)
    print("dense T=64 seed %d: %d of %d lines compared" % (seed, used, B1))
    assert used >= 28


def _loss_nll(x, lens, labels):
    """-ln P_ctc per line from vocr_ctc_loss_grad (no gradient)."""
    T, B, V = x.shape
    flat = np.array([v for l in labels for v in l] + [0], dtype=np.int32)
    ll = np.array([len(l) for l in labels], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(ll)[:-1]]).astype(np.int32)
    mll = int(ll.max())
    lib = _lib.load()
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in (flat, off, ll, np.array(lens, dtype=np.int32))]
    ws = torch.empty(lib.vocr_ctc_workspace_bytes(T, B, V, mll) // 4 + 4, dtype=torch.float32, device="cuda")
    nll = torch.empty(B, dtype=torch.float32, device="cuda")
    _lib.call("vocr_ctc_loss_grad", xd.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
              nll.data_ptr(), None, ws.data_ptr(), T, B, V, mll, None)
    torch.cuda.synchronize()
    return nll.cpu().numpy()


def _loss_case(name):
    if name == "peaky":
        x = bd.peaky_logits(np.random.default_rng(7), T1, B1, V1, p_char=0.10)
        lens = [T1] * B1
        labels = [ar.greedy_labels(x[:, b], T1) for b in range(B1)]
    elif name == "dense":
        x = np.random.default_rng(11).normal(0, 1, (64, B1, V1)).astype(np.float32)
        lens = [64] * B1
        labels = [ar.greedy_labels(x[:, b], 64)[:12] for b in range(B1)]
    else:
        lens = [0, 1, 60, 17, 2, 59, 33]
        x = np.random.default_rng(5).normal(0, 1, (60, 7, V1)).astype(np.float32)
        labels = [ar.greedy_labels(x[:, b], 60)[:8 + b] for b in range(7)]          # lines 0, 1 and 4 cannot hold theirs
    return x, lens, labels


@pytest.mark.parametrize("name", ["peaky", "dense", "ragged"])
def test_forward_score_equals_the_loss_kernel(name):
    """canon = None: out_scores[..., 1] = -nll of vocr_ctc_loss_grad on the same logits and labels to within 2 eps_line (two fp32 sums in
    different orders, each within eps_line of the truth); +-inf must match exactly."""
    x, lens, labels = _loss_case(name)
    nll = _loss_nll(x, lens, labels)
    sc, _, _ = _run(x, lens, [[l] for l in labels])
    finite = 0
    for b in range(x.shape[1]):
        ref = ar.align(x[:, b], lens[b], labels[b])
        print("loss %s line %d: align %r, -nll %r, fp64 %r" % (name, b, sc[b, 0, 1], -nll[b], ref.ctc))
        if np.isinf(nll[b]) or np.isinf(sc[b, 0, 1]):
            assert sc[b, 0, 1] == -nll[b] and ref.ctc == -np.inf, (b, sc[b, 0], nll[b])
        else:
            finite += 1
            assert abs(sc[b, 0, 1] + nll[b]) <= 2 * eps_line(x.shape[0], ref.viterbi), (b, sc[b, 0, 1], -nll[b])
    assert finite >= 4


def test_edge_cases(english):
    al, canon, cls = english
    rng = np.random.default_rng(21)
    T, V = 40, V1
    x = rng.normal(0, 1, (T, 7, V)).astype(np.float32)
    g = [ar.greedy_labels(x[:, b], T) for b in range(7)]
    # len = 0 (with and without labels), L = 0, a labelling longer than the line, labels out of range, one in the blank's class
    lens = [0, 0, T, 3, T, T, T]
    labels = [[[]], [g[1][:3]], [[]], [g[3][:9]], [[5, V, 7]], [[5, 0, 7]], [[-3]]]
    sc, sp, ls = _run(x, lens, labels)
    assert sc[0, 0].tolist() == [0.0, 0.0] and np.all(sc[[1, 3, 4, 5, 6], 0] == -np.inf) and np.all(sp == -1) and np.all(ls == 0)
    assert _compare(x, lens, labels) == 2                                            # the two empty labellings; L = 0: sum of ln p(blank)
    assert sc[2, 0, 0] == sc[2, 0, 1] and np.isfinite(sc[2, 0, 0])
    # B = 1; B = 7 ragged
    assert _compare(x[:, :1], [T], [[g[0][:10]]]) == 1
    rag = [0, 1, 40, 17, 2, 39, 33]
    assert _compare(x, rag, [[g[b][:6]] for b in range(7)]) >= 4
    # a repeated character at minimum length: len = L + repeats, every step is forced
    lab = [4, 4, 9, 9, 9, 2]
    y = rng.normal(0, 1, (T, 1, V)).astype(np.float32)
    sc, sp, ls = _run(y, [9], [[lab]])
    ref = ar.align(y[:, 0], 9, lab)
    assert ref.path == [1, 2, 3, 5, 6, 7, 8, 9, 11] and ref.gap == np.inf
    assert np.array_equal(sp[0, 0], ref.spans) and abs(sc[0, 0, 0] - ref.viterbi) <= 1e-3 and abs(sc[0, 0, 1] - ref.viterbi) <= 1e-3
    assert _run(y, [8], [[lab]])[0][0, 0].tolist() == [-np.inf, -np.inf]
    # a merged class: the two columns of the same string, the label given once by each member
    pair = [v for v in range(V) if canon[v] != v]
    assert len(pair) == 1
    hi, lo = pair[0], int(canon[pair[0]])
    z = bd.peaky_logits(np.random.default_rng(9), 60, 2, V, classes=[3, lo, hi, 17], p_char=0.3)
    both = [[[3, lo, 17, hi, lo]], [[3, hi, 17, lo, hi]]]
    z[:, 1] = z[:, 0]
    sc, sp, ls = _run(z, [60, 60], both, canon)
    assert sc[0].tobytes() == sc[1].tobytes() and sp[0].tobytes() == sp[1].tobytes() and ls[0].tobytes() == ls[1].tobytes()
    _compare(z, [60, 60], both, canon)
    zz = np.random.default_rng(10).normal(0, 1, (60, 2, V)).astype(np.float32)      # dense: the class is the logsumexp of both columns
    sc, _, _ = _run(zz, [60, 60], [[[lo, 5, hi]], [[hi, 5]]], canon)
    for b, l in enumerate([[lo, 5, hi], [hi, 5]]):
        ref = ar.align(zz[:, b], 60, l, canon)
        assert abs(sc[b, 0, 0] - ref.viterbi) <= 1e-3 and abs(sc[b, 0, 1] - ref.ctc) <= 1e-3
    sc, _, _ = _run(zz, [2, 3], [[[lo, hi]], [[hi, lo]]], canon)                       # one symbol twice: a blank has to sit between
    assert np.all(sc[0] == -np.inf) and np.isfinite(sc[1]).all()
    assert np.isfinite(_run(zz, [2, 3], [[[lo, hi]], [[hi, lo]]], None)[0]).all()      # ... and none without the classes
    # labellings with S > 64 next to ones with S <= 64 in the same call (S = 63 and S = 65 among them), n = 2 with an empty second rank:
    # every other logit of these lines is -inf, so a line is cut to the frames whose greedy labelling has the wanted length
    w = bd.peaky_logits(np.random.default_rng(12), 200, 4, V, p_char=0.4)
    want = [None, 31, 32, 7]
    wl = [200 if k is None else next(n for n in range(200) if len(ar.greedy_labels(w[:, b], n)) == k) for b, k in enumerate(want)]
    gl = [ar.greedy_labels(w[:, b], wl[b]) for b in range(4)]
    assert [len(l) for l in gl[1:]] == want[1:] and len(gl[0]) > 32
    assert _compare(w, wl, [[l, []] for l in gl]) == 4
    assert _compare(w, wl, [[gl[(b + 1) % 4], gl[b]] for b in range(4)]) == 4          # the first rank is another line's: no alignment


def _mass_lost_by_the_search(x, lens, K, nbest, canon):
    """fp64, restatements only: the largest ln P_ctc(labels | x) - (the search's acoustic score) over the hypotheses of a K-beam search.
    The search's acoustic score sums only the paths that stayed in the beam, so it is a LOWER BOUND of the forward score and reaches it
    when the beam is wide enough to prune nothing of weight."""
    from tests import beam_ref as br
    worst = 0.0
    for b in range(x.shape[1]):
        for hyp in br.beam_search(x[:, b], lens[b], K, nbest=nbest, canon=canon)[0]:
            d = ar.align(x[:, b], lens[b], hyp[0], canon).ctc - hyp[2]
            assert d > -1e-9
            worst = max(worst, d)
    return worst


def test_nbest_from_the_beam_search_on_the_device(english):
    """n = 4 straight from ops.ctc_beam_search's outputs without leaving the device: every filled rank aligns and the aligned path is the
    reference's.  The forward score is never below the search's acoustic score (the search sums only the paths its beam kept: at K = 16
    the fp64 restatements differ by up to 2.0e-3 on this data), and equals it at K = 128, where they differ by 1.8e-5 at most."""
    al, canon, cls = english
    x = bd.peaky_logits(np.random.default_rng(7), T1, B1, V1, classes=cls)
    assert _mass_lost_by_the_search(x, [T1] * B1, 128, 4, canon) < 1e-4         # a tenth of the tolerance below
    xd = torch.from_numpy(x).cuda()
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda()
    for K in (16, 128):
        lab, ln, bsc = ops.ctc_beam_search(xd, [T1] * B1, cd, K, 4)
        sc, sp, ls = ops.ctc_align(xd, [T1] * B1, lab, ln, cd)
        torch.cuda.synchronize()
        assert tuple(sc.shape) == (B1, 4, 2) and tuple(sp.shape) == (B1, 4, T1, 2)
        lab, ln, bsc, sc, sp, ls = [t.cpu().numpy() for t in (lab, ln, bsc, sc, sp, ls)]
        used, worst = 0, 0.0
        for b in range(B1):
            for q in range(4):
                if not np.isfinite(bsc[b, q, 0]):
                    continue
                worst = max(worst, sc[b, q, 1] - bsc[b, q, 1])
                assert sc[b, q, 1] >= bsc[b, q, 1] - 1e-3, (K, b, q, sc[b, q], bsc[b, q])
                if K == 128:
                    assert abs(sc[b, q, 1] - bsc[b, q, 1]) <= 1e-3, (b, q, sc[b, q], bsc[b, q])
                if q == 0 or b < 4:
                    ref = ar.align(x[:, b], T1, lab[b, q, :ln[b, q]], canon)
                    used += _check_line((sc[b, q], sp[b, q], ls[b, q]), ref, int(ln[b, q]), T1, 1e-3, (b, q))
        print("K = %d: largest forward score - search's acoustic score %.3g" % (K, worst))
        assert used >= 30


def test_bit_identical_runs(english):
    al, canon, cls = english
    x = np.random.default_rng(13).normal(0, 1, (T1, B1, V1)).astype(np.float32)
    labels = [[ar.greedy_labels(x[:, b], T1)[:60], ar.greedy_labels(x[:, b], T1)[:20]] for b in range(B1)]
    a = _run(x, [T1 - b for b in range(B1)], labels, canon)
    b = _run(x, [T1 - b for b in range(B1)], labels, canon)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_long_lines_keep_rows_and_back_pointers_in_the_workspace():
    """T = 4000 with 1796 and 1554 labels (label_stride = the longer one): beyond 1663 labels the rows of the sweep do not fit the LDS,
    and neither do the back pointers of 4000 frames x 57 chunks; both lines are decided by the reference (gaps 4.9 and 2.3)."""
    T = 4000
    x = bd.peaky_logits(np.random.default_rng(31), T, 2, V1, p_char=0.9)
    lens = [T, 3500]
    labels = [[ar.greedy_labels(x[:, b], lens[b])] for b in range(2)]
    assert len(labels[0][0]) > 1663 > len(labels[1][0]) > 1000
    assert _compare(x, lens, labels, atol=1e-3) == 2
    y = x[:3000]                                       # 1353 labels: the rows fit the LDS, the back pointers of 3000 frames do not
    short = [[ar.greedy_labels(y[:, 0], 3000)], [ar.greedy_labels(y[:, 1], 100)]]
    assert 1000 < len(short[0][0]) <= 1663 and _compare(y, [3000, 100], short, atol=1e-3) == 2


def test_unsupported_shapes_fail_before_any_launch():
    x = torch.zeros(8, 2, 300, device="cuda")
    lab = torch.ones(2, 3, dtype=torch.int32, device="cuda")
    ln = torch.full((2,), 3, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="ctc_align"):
        ops.ctc_align(x, [8, 8], lab, ln)
    with pytest.raises(RuntimeError, match="ctc_align"):
        ops.ctc_align(x[:, :, :50], [8, 8], lab.float(), ln)
    sc, sp, ls = ops.ctc_align(x[:, :, :50].contiguous(), [8, 8], lab, ln)             # 2-d labels: no n axis in the outputs
    assert tuple(sc.shape) == (2, 2) and tuple(sp.shape) == (2, 3, 2) and tuple(ls.shape) == (2, 3, 2)
    assert np.isfinite(sc.cpu().numpy()).all() and np.all(sp.cpu().numpy() >= 0)     # 1 1 1 needs 5 frames and has 8


def _tiny_model(al):
    from oracle import closed_form as cf
    hp = dict(input_line_height=30, rds_line_height=30, lstm_input_dim=32, num_lstm_layers=1, num_lstm_hidden_units=32,
              p_lstm_dropout=0.0, num_in_channels=1)
    sd_np = cf.closed_form_state(hp, len(al))
    model = va.CnnOcrModel(alphabet=al, verbose=False, **hp)
    sd = model.state_dict()
    for k, v in sd_np.items():
        sd[k] = torch.from_numpy(v)
    model.load_state_dict(sd)
    return model


@pytest.fixture(scope="module")
def word_lm(tmp_path_factory, english):
    from tests import word_beam_data as wd
    al = english[0]
    rng = np.random.default_rng(1)
    words, wts = wd.make_lexicon(rng, 400)
    sents = wd.make_sentences(rng, words, wts, 1532, max_words=6)
    path = str(tmp_path_factory.mktemp("wlm") / "word3.arpa")
    wd.write_word_arpa(path, words, wts, sents[:1500], seed=2)
    x, lens = wd.sentence_logits(np.random.default_rng(3), sents[1500:], al, T1)
    return va.WordNgramLM.from_arpa(path, al), x, lens


def _check_alignments(strings_ux, aligns, al, lens):
    for b, (s, a) in enumerate(zip(strings_ux, aligns)):
        assert a is not None and [c.uxxxx for c in a.chars] == s.split(), b
        assert a.ctc_logp >= a.viterbi_logp - 1e-4
        prev = -1
        for c in a.chars:
            assert prev < c.first_frame <= c.last_frame < lens[b] and c.mean_logp <= c.peak_logp + 1e-6 <= 1e-6
            prev = c.last_frame


def test_decode_aligned_of_every_decoder(english, word_lm):
    """decode_aligned returns decode's strings; on peaky logits every alignment's ctc_logp is the search's acoustic score (1e-3) where
    the search pruned nothing of weight (the character search at beam = 128, the word search on its sentence logits at beam = 16: the
    fp64 restatements agree exactly there), and is never below it."""
    al, canon, cls = english
    x = bd.peaky_logits(np.random.default_rng(7), T1, B1, V1, classes=cls)
    x[:, :, 0] = np.where(np.isinf(x[:, :, 0]), x.max(axis=2) - 30.0, x[:, :, 0])     # a blank is always possible
    xd = torch.from_numpy(x).cuda()
    lens = [T1 - 3 * b for b in range(B1)]
    aligner = va.CtcAligner(al)
    for dec in (va.ArgmaxDecoder(al), va.BeamDecoder(al, beam=16)):
        for ux in (True, False):
            hyps, aligns = dec.decode_aligned(xd, lens, uxxxx=ux)
            assert hyps == dec.decode(xd, lens, uxxxx=ux)
        strings = dec.decode(xd, lens, uxxxx=True)
        _check_alignments(strings, aligns, al, lens)
        again = aligner.align(xd, lens, strings)                 # the same through the strings (which name a class by any member)
        assert [[c[1:] for c in a.chars] for a in again] == [[c[1:] for c in a.chars] for a in aligns]
        assert [a.ctc_logp for a in again] == [a.ctc_logp for a in aligns]
    for a, h in zip(aligns, dec.decode_nbest(xd, lens, 1)):                           # beam = 16: the search's score is a lower bound
        assert a.ctc_logp >= h[0][1][1] - 1e-3
    # a beam that prunes nothing of weight (the fp64 restatements differ by 2.5e-7 here): the two scores are the same number
    assert _mass_lost_by_the_search(x, lens, 128, 4, canon) < 1e-4
    dec = va.BeamDecoder(al, beam=128, nbest=4)
    nb = dec.decode_nbest(xd, lens)
    hyps, lists = dec.decode_aligned(xd, lens, nbest=4)
    assert hyps == dec.decode(xd, lens)
    n = 0
    for b in range(B1):
        assert [(h[0], h[1]) for h in lists[b]] == nb[b]
        for labels, (total, acoustic, lm), a in lists[b]:
            assert a is not None and [c.label for c in a.chars] == labels
            assert abs(a.ctc_logp - acoustic) <= 1e-3, (b, a.ctc_logp, acoustic)
            n += 1
    assert n >= 3 * B1
    from_lists = aligner.align(xd, lens, nb)                                          # decode_nbest's lists are accepted as labels
    assert [[a.chars for a in row] for row in from_lists] == [[h[2].chars for h in row] for row in lists]
    lm, xs, slens = word_lm
    wdec = va.WordBeamDecoder(al, lm, beam=16, lm_weight=0.8)
    xsd = torch.from_numpy(xs).cuda()
    hyps, aligns = wdec.decode_aligned(xsd, slens, uxxxx=True)
    assert hyps == wdec.decode(xsd, slens, uxxxx=True)
    acoustic = [h[0][1][1] if h else None for h in wdec.decode_nbest(xsd, slens, 1)]
    for b, a in enumerate(aligns):
        assert (a is None) == (acoustic[b] is None)
        if a is not None:
            assert abs(a.ctc_logp - acoustic[b]) <= 1e-3
            assert [w.token for w in aligner.words(a)] == form_tokenized_words(hyps[b].split())
    assert sum(a is not None for a in aligns) >= len(aligns) - 2


def test_decode_dataset_writes_word_rows(tmp_path):
    from vistaocr_amd.loop import SortByWidthCollater, decode_dataset
    al = va.english_alphabet()
    model = _tiny_model(al)
    r = np.random.RandomState(0)
    items = [(torch.from_numpy(r.uniform(0, 1, size=(1, 30, w)).astype(np.float32)), [1], {"width": w, "utt-id": "doc7_line_%d" % i})
             for i, w in enumerate([140, 96, 201, 64])]
    loader = [SortByWidthCollater(items[:2]), SortByWidthCollater(items[2:])]
    assert decode_dataset(model, loader, str(tmp_path / "default")) == 4
    assert sorted(os.listdir(tmp_path / "default")) == ["hyp-chars.txt", "hyp-chars.txt.utf8"]
    for name, dec in (("greedy", None), ("beam", va.BeamDecoder(al, beam=8))):
        d = tmp_path / name
        assert decode_dataset(model, loader, str(d), decoder=dec, aligner=va.CtcAligner(al)) == 4
        assert sorted(os.listdir(d)) == ["hyp-chars.txt", "hyp-chars.txt.utf8", "hyp-words.tsv"]
        if dec is None:                                                               # the two files of the default call, byte for byte
            for f in ("hyp-chars.txt", "hyp-chars.txt.utf8"):
                assert open(d / f, "rb").read() == open(tmp_path / "default" / f, "rb").read()
        widths = {"doc7_line_%d" % i: w for i, w in enumerate([140, 96, 201, 64])}
        rows = [l.split("\t") for l in open(d / "hyp-words.tsv").read().splitlines()]
        want = []
        for line in open(d / "hyp-chars.txt").read().splitlines():
            ux, uid = line.rsplit(" (", 1)
            want += [(uid.rstrip(")"), tok) for tok in form_tokenized_words(ux.split())]
        assert [(r[0], r[1]) for r in rows] == want and len(rows) > 0
        for uid, tok, x0, x1, conf, mean in rows:
            assert 0 <= int(x0) < int(x1) <= widths[uid] and 0.0 < float(conf) <= 1.0 and float(mean) <= 0.0
