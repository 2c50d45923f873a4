"""GPU: vocr_ctc_keyword_scores (vistaocr_amd/csrc/ctc_keyword.hip) through ops.ctc_keyword_scores, KeywordSpotter and decode_dataset,
against the fp64 restatement of tests/kws_ref.py (itself checked against a brute force over all paths in tests/test_kws_cpu.py).

EVERY entry of all three outputs is compared.  Log counts and best scores: -inf exactly where the reference has -inf, never NaN or
+inf, finite entries within
    bound = 4 * (T + 2) * 2^-24 * max(|score|, 1)
of fp64: tests/test_align_gpu.py's eps_line (a linear worst-case bound on the fp32 rounding accumulated over the frames' additions, the
floor of 1 covering the log-softmax's own rounding) with the two boundary factors counted as frames.  Spans must be IDENTICAL wherever
the reference's decision gap exceeds twice that bound; at most 10 % of the (line, query) pairs of a case may be left out this way.  The
seeds below keep the fp64 reference alone under that cap.  Its left-out share, computed on the CPU: 4.8 % (1 of 21 pairs) at L = 1
and at L = 128, 3.2 % in the mixed call, 3.8 % on the peaky lines of the alphabet test, 0.39 % (8 of 2048 pairs) on configs[1]'s shape
with dense logits, 0 % in every other case, configs[1]'s shape with peaky logits included.  (The peaky lines of these tests give every
frame a competitor 2 .. 8 below the peak: with beam_data's defaults many frames have probability exactly 1 and single-character queries
tie exactly.)

Each test prints the largest difference and the largest fraction of the bound used (profiles/ctc_kws_errors.txt keeps a run's output)."""
import os

import numpy as np
import pytest
import torch

import vistaocr_amd as va
from tests import align_ref as ar
from tests import beam_data as bd
from tests import kws_ref as kr
from vistaocr_amd import ops

pytestmark = pytest.mark.gpu

NEG = -np.inf
T1, B1, V1 = 294, 32, 96           # configs[1]'s logits shape


def bound(T, score):
    return 4.0 * (T + 2) * 2.0 ** -24 * np.maximum(np.abs(score), 1.0)


def _run(x, lens, queries, flags=None, canon=None, width=None):
    """x [T,B,V]; queries a list of label lists.  Host (log_count [B,Q], best [B,Q], span [B,Q,2])."""
    L = max([len(q) for q in queries] + [1]) if width is None else width
    lab = np.zeros((len(queries), L), dtype=np.int32)
    for i, q in enumerate(queries):
        lab[i, :min(len(q), L)] = q[:L]
    ln = np.array([len(q) for q in queries], dtype=np.int32)
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda() if canon is not None else None
    fd = torch.as_tensor(flags, dtype=torch.int32).cuda() if flags is not None else None
    out = ops.ctc_keyword_scores(xd, lens, torch.from_numpy(lab).cuda(), torch.from_numpy(ln).cuda(), fd, cd)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _check(name, x, lens, queries, flags=None, canon=None, got=None, ref=None, need_finite=1):
    """All entries of all outputs against the reference.  Returns (got, ref)."""
    T = x.shape[0]
    lc, best, span = _run(x, lens, queries, flags, canon) if got is None else got
    ref = kr.search(x, lens, queries, flags, canon) if ref is None else ref
    worst, frac, finite = 0.0, 0.0, 0
    for what, g, r in (("log_count", lc, ref["log_count"]), ("best", best, ref["best"])):
        assert not np.isnan(g).any() and not np.any(g == np.inf), (name, what)
        assert np.array_equal(g == NEG, r == NEG), (name, what, np.argwhere((g == NEG) != (r == NEG))[:5].tolist())
        fin = r != NEG
        finite += int(fin.sum())
        if fin.any():
            d = np.abs(g[fin].astype(np.float64) - r[fin])
            bnd = bound(T, r[fin])
            worst, frac = max(worst, float(d.max())), max(frac, float((d / bnd).max()))
    dead = ref["best"] == NEG
    assert np.all(span[dead] == -1), name
    decided = ~dead & (ref["gap"] > 2 * bound(T, ref["best"]))
    left_out = float((~dead & ~decided).sum()) / max(int(dead.size), 1)
    wrong = np.argwhere(decided & np.any(span != ref["span"], axis=-1))
    print("%s: %d pairs, %d finite scores, largest |fp32 - fp64| %.3g, largest fraction of the bound %.3f, spans compared on %d, "
          "left out %.2f %%" % (name, dead.size, finite, worst, frac, int(decided.sum()), 100 * left_out))
    assert frac <= 1.0, (name, worst, frac)
    assert len(wrong) == 0, (name, wrong[:5].tolist(), span[tuple(wrong[0])].tolist(), ref["span"][tuple(wrong[0])].tolist())
    assert left_out <= 0.10, (name, left_out)
    assert finite >= need_finite, (name, finite)
    return (lc, best, span), ref


def _lines(seed, T, V, n_peaky, n_dense, p_char=0.9):
    """n_peaky peaky lines followed by n_dense lines of N(0,1) logits, [T, B, V]."""
    rng = np.random.default_rng(seed)
    parts = []
    if n_peaky:
        parts.append(bd.peaky_logits(rng, T, n_peaky, V, p_char=p_char, p_alt=1.0, cost=(2.0, 8.0)))    # a near competitor in every frame: no ties
    if n_dense:
        parts.append(rng.normal(0, 1, (T, n_dense, V)).astype(np.float32))
    return np.concatenate(parts, axis=1)


def _queries_of_length(rng, x, lens, n_peaky, V, L):
    """Per peaky line one substring of length L of its greedy labelling (where it has one), and one random query of that length."""
    out = []
    for b in range(n_peaky):
        g = ar.greedy_labels(x[:, b], lens[b])
        if len(g) >= L:
            o = int(rng.integers(0, len(g) - L + 1))
            out.append(g[o:o + L])
    out.append([int(v) for v in rng.integers(1, V, L)])
    return out


QUERY_LENGTHS = [1, 8, 9, 16, 17, 32, 33, 128]       # around every lane layout's limit (scripts/ctc_parent_ab.py runs them too)


@pytest.mark.parametrize("L", QUERY_LENGTHS)
def test_query_lengths_and_lane_layouts(L):
    """S = 2L-1 = 1; 15 / 17 (the 16-lane segment's seam); 31 / 33; 63 / 65 (one position per lane against four); 255.  Two peaky lines
    (substrings of their greedy labellings: real occurrences) and one short dense line (every query has a finite, tiny count), Q = 7
    where the layout packs 4 or 2 queries per wave: no multiple of either."""
    T = 340 if L > 33 else 120
    V = 40
    x = _lines(40 + L, T, V, 2, 1)
    lens = [T, T - 7, min(T, 2 * L + 5)]
    rng = np.random.default_rng(L)
    qs = _queries_of_length(rng, x, lens, 2, V, L)
    assert len(qs) == 3
    while len(qs) < 7:
        qs += _queries_of_length(rng, x, lens, 2, V, L)
    _check("L = %d" % L, x, lens, qs[:7], need_finite=14)


def test_mixed_lengths_land_at_the_callers_index():
    """One call with every length of the layouts' seams in scrambled order, next to invalid ones: the device sorts the queries, the
    results must sit at the caller's index."""
    T, V = 340, 40
    x = _lines(77, T, V, 2, 1)
    lens = [T, T - 11, 300]
    rng = np.random.default_rng(78)
    qs = []
    for L in (1, 8, 9, 16, 17, 32, 33, 128, 2, 5, 12, 64, 100):
        qs += _queries_of_length(rng, x, lens, 2, V, L)
    qs += [[0], [V], []]
    order = rng.permutation(len(qs))
    qs = [qs[i] for i in order]
    (lc, best, span), ref = _check("mixed lengths", x, lens, qs, need_finite=60)
    again = _run(x, lens, qs[::-1])                                        # the reversed list: the reversed columns, bit for bit
    for u, v in zip((lc, best, span), again):
        assert np.array_equal(u, v[:, ::-1], equal_nan=True)


def test_frame_counts():
    """T = 1; lens = 0; ragged lens in one batch; a query longer than the line; a repeated label that needs its blanks: aaa in 5 frames
    (one path) and in 4 (none)."""
    V = 8
    x = np.random.default_rng(3).normal(0, 1, (12, 6, V)).astype(np.float32)
    lens = [0, 1, 12, 5, 4, 7]
    qs = [[3], [3, 3, 3], [1, 2], [2, 2, 2, 2, 2, 2, 2], [5, 6, 7, 1, 2, 3, 4, 5, 6, 7, 1, 2, 3], [4, 4]]
    (lc, best, span), ref = _check("frame counts", x, lens, qs, need_finite=20)
    assert np.all(lc[0] == NEG) and np.all(span[0] == -1)                  # lens = 0
    assert np.isfinite(lc[1, 0]) and np.all(lc[1, 1:] == NEG)              # one frame holds one label
    assert np.isfinite(lc[3, 1]) and lc[4, 1] == NEG and tuple(span[3, 1]) == (0, 4)
    assert np.all(lc[:, 3] == NEG) and np.all(lc[:, 4] == NEG)             # 13 and 7 + 6 frames needed, 12 there
    y = np.random.default_rng(4).normal(0, 1, (1, 2, 5)).astype(np.float32)
    _check("T = 1", y, [1, 1], [[1], [4], [2, 3]], need_finite=8)


def test_alphabet_sizes_classes_and_minus_infinity():
    """V = 2 and V = 256; canon with a two-member class as k_1, as k_L and as neither; -inf logits; a whole -inf row."""
    x = np.random.default_rng(5).normal(0, 1, (9, 2, 2)).astype(np.float32)
    _check("V = 2", x, [9, 6], [[1], [1, 1], [1, 1, 1]], need_finite=12)
    x = np.random.default_rng(6).normal(0, 1, (20, 2, 256)).astype(np.float32)
    _check("V = 256", x, [20, 13], [[255], [1, 255, 128], [64, 64], [200, 3, 77, 5, 255, 254, 253]], need_finite=16)
    V = 12
    canon = np.arange(V)
    canon[9] = 4                                                           # columns 4 and 9 are one symbol
    x = np.random.default_rng(7).normal(0, 1, (16, 3, V)).astype(np.float32)
    qs = [[4, 2, 3], [9, 2, 3], [2, 3, 9], [2, 3, 4], [2, 4, 3], [4, 9], [9], [1, 2]]
    (lc, best, span), _ = _check("two-member class", x, [16, 16, 11], qs, canon=canon, need_finite=40)
    for u in (lc, best, span):                                             # a label given by either member: the same bits
        assert np.array_equal(u[:, 0], u[:, 1]) and np.array_equal(u[:, 2], u[:, 3])
    _check("no classes", x, [16, 16, 11], qs, need_finite=40)
    y = x.copy()
    y[:, 0, 2] = NEG                                                       # a class that never occurs
    y[3:6, 1, 1:] = NEG                                                    # frames that can only be blank
    y[7, 2, :] = NEG                                                       # a frame with no probability at all: nothing crosses it
    (lc, best, span), _ = _check("-inf logits", y, [16, 16, 11], qs, canon=canon, need_finite=20)
    assert np.all(lc[0, [0, 1, 2, 3, 4, 7]] == NEG) and np.isfinite(lc[0, 5])
    z = bd.peaky_logits(np.random.default_rng(8), 60, 4, 30, p_char=0.5)
    lens = [60, 60, 41, 60]
    qs = [ar.greedy_labels(z[:, b], lens[b])[o:o + n] for b in range(4) for o, n in ((0, 3), (2, 5), (4, 1))] + [[1, 2]]
    _check("peaky", z, lens, qs, need_finite=12)


def test_peak_before_the_start_and_after_the_end():
    """The frames directly before the best span's start and directly after its end give the keyword's first / last class the probability
    1 - 2^-20: entry and exit are ln(2^-20) there, where 1 - p in fp32 has no digits left (the log-softmax of such a frame rounds to 0).
    Queries a, ab and ba on the frames (a peak) a b (b peak), next to the frames in between."""
    V = 5
    lo = float(np.log(2.0 ** -20 / (1 - 2.0 ** -20) / (V - 1)))            # every other class, the peak's logit being 0
    x = np.random.default_rng(9).normal(0, 1, (6, 1, V)).astype(np.float32)
    x[1, 0, :], x[1, 0, 1] = lo, 0.0                                       # frame 1: class 1 has 1 - 2^-20
    x[4, 0, :], x[4, 0, 2] = lo, 0.0                                       # frame 4: class 2
    qs = [[1], [2], [1, 2], [2, 1], [3, 1], [2, 3], [1, 3, 2], [3]]
    (lc, best, span), ref = _check("peaks", x, [6], qs, need_finite=16)
    assert np.isfinite(ref["log_count"]).all()
    flags = [1, 2, 3, 0, 1, 2, 3, 0]
    _check("peaks, anchored", x, [6], qs, flags, need_finite=16)
    # the same with the peak frames at the line's ends
    y = x[1:5].copy()
    _check("peaks at the ends", y, [4], [[3], [4], [3, 4], [1, 3], [3, 2], [1], [2]], need_finite=14)


def test_tie_rule():
    """Constant logits, T = 4, one single-label query: the spans (0,0) and (T-1,T-1) tie bit-exactly (0 + lp + notc and notc + lp + 0),
    the earliest end frame wins (both sums are the one rounded lp + notc, in fp32 as in fp64)."""
    x = np.zeros((4, 2, 3), dtype=np.float32)
    x[:, 1] = 1.25
    lc, best, span = _run(x, [4, 4], [[1], [2]])
    ref = kr.search(x, [4, 4], [[1], [2]])
    assert np.all(ref["gap"] == 0.0)
    assert np.array_equal(span, ref["span"]) and np.all(span == 0)
    assert np.allclose(best, ref["best"], atol=1e-6) and np.allclose(lc, ref["log_count"], atol=1e-6)
    assert np.array_equal(best[0], best[1])


def test_anchors_and_the_forward_score():
    """Each anchor alone, and both: with both the count is P_ctc(query | x), which ops.ctc_align computes on the device too; the two
    fp32 results agree within the bound."""
    T, V = 50, 30
    x = _lines(11, T, V, 3, 1, p_char=0.4)
    lens = [T, T, 30, 20]
    whole = [ar.greedy_labels(x[:, b], lens[b]) for b in range(3)]
    qs = [w for w in whole] + [whole[0][:3], whole[0][-3:], whole[1][:1], whole[2][-2:], [3, 4]]
    for fl in (1, 2, 3):
        _check("anchors = %d" % fl, x, lens, qs, [fl] * len(qs), need_finite=6)
    fl = [3, 0, 1, 2, 3, 0, 1, 2]
    _check("anchors mixed", x, lens, qs, fl, need_finite=10)
    M = max(len(q) for q in qs)
    lab = np.zeros((4, len(qs), M), dtype=np.int32)
    ln = np.zeros((4, len(qs)), dtype=np.int32)
    for i, q in enumerate(qs):
        lab[:, i, :len(q)] = q
        ln[:, i] = len(q)
    xd = torch.from_numpy(x).cuda()
    sc = ops.ctc_align(xd, lens, torch.from_numpy(lab).cuda(), torch.from_numpy(ln).cuda())[0].cpu().numpy()[:, :, 1]
    lc = _run(x, lens, qs, [3] * len(qs))[0]
    assert np.array_equal(lc == NEG, sc == NEG) and np.isfinite(lc).sum() >= 3
    fin = np.isfinite(lc)
    d = np.abs(lc[fin].astype(np.float64) - sc[fin])
    bnd = bound(T, lc[fin])
    print("both anchors against ops.ctc_align: %d finite scores, largest difference %.3g, largest fraction of the bound %.3f"
          % (int(fin.sum()), d.max(), (d / bnd).max()))
    assert np.all(d <= bnd)


def test_trimmed_spans():
    """Flag bits 2 / 3 (the whole-word search's): the same scores bit for bit, the span without the first / last label's frames."""
    T, V = 60, 30
    x = _lines(12, T, V, 3, 1, p_char=0.5)
    lens = [T, T, 45, 20]
    qs = [ar.greedy_labels(x[:, b], lens[b])[o:o + n] for b in range(3) for o, n in ((0, 3), (1, 4), (3, 9))] + [[1, 2], [5]]
    plain = _run(x, lens, qs, [0] * len(qs))
    for fl in (4, 8, 12, 5, 10):
        got, ref = _check("trim = %d" % fl, x, lens, qs, [fl] * len(qs), need_finite=10)
        ok = np.array([len(q) >= (3 if fl & 12 == 12 else 2) for q in qs])
        assert np.all(got[0][:, ~ok] == NEG)
        if not fl & 3:
            assert np.array_equal(got[0][:, ok], plain[0][:, ok]) and np.array_equal(got[1][:, ok], plain[1][:, ok])
            hit = got[2][:, ok, 0] >= 0
            assert np.all(got[2][:, ok, 0][hit] >= plain[2][:, ok, 0][hit]) and np.all(got[2][:, ok, 1][hit] <= plain[2][:, ok, 1][hit])


def test_invalid_queries_poison_only_their_own_column():
    V = 10
    canon = np.arange(V)
    canon[7] = 0                                                           # column 7 is in the blank's class
    x = np.random.default_rng(13).normal(0, 1, (14, 3, V)).astype(np.float32)
    good = [[1, 2], [3], [4, 5, 6]]
    qs = [good[0], [1, 0, 2], good[1], [V], [2, 7], good[2], [], [-3, 1]]
    (lc, best, span), _ = _check("invalid queries", x, [14, 9, 14], qs, canon=canon, need_finite=18)
    bad = [1, 3, 4, 6, 7]
    assert np.all(lc[:, bad] == NEG) and np.all(best[:, bad] == NEG) and np.all(span[:, bad] == -1)
    alone = _run(x, [14, 9, 14], good, canon=canon)
    for u, v in zip((lc, best, span), alone):
        assert np.array_equal(u[:, [0, 2, 5]], v)
    # a length beyond the array's width is invalid too; the labels behind it are never read
    lc2 = _run(x, [14, 9, 14], [[1, 2, 3], [1, 2]], width=2)[0]
    assert np.all(lc2[:, 0] == NEG) and np.isfinite(lc2[:, 1]).all()
    with pytest.raises(RuntimeError, match="ctc_keyword_scores"):
        ops.ctc_keyword_scores(torch.zeros(4, 1, 300, device="cuda"), [4], torch.ones(1, 2, dtype=torch.int32, device="cuda"),
                               torch.full((1,), 2, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="ctc_keyword_scores"):
        ops.ctc_keyword_scores(torch.zeros(4, 1, 30, device="cuda"), [4], torch.ones(1, 129, dtype=torch.int32, device="cuda"),
                               torch.full((1,), 2, dtype=torch.int32, device="cuda"))


@pytest.fixture(scope="module")
def bench_case():
    """configs[1]'s shape, peaky logits, Q = 64 of lengths 3 .. 12: half substrings of the lines' greedy labellings, half random."""
    x = bd.peaky_logits(np.random.default_rng(7), T1, B1, V1, p_char=0.35)
    rng = np.random.default_rng(8)
    qs = []
    for i in range(32):
        g = ar.greedy_labels(x[:, i], T1)
        L = int(rng.integers(3, 13))
        o = int(rng.integers(0, len(g) - L + 1))
        qs.append(g[o:o + L])
        qs.append([int(v) for v in rng.integers(1, V1, int(rng.integers(3, 13)))])
    lens = [T1 - 3 * b for b in range(B1)]
    return x, lens, qs, kr.search(x, lens, qs)


def test_bench_shape(bench_case):
    x, lens, qs, ref = bench_case
    _check("T = 294, B = 32, V = 96, Q = 64", x, lens, qs, ref=ref, need_finite=48)


@pytest.fixture(scope="module")
def bench_case_dense():
    """The same shape with beam_data's dense logits (N(0, 3) in every column), where every (line, query) pair has a finite count and a
    best span: the peaky case above is -inf off its peaks, so only a line's own substrings are live there.  Queries as above, the
    substrings taken from these lines' greedy labellings."""
    x = bd.dense_logits(np.random.default_rng(16), T1, B1, V1)
    rng = np.random.default_rng(116)
    lens = [T1 - 3 * b for b in range(B1)]
    qs = []
    for i in range(32):
        g = ar.greedy_labels(x[:, i], lens[i])
        L = int(rng.integers(3, 13))
        o = int(rng.integers(0, len(g) - L + 1))
        qs.append(g[o:o + L])
        qs.append([int(v) for v in rng.integers(1, V1, int(rng.integers(3, 13)))])
    return x, lens, qs, kr.search(x, lens, qs)


def test_bench_shape_dense(bench_case_dense):
    x, lens, qs, ref = bench_case_dense
    _check("T = 294, B = 32, V = 96, Q = 64, dense", x, lens, qs, ref=ref, need_finite=2 * B1 * 64)


def test_bit_identical_runs(bench_case, bench_case_dense):
    for x, lens, qs, _ in (bench_case, bench_case_dense):
        a, b = _run(x, lens, qs), _run(x, lens, qs)
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()


def _sentence_logits(al, text, T, rng, sharp=14.0):
    """Logits [T, V] that spell `text` (utf-8): every character two frames, a blank frame between, N(0,1) noise under a peak."""
    x = rng.normal(0, 1, (T, len(al))).astype(np.float32)
    t = 1
    for ch in text:
        k = al.char_to_idx["u%04x" % ord(ch)]
        x[t:t + 2, k] += sharp
        x[t + 2, 0] += sharp
        t += 3
    x[0, 0] += sharp
    x[t:, 0] += sharp
    return x


def test_keyword_spotter():
    """utf-8, uxxxx and index keywords give the same arrays; found words are found where they are; whole_word = the reference's sum of
    the four bounded queries, the span without the spaces."""
    al = va.english_alphabet()
    canon = np.array(al.canonical_indices())
    rng = np.random.default_rng(15)
    T = 100
    texts = ["the other cat", "a cat the", "then no"]
    x = np.stack([_sentence_logits(al, s, T, rng) for s in texts], axis=1)
    lens = [T, 60, T]
    xd = torch.from_numpy(x).cuda()
    words = ["the", "cat", "other", "no", "zebra"]
    idx = [[al.char_to_idx["u%04x" % ord(c)] for c in w] for w in words]
    sp = va.KeywordSpotter(al)
    h8 = sp.search(xd, lens, words)
    hux = sp.search(xd, lens, [" ".join("u%04x" % ord(c) for c in w) for w in words])
    hidx = sp.search(xd, lens, idx)
    for a, b, c in zip(h8[1:], hux[1:], hidx[1:]):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    ref = kr.search(x, lens, idx, None, canon)
    _check("spotter", x, lens, idx, canon=canon, got=(h8.log_count, h8.best_logp, h8.best_span), ref=ref, need_finite=15)
    assert h8.expected_count.shape == (3, 5) and np.all(h8.prob_upper <= 1.0)
    print("expected counts:\n%s" % np.round(h8.expected_count, 3))
    assert np.allclose(h8.expected_count[0, :3], [2.0, 1.0, 1.0], atol=0.05)           # "the" in "the" and in "other"
    assert np.allclose(h8.expected_count[1, :2], [1.0, 1.0], atol=0.05) and h8.expected_count[2, 0] > 0.9
    assert np.all(h8.expected_count[:, 4] < 1e-6)
    assert h8.best_span[0, 1].tolist() == [31, 38]                                     # c a t: characters 10 .. 12, frames 1 + 3 * 10 ..
    # whole words: "the" once in line 0 (not in "other"), once at the end of line 1, not in "then"
    ww = va.KeywordSpotter(al, whole_word=True)
    hw = ww.search(xd, lens, words)
    s = al.char_to_idx["u0020"]
    four = [q for l in idx for q in ([s] + l + [s], l + [s], [s] + l, l)]
    r4 = kr.search(x, lens, four, [12, 9, 6, 3] * len(idx), canon)
    want = np.logaddexp.reduce(r4["log_count"].reshape(3, len(idx), 4), axis=2)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(hw.log_count), fin)
    d = np.abs(hw.log_count[fin].astype(np.float64) - want[fin])
    bnd = bound(T, want[fin])                                                          # a log count like any other: the one bound
    print("whole word: %d finite log counts, largest |fp32 - fp64| %.3g, largest fraction of the bound %.3f"
          % (int(fin.sum()), d.max(), (d / bnd).max()))
    assert np.all(d <= bnd)
    assert np.allclose(hw.expected_count[0, :3], [1.0, 1.0, 1.0], atol=0.05) and hw.expected_count[2, 0] < 0.01
    assert abs(hw.expected_count[1, 0] - 1.0) < 0.05 and abs(hw.expected_count[2, 3] - 1.0) < 0.05
    best4 = r4["best"].reshape(3, len(idx), 4)
    which = np.argmax(best4, axis=2)
    for b in range(3):
        for q in range(len(idx)):
            if np.isfinite(best4[b, q]).any() and np.sort(best4[b, q])[-1] - np.sort(best4[b, q])[-2] > 1e-3:
                assert hw.best_span[b, q].tolist() == r4["span"].reshape(3, len(idx), 4, 2)[b, q, which[b, q]].tolist(), (b, q)
    assert hw.best_span[0, 0].tolist() == [1, 8] and hw.best_span[0, 1].tolist() == [31, 38]
    with pytest.raises(ValueError, match="u0020"):
        va.KeywordSpotter(va.Alphabet(["<ctc-blank>", "u0061", "u0062"]), whole_word=True)
    with pytest.raises(ValueError, match="not in the alphabet"):
        sp.search(xd, lens, ["café"])


def test_decode_dataset_writes_keyword_rows(tmp_path):
    from tests.test_align_gpu import _tiny_model
    from vistaocr_amd.loop import SortByWidthCollater, decode_dataset
    al = va.english_alphabet()
    model = _tiny_model(al)
    r = np.random.RandomState(0)
    widths = [140, 96, 201, 64]
    items = [(torch.from_numpy(r.uniform(0, 1, size=(1, 30, w)).astype(np.float32)), [1], {"width": w, "utt-id": "doc7_line_%d" % i})
             for i, w in enumerate(widths)]
    loader = [SortByWidthCollater(items[:2]), SortByWidthCollater(items[2:])]
    assert decode_dataset(model, loader, str(tmp_path / "default")) == 4
    # keywords taken from what the model says: the first characters of every hypothesis, and one it does not say
    hyps = [l.rsplit(" (", 1)[0].split() for l in open(tmp_path / "default" / "hyp-chars.txt").read().splitlines()]
    kws = sorted(set(" ".join(h[:2]) for h in hyps if len(h) >= 2)) + ["u007a u007a u007a u007a"]
    sp = va.KeywordSpotter(al)
    assert decode_dataset(model, loader, str(tmp_path / "kws"), spotter=sp, keywords=kws, min_count=0.0) == 4
    assert sorted(os.listdir(tmp_path / "kws")) == ["hyp-chars.txt", "hyp-chars.txt.utf8", "hyp-kws.tsv"]
    for f in ("hyp-chars.txt", "hyp-chars.txt.utf8"):
        assert open(tmp_path / "kws" / f, "rb").read() == open(tmp_path / "default" / f, "rb").read()
    rows = [l.split("\t") for l in open(tmp_path / "kws" / "hyp-kws.tsv").read().splitlines()]
    wid = {"doc7_line_%d" % i: w for i, w in enumerate(widths)}
    # the expected rows: the same forward passes (decode_dataset's seed), searched directly
    torch.manual_seed(7)
    torch.cuda.manual_seed_all(7)
    want = []
    with torch.no_grad():
        for xb, _t, wb, _tl, meta in loader:
            out, lens = model(xb.cuda(), wb)
            hits = sp.search(out, lens, kws)
            for i in range(len(meta["utt-ids"])):
                for q, kw in enumerate(kws):
                    if hits.best_span[i, q, 0] >= 0:
                        want.append([meta["utt-ids"][i], kw, "%.6f" % hits.expected_count[i, q], "%.6f" % hits.best_logp[i, q]])
    assert [r[:4] for r in rows] == want and len(rows) >= 4 * (len(kws) - 1) and set(r[0] for r in rows) == set(wid)
    for uid, kw, count, logp, x0, x1 in rows:
        assert float(count) >= 0.0 and float(logp) < 0.0 and 0 <= int(x0) < int(x1) <= wid[uid]
    assert any(float(r[2]) >= 0.5 for r in rows)
    # a threshold keeps the rows at or above it, unchanged
    assert decode_dataset(model, loader, str(tmp_path / "kws5"), spotter=sp, keywords=kws, min_count=0.5) == 4
    rows5 = [l.split("\t") for l in open(tmp_path / "kws5" / "hyp-kws.tsv").read().splitlines()]
    assert rows5 == [r for r in rows if float(r[2]) >= 0.5]
    assert not os.path.exists(tmp_path / "default" / "hyp-kws.tsv")
