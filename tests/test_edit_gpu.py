"""GPU: vocr_ctc_edit_scores (vistaocr_amd/csrc/ctc_edit.hip) through ops.ctc_edit_scores, CtcAligner.alternatives, the decoders'
decode_alternatives and decode_dataset(..., alternatives=k), against the fp64 restatement (tests/edit_ref.py, itself held to the forward
score of every edited labelling by tests/test_edit_cpu.py), the alignment and loss kernels, and itself (determinism).

EVERY entry of all four outputs is compared: -inf exactly where the reference is -inf and nowhere else, never NaN, and a finite entry
within the project's worst-case bound of tests/test_align_gpu.py applied to the fp64 value of that entry,
    eps_line(T, score) = 4 * T * 2^-24 * max(|score|, 1):
any single path of an edited labelling still has T frames, split between the alpha side and the beta side, so the same linear bound on
the fp32 rounding holds.  The data comes from tests/beam_data.py and align_ref.greedy_labels, not from the code under test.  Each test
prints the largest difference it saw and the largest fraction of the bound used (profiles/ctc_edit_errors.txt)."""
import os

import numpy as np
import pytest
import torch

import vistaocr_amd as va
from tests import align_ref as ar
from tests import beam_data as bd
from tests import edit_ref as er
from tests.test_align_gpu import _loss_case, _loss_nll, _tiny_model
from tests.test_edit_cpu import CASES, case_logits
from vistaocr_amd import ops

pytestmark = pytest.mark.gpu

T1, B1, V1 = 294, 32, 96           # configs[1]'s logits shape
NEG = -np.inf


def eps_line(T, score):
    return 4.0 * T * 2.0 ** -24 * np.maximum(np.abs(score), 1.0)


def _pack(labels):
    B, n = len(labels), max(len(h) for h in labels)
    M = max([len(l) for h in labels for l in h] + [1])
    lab = np.zeros((B, n, M), dtype=np.int32)
    ln = np.full((B, n), -1, dtype=np.int32)
    for b, h in enumerate(labels):
        for q, l in enumerate(h):
            lab[b, q, :len(l)] = l
            ln[b, q] = len(l)
    return lab, ln


def _run(x, lens, labels, canon=None):
    """x [T,B,V]; labels: per line a list of labellings (the n axis).  Returns host (ctc [B,n], sub [B,n,M,V], dele [B,n,M], ins)."""
    lab, ln = _pack(labels)
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda() if canon is not None else None
    out = ops.ctc_edit_scores(xd, lens, torch.from_numpy(lab).cuda(), torch.from_numpy(ln).cuda(), cd)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _expected(x, lens, labels, canon, M, fn=er.edit_scores):
    """The reference's four arrays in the kernel's layout: -inf beyond every labelling's length and for a rank that is not there."""
    T, B, V = x.shape
    n = max(len(h) for h in labels)
    ctc, sub = np.full((B, n), NEG), np.full((B, n, M, V), NEG)
    dele, ins = np.full((B, n, M), NEG), np.full((B, n, M + 1, V), NEG)
    for b, h in enumerate(labels):
        for q, l in enumerate(h):
            if l is None or len(l) > M:
                continue
            ref = fn(x[:, b].astype(np.float64), lens[b], l, canon)
            L = len(l)
            ctc[b, q], sub[b, q, :L], dele[b, q, :L], ins[b, q, :L + 1] = ref.ctc, ref.sub, ref.dele, ref.ins
    return ctc, sub, dele, ins


def _check(got, want, T, name):
    """Every entry.  Returns (largest difference, largest fraction of its bound) over the finite ones."""
    worst, frac, finite = 0.0, 0.0, 0
    for part, g, w in zip(("ctc", "sub", "del", "ins"), got, want):
        g = g.astype(np.float64)
        assert g.shape == w.shape, (name, part, g.shape, w.shape)
        assert not np.isnan(g).any() and not np.any(g == np.inf), (name, part)
        mism = np.isneginf(g) != np.isneginf(w)
        assert not mism.any(), (name, part, "-inf mismatch at", np.argwhere(mism)[:5].tolist(), g[mism][:5], w[mism][:5])
        fin = np.isfinite(w)
        if fin.any():
            d = np.abs(g[fin] - w[fin])
            r = d / eps_line(T, w[fin])
            k = int(np.argmax(r))
            worst, frac, finite = max(worst, float(d.max())), max(frac, float(r.max())), finite + int(fin.sum())
            assert r.max() <= 1.0, (name, part, "entry", np.argwhere(fin)[k].tolist(), "got", g[fin][k], "fp64", w[fin][k], "bound",
                                    eps_line(T, w[fin][k]))
    print("edit-errors %-34s T %4d  finite entries %8d  max |diff| %.3g  max diff/bound %.3f" % (name, T, finite, worst, frac))
    return worst, frac


def _compare(x, lens, labels, canon, name, fn=er.edit_scores):
    x = np.ascontiguousarray(x, dtype=np.float32)               # the reference sees the logits the kernel sees
    got = _run(x, lens, labels, canon)
    return _check(got, _expected(x, lens, labels, canon, got[1].shape[2], fn), x.shape[0], name)


@pytest.fixture(scope="module")
def english():
    al = va.english_alphabet()
    canon = np.array(al.canonical_indices())
    return al, canon, np.nonzero(canon == np.arange(len(al)))[0][1:]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_small_exact_cases(i):
    """The cases of tests/test_edit_cpu.py against the DIRECT definition: the fp64 forward score of every edited labelling."""
    T, V, length, labels, canon, what = CASES[i]
    x = case_logits(i)[:, None, :]
    _compare(x, [length], [[labels]], canon, "exact case %d" % i, fn=er.direct_scores)


def test_small_cases_in_one_batch():
    """Lines of different lengths, labellings of different lengths and validity in ONE call (n = 3, a rank that is not there)."""
    rng = np.random.default_rng(41)
    T, B, V = 9, 6, 6
    x = rng.normal(0, 1.5, (T, B, V))
    x[4, 2, :] = NEG
    x[:, 3, 2] = NEG
    lens = [9, 0, 9, 7, 3, 1]
    labels = [[[1, 2, 3], [], [5, 5]], [[], [1]], [[2, 2, 4, 1], [3]], [[1, 2], [2, 1, 2], [4]], [[1, 1, 1], [2, 3], [6]], [[2], [1, 2], []]]
    _compare(x, lens, labels, [0, 1, 2, 3, 3, 5], "mixed batch", fn=er.direct_scores)


@pytest.mark.parametrize("p_char", [0.35, 0.10])
@pytest.mark.parametrize("seed", [7, 11])
def test_bench_shape_peaky(seed, p_char):
    """T = 294, B = 32, V = 96, greedy labels: L 43-67 at p_char 0.35 (the lattice kernel's LDS-row path), 5-24 at 0.10 (one wave)."""
    x = bd.peaky_logits(np.random.default_rng(seed), T1, B1, V1, p_char=p_char)
    labels = [[ar.greedy_labels(x[:, b], T1)] for b in range(B1)]
    lo, hi = min(len(h[0]) for h in labels), max(len(h[0]) for h in labels)
    print("peaky seed %d p_char %.2f: L %d-%d" % (seed, p_char, lo, hi))
    assert (lo > 32) if p_char == 0.35 else (hi <= 31)
    _compare(x, [T1] * B1, labels, None, "peaky seed %d p_char %.2f" % (seed, p_char))


@pytest.mark.parametrize("T", [64, T1])
@pytest.mark.parametrize("seed", [7, 11])
def test_dense_with_the_english_classes(seed, T, english):
    """N(0,1) logits, the whole greedy labelling of every line (about one label per frame), the English alphabet's classes: every edit
    has a finite score unless a repeated class leaves no room for its blank."""
    al, canon, cls = english
    B = B1 if T == 64 else 8                                    # the fp64 reference takes over a second per line at T = 294
    x = np.random.default_rng(seed).normal(0, 1, (T, B, V1)).astype(np.float32)
    labels = [[ar.greedy_labels(x[:, b], T)] for b in range(B)]
    _compare(x, [T - (b % 5) for b in range(B)], labels, canon, "dense seed %d T %d" % (seed, T))


def test_dense_short_labellings():
    """N(0,1) logits at T = 294 with the first 60 and the first 20 greedy labels (n = 2): scores near -1300, every entry finite."""
    x = np.random.default_rng(13).normal(0, 1, (T1, 8, V1)).astype(np.float32)
    labels = [[ar.greedy_labels(x[:, b], T1)[:60], ar.greedy_labels(x[:, b], T1)[:20]] for b in range(8)]
    _compare(x, [T1 - 7 * b for b in range(8)], labels, None, "dense 60 and 20 labels")


def test_nbest_from_the_beam_search_on_the_device(english):
    """The [B, 4, T] labels of a K = 16 search go in as they are (label_stride = T, so M = T)."""
    al, canon, cls = english
    x = bd.peaky_logits(np.random.default_rng(7), T1, B1, V1, classes=cls)
    xd = torch.from_numpy(x).cuda()
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda()
    lab, ln, bsc = ops.ctc_beam_search(xd, [T1] * B1, cd, 16, 4)
    got = ops.ctc_edit_scores(xd, [T1] * B1, lab, ln, cd)
    torch.cuda.synchronize()
    got = [g.cpu().numpy() for g in got]
    assert got[1].shape == (B1, 4, T1, V1) and got[3].shape == (B1, 4, T1 + 1, V1)
    lab, ln = lab.cpu().numpy(), ln.cpu().numpy()
    labels = [[[int(v) for v in lab[b, q, :ln[b, q]]] if 0 <= ln[b, q] <= T1 else None for q in range(4)] for b in range(B1)]
    assert sum(l is not None and len(l) > 0 for h in labels for l in h) >= 3 * B1
    _check(got, _expected(x, [T1] * B1, labels, canon, T1), T1, "4-best of a K = 16 search")


def _align_fwd(x, lens, labels, canon=None):
    lab, ln = _pack([[l] for l in labels])
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda() if canon is not None else None
    sc, _, _ = ops.ctc_align(xd, lens, torch.from_numpy(lab).cuda(), torch.from_numpy(ln).cuda(), cd)
    return sc.cpu().numpy()[:, 0, 1]


@pytest.mark.parametrize("name", ["peaky", "dense", "ragged"])
def test_unedited_score_equals_the_alignment_and_the_loss_kernel(name):
    """out_ctc, and out_sub at the label's own column, are ln P_ctc(labels | x): each within eps_line of fp64, hence within 2 eps_line
    of vocr_ctc_align's forward score and of -nll of vocr_ctc_loss_grad (fp32 sums in different orders); +-inf must match exactly."""
    x, lens, labels = _loss_case(name)
    T, B = x.shape[0], x.shape[1]
    nll = _loss_nll(x, lens, labels)
    fwd = _align_fwd(x, lens, labels)
    ctc, sub, dele, ins = _run(x, lens, [[l] for l in labels])
    finite, worst = 0, 0.0
    for b in range(B):
        ref = ar.align(x[:, b], lens[b], labels[b]).ctc
        own = [sub[b, 0, p, v] for p, v in enumerate(labels[b])]
        print("line %d: edit %r own column %r..%r align %r -nll %r fp64 %r" % (b, ctc[b, 0], min(own + [np.inf]), max(own + [NEG]), fwd[b],
                                                                              -nll[b], ref))
        if ref == NEG:
            assert ctc[b, 0] == NEG and fwd[b] == NEG and nll[b] == np.inf and all(v == NEG for v in own), b
            continue
        finite += 1
        eps = eps_line(T, ref)
        for v in [ctc[b, 0]] + own:
            assert abs(v - ref) <= eps and abs(v - fwd[b]) <= 2 * eps and abs(v + nll[b]) <= 2 * eps, (b, v, ref, fwd[b], -nll[b])
            worst = max(worst, abs(v - fwd[b]), abs(v + nll[b]))
    print("edit-errors %-34s T %4d  largest |edit - align|, |edit + nll| %.3g" % ("consistency " + name, T, worst))
    assert finite >= 4


def test_columns_of_one_class_are_bit_equal_and_runs_are_bit_identical(english):
    al, canon, cls = english
    x = np.random.default_rng(13).normal(0, 1, (T1, B1, V1)).astype(np.float32)
    labels = [[ar.greedy_labels(x[:, b], T1)[:60], ar.greedy_labels(x[:, b], T1)[:20]] for b in range(B1)]
    lens = [T1 - b for b in range(B1)]
    a = _run(x, lens, labels, canon)
    b = _run(x, lens, labels, canon)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    merged = [v for v in range(V1) if canon[v] != v]
    assert merged
    for v in merged:
        c = int(canon[v])
        if c == 0:
            assert np.all(a[1][..., v] == NEG) and np.all(a[3][..., v] == NEG)
        else:
            assert a[1][..., v].tobytes() == a[1][..., c].tobytes() and a[3][..., v].tobytes() == a[3][..., c].tobytes()
            assert np.isfinite(a[1][..., v]).any()
    assert np.all(a[1][..., 0] == NEG) and np.all(a[3][..., 0] == NEG)


def test_edge_shapes(english):
    """Ragged lines with labellings that do not fit, S = 63 and S = 65 next to each other in one call, an empty second rank, B = 1."""
    al, canon, cls = english
    rng = np.random.default_rng(21)
    T, V = 40, V1
    x = rng.normal(0, 1, (T, 7, V)).astype(np.float32)
    g = [ar.greedy_labels(x[:, b], T) for b in range(7)]
    _compare(x, [0, 1, 40, 17, 2, 39, 33], [[g[b][:6]] for b in range(7)], None, "ragged, 6 labels")
    _compare(x, [0, 0, T, 3, T, T, T], [[[]], [g[1][:3]], [[]], [g[3][:9]], [[5, V, 7]], [[5, 0, 7]], [[-3]]], None, "empty and invalid")
    _compare(x[:, :1], [T], [[g[0][:10]]], canon, "B = 1")
    w = bd.peaky_logits(np.random.default_rng(12), 200, 4, V, p_char=0.4)
    want = [None, 31, 32, 7]
    wl = [200 if k is None else next(n for n in range(200) if len(ar.greedy_labels(w[:, b], n)) == k) for b, k in enumerate(want)]
    gl = [ar.greedy_labels(w[:, b], wl[b]) for b in range(4)]
    assert [len(l) for l in gl[1:]] == want[1:] and len(gl[0]) > 32
    _compare(w, wl, [[l, []] for l in gl], None, "S = 63, 65, 15 and > 64")
    _compare(w, wl, [[gl[(b + 1) % 4], gl[b]] for b in range(4)], None, "another line's labelling")


# ---- planted errors -------------------------------------------------------------------------------------------------------------

PLANT_SEED, PLANT_TOL, PLANT_EPS = 7, 0.05, 0.02


def planted_cases(x, canon, classes, per_line=4):
    """fp64 only.  For every line of peaky logits x: its greedy labelling g, aligned by the reference; positions p whose span holds a
    frame with a competitor class c' (a finite logit; not the blank, not g[p]'s class, not a neighbour's class, so no repeat appears).
    The planted labelling is g with g[p] replaced by c'.  A position is DECIDED when, in the reference's posteriors of the planted
    labelling at p, the original class is the most probable outcome other than keeping c', its posterior exceeds the next one's by more
    than PLANT_TOL, and eps_line of both scores is at most PLANT_EPS: a raw score within eps_line <= 0.02 of fp64 moves a posterior by
    at most a factor e^(2 * 0.02) - 1 = 4.1 % of itself, two posteriors sum to at most 1, so a gap above 0.05 survives.
    Returns per line a list of (planted labelling, p, original class, decided)."""
    T, B, V = x.shape
    cls = ar.classes_of(V, canon)
    out = []
    for b in range(B):
        g = ar.greedy_labels(x[:, b], T)
        al = ar.align(x[:, b], T, g, canon)
        row = []
        if al.spans is not None:
            for p in range(len(g)):
                if len(row) == per_line:
                    break
                near = {int(cls[g[k]]) for k in (p - 1, p, p + 1) if 0 <= k < len(g)}
                comp = [int(c) for t in range(al.spans[p, 0], al.spans[p, 1] + 1) for c in classes
                        if np.isfinite(x[t, b, c]) and int(cls[c]) not in near]
                if not comp:
                    continue
                planted = g[:p] + [comp[0]] + g[p + 1:]
                ref = er.edit_scores(x[:, b].astype(np.float64), T, planted, canon)
                ch, _ = er.posteriors(ref, planted, canon, V)
                others = ch[p].copy()
                others[cls[comp[0]]] = -1.0
                order = np.argsort(-others)
                orig = int(cls[g[p]])
                s1 = ref.sub[p, order[0]] if order[0] < V else ref.dele[p]
                s2 = ref.sub[p, order[1]] if order[1] < V else ref.dele[p]
                decided = bool(order[0] == orig and others[order[0]] - others[order[1]] > PLANT_TOL
                               and eps_line(T, s1) <= PLANT_EPS and (not np.isfinite(s2) or eps_line(T, s2) <= PLANT_EPS))
                row.append((planted, p, orig, decided))
        out.append(row)
    return out


def test_planted_errors_rank_the_original_character_first(english):
    """One character of the greedy transcript replaced by a competitor of one of its frames: alternatives() must name the original
    character as the first alternative there, on every position the fp64 reference decides (128 of 128 at this seed; >= 20 asserted)."""
    al, canon, cls = english
    x = bd.peaky_logits(np.random.default_rng(PLANT_SEED), T1, B1, V1, classes=cls)
    cases = planted_cases(x, canon, cls)
    decided = sum(c[3] for row in cases for c in row)
    print("planted errors: %d positions, %d decided by the fp64 reference" % (sum(len(r) for r in cases), decided))
    assert decided >= 20
    lines = [b for b in range(B1) if cases[b]]
    xd = torch.from_numpy(np.ascontiguousarray(x[:, lines])).cuda()
    got = va.CtcAligner(al).alternatives(xd, [T1] * len(lines), [[(c[0], None) for c in cases[b]] for b in lines], topk=3)
    for row, b in zip(got, lines):
        assert len(row) == len(cases[b])
        for la, (planted, p, orig, ok) in zip(row, cases[b]):
            assert la is not None and [c.label for c in la.chars] == planted
            if ok:
                c = la.chars[p]
                assert c.alternatives and c.alternatives[0][0] == al.idx_to_char[orig], (b, p, c, al.idx_to_char[orig])


# ---- host arithmetic ------------------------------------------------------------------------------------------------------------

class _Raw(object):
    def __init__(self, ctc, sub, dele, ins):
        self.ctc, self.sub, self.dele, self.ins = ctc, sub, dele, ins


def _check_alternatives(lines, labels, raw, canon, al, topk, name):
    """`lines`: LineAlternatives per line; `raw`: the kernel's own host arrays for `labels` (n = 1).  Posteriors recomputed in fp64 from
    the raw scores must agree to 1e-6, and the alternatives must be the top-k in order wherever neighbours differ by more than that."""
    V = len(canon)
    cls = ar.classes_of(V, canon)
    worst, checked = 0.0, 0
    for b, (la, lab) in enumerate(zip(lines, labels)):
        if la is None:
            continue
        L = len(lab)
        assert len(la.chars) == L and len(la.gaps) == L + 1 and la.ctc_logp == float(raw[0][b, 0])
        ch, gp = er.posteriors(_Raw(raw[0][b, 0], raw[1][b, 0], raw[2][b, 0], raw[3][b, 0]), lab, canon, V)
        for p in range(L + 1):
            groups = [(gp[p, :V].copy(), la.gaps[p][1])]
            assert abs(la.gaps[p][0] - gp[p, V]) <= 1e-6, (name, b, p)
            if p < L:
                c, own = la.chars[p], cls[lab[p]]
                assert c.uxxxx == al.idx_to_char[lab[p]] and abs(c.posterior - ch[p, own]) <= 1e-6, (name, b, p, c, ch[p, own])
                worst = max(worst, abs(c.posterior - ch[p, own]))
                others = ch[p].copy()
                others[own] = -1.0
                groups.append((others, c.alternatives))
            for others, got in groups:
                order = np.argsort(-others, kind="stable")[:topk]
                assert len(got) <= topk
                assert len(got) == int(np.sum(others[order] > 0)) or any(0 < others[k] < 1e-38 for k in order), (name, b, p, got)
                for r, (ux, post) in enumerate(got):
                    assert abs(post - others[order[r]]) <= 1e-6, (name, b, p, r, got, others[order])
                    worst = max(worst, abs(post - others[order[r]]))
                    tied = any(k != order[r] and abs(others[k] - others[order[r]]) <= 1e-6 for k in range(len(others)))
                    if not tied:
                        assert ux == (None if order[r] == V else al.idx_to_char[int(order[r])]), (name, b, p, r, got)
                    checked += 1
    print("alternatives %s: %d ranked outcomes checked, largest posterior difference %.3g" % (name, checked, worst))
    return checked


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


def _raw_for(xd, lens, labels, canon):
    lab, ln = _pack([[l] for l in labels])
    out = ops.ctc_edit_scores(xd, lens, torch.from_numpy(lab).cuda(), torch.from_numpy(ln).cuda(), torch.as_tensor(canon, dtype=torch.int32).cuda())
    return [o.cpu().numpy() for o in out]


def test_alternatives_are_the_softmax_of_the_raw_scores(english, word_lm):
    al, canon, cls = english
    x = bd.peaky_logits(np.random.default_rng(7), T1, B1, V1, classes=cls)
    x[:, :, 0] = np.where(np.isinf(x[:, :, 0]), x.max(axis=2) - 30.0, x[:, :, 0])     # a blank is always possible
    y = np.random.default_rng(5).normal(0, 1, (64, B1, V1)).astype(np.float32)
    aligner = va.CtcAligner(al)
    for name, data, T in (("peaky", x, T1), ("dense", y, 64)):
        xd = torch.from_numpy(data).cuda()
        lens = [T - 3 * (b % 7) for b in range(B1)]
        labels = [ar.greedy_labels(data[:, b], lens[b])[:40] for b in range(B1)]
        raw = _raw_for(xd, lens, labels, canon)
        for k in (1, 3):
            lines = aligner.alternatives(xd, lens, labels, topk=k)
            assert _check_alternatives(lines, labels, raw, canon, al, k, "aligner %s topk %d" % (name, k)) > 100
        as_strings = aligner.alternatives(xd, lens, [" ".join(al.idx_to_char[v] for v in l) for l in labels], topk=3)
        assert [[c[1:] for c in a.chars] for a in as_strings] == [[c[1:] for c in a.chars] for a in lines]
        for dec in (va.ArgmaxDecoder(al), va.BeamDecoder(al, beam=16)):
            hyps, lines = dec.decode_alternatives(xd, lens, 3, uxxxx=True)
            assert hyps == dec.decode(xd, lens, uxxxx=True) and dec.decode_alternatives(xd, lens)[0] == dec.decode(xd, lens)
            labels_d = [[al.char_to_idx[t] for t in h.split()] for h in hyps]
            assert all(a is not None for a in lines)
            raw_d = _raw_for(xd, lens, labels_d, canon)
            assert _check_alternatives(lines, labels_d, raw_d, canon, al, 3, "%s %s" % (type(dec).__name__, name)) > 100
    lm, xs, slens = word_lm
    wdec = va.WordBeamDecoder(al, lm, beam=16, lm_weight=0.8)
    xsd = torch.from_numpy(xs).cuda()
    hyps, lines = wdec.decode_alternatives(xsd, slens, 3, uxxxx=True)
    assert hyps == wdec.decode(xsd, slens, uxxxx=True)
    none = [h[0] if h else None for h in wdec.decode_nbest(xsd, slens, 1)]
    assert [a is None for a in lines] == [h is None for h in none] and sum(a is not None for a in lines) >= len(lines) - 2
    labels_w = [[al.char_to_idx[t] for t in h.split()] for h in hyps]
    raw_w = _raw_for(xsd, slens, labels_w, canon)
    assert _check_alternatives(lines, labels_w, raw_w, canon, al, 3, "WordBeamDecoder") > 100


def test_decode_dataset_writes_alternative_rows(tmp_path):
    from vistaocr_amd.loop import SortByWidthCollater, decode_dataset
    al = va.english_alphabet()
    model = _tiny_model(al)
    r = np.random.RandomState(0)
    items = [(torch.from_numpy(r.uniform(0, 1, size=(1, 30, w)).astype(np.float32)), [1], {"width": w, "utt-id": "doc7_line_%d" % i})
             for i, w in enumerate([140, 96, 201, 64])]
    loader = [SortByWidthCollater(items[:2]), SortByWidthCollater(items[2:])]
    assert decode_dataset(model, loader, str(tmp_path / "default")) == 4
    assert sorted(os.listdir(tmp_path / "default")) == ["hyp-chars.txt", "hyp-chars.txt.utf8"]
    assert decode_dataset(model, loader, str(tmp_path / "words"), aligner=va.CtcAligner(al)) == 4
    assert sorted(os.listdir(tmp_path / "words")) == ["hyp-chars.txt", "hyp-chars.txt.utf8", "hyp-words.tsv"]
    for name, kw in (("alt", {}), ("alt_beam", {"decoder": va.BeamDecoder(al, beam=8)}), ("alt_words", {"aligner": va.CtcAligner(al)})):
        d = tmp_path / name
        assert decode_dataset(model, loader, str(d), alternatives=2, **kw) == 4
        assert sorted(os.listdir(d)) == ["hyp-chars-alt.tsv", "hyp-chars.txt", "hyp-chars.txt.utf8"] + (["hyp-words.tsv"] if "aligner" in kw else [])
        if "decoder" not in kw:                                                       # the files of the default call, byte for byte
            for f in ("hyp-chars.txt", "hyp-chars.txt.utf8"):
                assert open(d / f, "rb").read() == open(tmp_path / "default" / f, "rb").read()
        if "aligner" in kw:
            assert open(d / "hyp-words.tsv", "rb").read() == open(tmp_path / "words" / "hyp-words.tsv", "rb").read()
        rows = [l.split("\t") for l in open(d / "hyp-chars-alt.tsv").read().splitlines()]
        want = []
        for line in open(d / "hyp-chars.txt").read().splitlines():
            ux, uid = line.rsplit(" (", 1)
            want += [(uid.rstrip(")"), str(p), tok) for p, tok in enumerate(ux.split())]
        assert [tuple(r[:3]) for r in rows if r[2] != "<gap>"] == want and len(want) > 0
        for r in rows:
            post = float(r[3])
            alts = [a.rsplit(":", 1) for a in r[4:]]
            assert 0.0 <= post <= 1.0 and len(alts) <= 2 and all(0.0 < float(v) <= 1.0 for _, v in alts)
            assert [float(v) for _, v in alts] == sorted([float(v) for _, v in alts], reverse=True)
            assert post + sum(float(v) for _, v in alts) <= 1.0 + 1e-5
            if r[2] == "<gap>":
                assert r[1].startswith("^") and int(r[1][1:]) >= 0 and post < 0.5 and all(u in al.char_to_idx for u, _ in alts)
            else:
                assert all(u == "<del>" or (u in al.char_to_idx and u != r[2]) for u, _ in alts)


def test_unsupported_shapes_fail_before_any_launch():
    x = torch.zeros(8, 2, 300, device="cuda")
    lab = torch.ones(2, 3, dtype=torch.int32, device="cuda")
    ln = torch.full((2,), 3, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="ctc_edit_scores"):
        ops.ctc_edit_scores(x, [8, 8], lab, ln)                                       # V > 256
    with pytest.raises(RuntimeError, match="ctc_edit_scores"):
        ops.ctc_edit_scores(x[:, :, :50], [8, 8], lab.float(), ln)
    with pytest.raises(RuntimeError, match="ctc_edit_scores"):
        ops.ctc_edit_scores(x[:, :, :50].contiguous(), [8, 8], lab.unsqueeze(1).expand(2, 129, 3).contiguous(), ln.unsqueeze(1).expand(2, 129))
    with pytest.raises(RuntimeError, match="ctc_edit_scores"):
        ops.ctc_edit_scores(x[:, :, :50].contiguous(), [8, 8, 8], lab, ln)
    with pytest.raises(RuntimeError, match="ctc_edit_scores"):                        # 128 labellings of stride T = 4000: 32 GB of lattices
        ops.ctc_edit_scores(torch.zeros(4000, 1, 50, device="cuda"), [4000], torch.ones(1, 128, 4000, dtype=torch.int32, device="cuda"),
                            torch.ones(1, 128, dtype=torch.int32, device="cuda"))
    ctc, sub, dele, ins = ops.ctc_edit_scores(x[:, :, :50].contiguous(), [8, 8], lab, ln)   # 2-d labels: no n axis in the outputs
    assert tuple(ctc.shape) == (2,) and tuple(sub.shape) == (2, 3, 50) and tuple(dele.shape) == (2, 3) and tuple(ins.shape) == (2, 4, 50)
    assert np.isfinite(ctc.cpu().numpy()).all()                                        # 1 1 1 needs 5 frames and has 8
