"""CPU: the fp64 restatement of the CTC aligner (tests/align_ref.py) against a brute force over all frame labellings, the host side of
vistaocr_amd.align (words(), pixel_spans()), and vocr_ctc_align's argument validation through the C-ABI without a device."""
import math

import numpy as np
import pytest

import vistaocr_amd as va
from tests import align_ref as ar
from vistaocr_amd import _lib
from vistaocr_amd.align import CharAlignment, CtcAligner, LineAlignment
from vistaocr_amd.textutils import form_tokenized_words

# (T, V, labels, canon): <= 6 frames, <= 3 classes besides the blank.  A repeated label, a merged class (columns 2 and 3 are one symbol,
# labelled once by each member), the empty labelling, an infeasible one (a repeat needs a blank: 3 frames for 2 labels), -inf columns.
EXACT = [
    (5, 3, [1, 2], None),
    (6, 3, [1, 1], None),
    (6, 4, [2, 1, 2], None),
    (5, 4, [1, 3], [0, 1, 2, 2]),
    (5, 4, [2, 3], [0, 1, 2, 2]),
    (6, 4, [3, 1, 2], [0, 1, 2, 2]),
    (4, 3, [], None),
    (2, 3, [1, 1], None),
    (3, 3, [1, 2, 1, 2], None),
    (6, 4, [1, 2, 3], None),
]


def exact_logits(i, T, V):
    rng = np.random.default_rng(100 + i)
    x = rng.normal(0, 1.5, size=(T, V))
    if i % 3 == 0:
        x[rng.integers(T), 1 + rng.integers(V - 1)] = -np.inf          # -inf logits are legal inputs
    return x


@pytest.mark.parametrize("i", range(len(EXACT)))
def test_reference_against_brute_force(i):
    T, V, labels, canon = EXACT[i]
    x = exact_logits(i, T, V)
    best, spans, total, margin = ar.brute_force(x, labels, canon)
    got = ar.align(x, T, labels, canon)
    if best == -np.inf:
        assert got.viterbi == -np.inf and got.ctc == -np.inf and got.spans is None
        return
    assert abs(got.viterbi - best) <= 1e-12 * abs(best) + 1e-12
    assert abs(got.ctc - total) <= 1e-12 * abs(total) + 1e-12
    assert got.ctc >= got.viterbi
    assert margin > 1e-9                                              # the seeds have a unique best path: its spans are testable
    assert np.array_equal(got.spans, spans)
    _, cls = ar.class_logprobs(x, canon)
    assert ar.path_is_valid(got.path, labels, cls)
    assert ar.path_from_spans(got.spans, T, len(labels)) == got.path
    clp, _ = ar.class_logprobs(x, canon)
    assert abs(ar.path_score(clp, labels, got.path) - got.viterbi) <= 1e-12 * abs(best) + 1e-12
    for p in range(len(labels)):
        seg = clp[spans[p, 0]:spans[p, 1] + 1, labels[p]]
        assert got.label_scores[p, 0] == np.max(seg) and abs(got.label_scores[p, 1] - np.sum(seg)) < 1e-12


def test_reference_edge_cases():
    x = np.random.default_rng(0).normal(size=(5, 4))
    clp, _ = ar.class_logprobs(x)
    a = ar.align(x, 5, [])
    assert abs(a.viterbi - np.sum(clp[:, 0])) < 1e-12 and a.ctc == a.viterbi and a.spans.shape == (0, 2)
    a = ar.align(x, 0, [])
    assert a.viterbi == 0.0 and a.ctc == 0.0
    assert ar.align(x, 0, [1]).spans is None
    assert ar.align(x, 5, [4]).viterbi == -np.inf and ar.align(x, 5, [0]).viterbi == -np.inf and ar.align(x, 5, [-1]).spans is None
    assert ar.align(x, 2, [1, 1]).viterbi == -np.inf                  # a repeat needs len >= L + repeats
    a = ar.align(x, 3, [1, 1])                                        # ... and at that length every step is forced
    assert a.path == [1, 2, 3] and a.gap == np.inf and np.array_equal(a.spans, [[0, 0], [2, 2]])
    y = x.copy()
    y[:, 2] = -np.inf
    assert ar.align(y, 5, [1, 2]).viterbi == -np.inf                  # a class the frames give -inf
    tie = np.zeros((3, 2))                                            # every path ties: stay first, and the final blank at the end
    a = ar.align(tie, 3, [1])
    assert a.gap == 0.0 and a.path == [1, 2, 2]
    assert ar.greedy_labels(np.array([[0, 1.0, 0], [0, 1.0, 0], [1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]), 5) == [1, 1, 2]


def _line(toks, frames):
    return LineAlignment(-1.0, -0.5, [CharAlignment(i + 1, t, f0, f1, pk, mean) for i, (t, (f0, f1, pk, mean)) in enumerate(zip(toks, frames))])


def test_words_follow_form_tokenized_words():
    al = CtcAligner(va.english_alphabet())
    toks = "u0020 u0061 u0062 u0020 u0020 u0063 u002c u0064 u0031 u0032 u0020".split()
    frames = [(2 * i, 2 * i + (i % 2), -0.1 * (i + 1), -0.2 * (i + 1)) for i in range(len(toks))]
    line = _line(toks, frames)
    words = al.words(line)
    assert [w.token for w in words] == form_tokenized_words(toks) == ["u0061_u0062", "u0063", "u002c", "u0064", "u0031", "u0032"]
    w = words[0]                                                      # characters 1 and 2: frames [2,3] and [4,4]
    assert (w.first_frame, w.last_frame) == (2, 4)
    assert w.min_conf == pytest.approx(math.exp(-0.3))
    assert w.mean_logp == pytest.approx((2 * -0.4 + 1 * -0.6) / 3)
    assert (words[2].first_frame, words[2].last_frame) == (12, 12) and words[2].min_conf == pytest.approx(math.exp(-0.7))
    assert al.words(_line([], [])) == [] and al.words(_line(["u0020"], [(0, 0, -1.0, -1.0)])) == []
    rng = np.random.default_rng(5)
    pool = "u0061 u0062 u0020 u002e u0035 u007a".split()
    for _ in range(20):
        toks = [pool[k] for k in rng.integers(len(pool), size=int(rng.integers(1, 15)))]
        line = _line(toks, [(i, i, -0.5, -0.5) for i in range(len(toks))])
        assert [w.token for w in al.words(line)] == form_tokenized_words(toks)


def test_pixel_spans_arithmetic():
    al = CtcAligner(va.english_alphabet())
    line = _line(["u0061", "u0062", "u0063"], [(0, 0, 0, 0), (3, 7, 0, 0), (293, 293, 0, 0)])
    assert al.pixel_spans(line, 600, 294) == [(0, 3), (6, 17), (597, 600)]        # floor(3*600/294) = 6, ceil(8*600/294) = 17
    assert al.pixel_spans(line.chars[1:2], 294, 294) == [(3, 8)]
    for w, n in ((600, 294), (97, 13), (64, 64), (1201, 576)):
        for first in range(0, n, 7):
            for last in range(first, min(first + 5, n)):
                (x0, x1), = al.pixel_spans([CharAlignment(1, "u0061", first, last, 0, 0)], w, n)
                assert x0 == math.floor(first * w / n) and x1 == math.ceil((last + 1) * w / n) and 0 <= x0 < x1 <= w


def test_c_abi_validation_without_a_device():
    lib = _lib.load()
    assert lib.vocr_ctc_align_workspace_bytes(294, 32, 96, 1, 31) > 0
    assert lib.vocr_ctc_align_workspace_bytes(294, 32, 96, 4, 294) > 0           # the beam searches' layout: label_stride = T
    assert lib.vocr_ctc_align_workspace_bytes(294, 32, 257, 1, 31) == 0
    assert lib.vocr_ctc_align_workspace_bytes(294, 32, 96, 129, 31) == 0
    assert lib.vocr_ctc_align_workspace_bytes(294, 32, 96, 1, 295) == 0          # a labelling longer than the line
    assert lib.vocr_ctc_align_workspace_bytes(0, 32, 96, 1, 0) == 0
    small, big = lib.vocr_ctc_align_workspace_bytes(4000, 2, 96, 1, 1663), lib.vocr_ctc_align_workspace_bytes(4000, 2, 96, 1, 4000)
    assert 0 < small < big                                                       # beyond 1663 labels the rows move to the workspace
    rc = lib.vocr_ctc_align(None, None, 294, 32, 96, None, None, None, 1, 31, 31, None, None, None, None, 0, None)
    assert rc == -1 and b"vocr_ctc_align" in lib.vocr_last_error()
    assert "CtcAligner" in va.__all__
