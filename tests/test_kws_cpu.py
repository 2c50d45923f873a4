"""CPU: the fp64 restatement of the CTC keyword search (tests/kws_ref.py) against a brute force over all frame paths, its identities
(both anchors = the CTC forward score; the four whole-word queries add up to the whole-word count), and the shape answers of
vocr_ctc_keyword_workspace_bytes / vocr_ctc_keyword_scores that need no device."""
import ctypes

import numpy as np
import pytest

from tests import align_ref as ar
from tests import kws_ref as kr

NEG = -np.inf

# (T, V, query, canon, lens, a column of -inf)
CASES = [
    (4, 3, [1], None, 4, None),
    (5, 3, [1, 1], None, 5, None),                # aa: needs its blank
    (6, 3, [1, 2, 1], None, 6, None),             # aba
    (6, 3, [1, 2, 2], None, 6, None),             # abb
    (6, 3, [2, 1], None, 4, None),                # lens < T
    (5, 4, [1, 3], [0, 1, 2, 1], 5, None),        # columns 1 and 3 are one class: "1 3" is a repeat
    (5, 4, [3, 2], [0, 1, 2, 1], 5, None),
    (5, 4, [1, 2], None, 5, 3),                   # a -inf column
    (5, 4, [3], None, 5, 3),                      # ... and a query on it
    (2, 3, [1, 1], None, 2, None),                # does not fit
]


def case_logits(i, T, V, dead=None):
    x = np.random.default_rng(100 + i).normal(0, 1.5, (T, V))
    if dead is not None:
        x[:, dead] = NEG
    return x


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_reference_against_brute_force(i, flags):
    T, V, query, canon, length, dead = CASES[i]
    x = case_logits(i, T, V, dead)
    count, best, span, margin = kr.brute_force(x[:length], query, flags, canon)
    got = kr.search(x[:, None, :], [length], [query], [flags], canon)
    lc, b, sp = got["log_count"][0, 0], got["best"][0, 0], tuple(int(v) for v in got["span"][0, 0])
    if count == NEG:
        assert lc == NEG and b == NEG and sp == (-1, -1)
        return
    assert abs(lc - count) <= 1e-12 * max(1.0, abs(count)), (lc, count)
    assert abs(b - best) <= 1e-12 * max(1.0, abs(best)), (b, best)
    assert margin > 1e-9 and sp == span, (sp, span, margin)
    assert got["gap"][0, 0] > 0


@pytest.mark.parametrize("flags", [4, 8, 12, 4 | 1, 8 | 2])
@pytest.mark.parametrize("i", [2, 3, 5, 6])
def test_trimmed_spans_against_brute_force(i, flags):
    """TRIM_START / TRIM_END: the same scores, the span without the first / last label's frames."""
    T, V, query, canon, length, dead = CASES[i]
    x = case_logits(i, T, V, dead)
    count, best, span, margin = kr.brute_force(x[:length], query, flags, canon)
    got = kr.search(x[:, None, :], [length], [query], [flags], canon)
    plain = kr.search(x[:, None, :], [length], [query], [flags & 3], canon)
    if len(query) < 3 and flags & 12 == 12:
        assert count == NEG and got["log_count"][0, 0] == NEG and tuple(got["span"][0, 0]) == (-1, -1)
        return
    assert got["log_count"][0, 0] == plain["log_count"][0, 0] and got["best"][0, 0] == plain["best"][0, 0]
    assert abs(got["log_count"][0, 0] - count) <= 1e-12 * max(1.0, abs(count))
    assert margin > 1e-9 and tuple(int(v) for v in got["span"][0, 0]) == span, (got["span"][0, 0], span)


def test_reference_edge_cases():
    x = case_logits(50, 5, 4)
    q = [[1, 2], [0], [4], [], [2, 0], [1]]
    got = kr.search(np.stack([x, x], axis=1), [5, 0], q, None, [0, 1, 2, 0])      # column 3 is in the blank's class
    assert np.isfinite(got["log_count"][0, 0]) and np.all(got["log_count"][0, 1:5] == NEG) and np.all(got["span"][0, 1:5] == -1)
    assert np.all(got["log_count"][1] == NEG) and np.all(got["best"][1] == NEG) and np.all(got["span"][1] == -1)
    assert kr.search(x[:, None], [5], [[3]], None, [0, 1, 2, 0])["log_count"][0, 0] == NEG
    y = x.copy()
    y[2] = NEG                                                                     # a whole -inf row: nothing crosses it
    got = kr.search(y[:, None], [5], [[1], [1, 2, 1, 2]])
    assert np.isfinite(got["log_count"][0, 0]) and got["log_count"][0, 1] == NEG and not np.isnan(got["best"]).any()
    # the tie rule: constant logits, spans (0,0) and (T-1,T-1) score alike, the earliest end wins
    got = kr.search(np.zeros((4, 1, 3)), [4], [[1]])
    assert tuple(got["span"][0, 0]) == (0, 0) and got["gap"][0, 0] == 0.0


@pytest.mark.parametrize("i", range(len(CASES)))
def test_both_anchors_are_the_ctc_forward_score(i):
    T, V, query, canon, length, dead = CASES[i]
    x = case_logits(i, T, V, dead)
    got = kr.search(x[:, None, :], [length], [query], [3], canon)
    want = ar.align(x, length, query, canon).ctc
    if want == NEG:
        assert got["log_count"][0, 0] == NEG
    else:
        assert abs(got["log_count"][0, 0] - want) <= 1e-12 * max(1.0, abs(want))


@pytest.mark.parametrize("query", [[1], [1, 2], [2, 2]])
def test_whole_word_is_the_sum_of_four_queries(query):
    T, V, sp = 6, 4, 3
    x = case_logits(70 + len(query), T, V)
    four = [[sp] + query + [sp], query + [sp], [sp] + query, query]
    got = kr.search(x[:, None, :], [T], four, [0, 1, 2, 3])["log_count"][0]
    want = kr.brute_force(x, query, 0, None, whole_word=sp)
    assert abs(np.logaddexp.reduce(got) - want) <= 1e-12 * max(1.0, abs(want)), (got, want)


def test_shape_answers_without_a_device():
    from vistaocr_amd import _lib, build
    build.build()
    lib = _lib.load()
    ws = lib.vocr_ctc_keyword_workspace_bytes
    assert ws(294, 32, 96, 1000, 12) > 0 and ws(294, 32, 96, 1, 128) > 0 and ws(1, 1, 2, 1, 1) > 0
    bad = [(294, 32, 1, 1000, 12), (294, 32, 257, 1000, 12), (294, 32, 96, 0, 12), (294, 32, 96, 1000, 129), (294, 32, 96, 1000, 0),
           (294, 32, 96, 1 << 18, 12)]                                             # the last: t * b * nq >= 2^31
    one = ctypes.c_void_p(16)
    for t, b, v, nq, ml in bad:
        assert ws(t, b, v, nq, ml) == 0, (t, b, v, nq, ml)
        rc = lib.vocr_ctc_keyword_scores(one, one, t, b, v, None, one, one, None, nq, max(ml, 1), ml, one, one, one, one, 1 << 30, None)
        assert rc == -1 and b"vocr_ctc_keyword_scores" in lib.vocr_last_error(), (t, b, v, nq, ml)
    # a null pointer, a stride below the longest query, a workspace that is too small: refused in front of any launch
    call = lambda *a: lib.vocr_ctc_keyword_scores(*a)
    assert call(None, one, 8, 2, 50, None, one, one, None, 3, 4, 4, one, one, one, one, 1 << 30, None) == -1
    assert call(one, one, 8, 2, 50, None, one, one, None, 3, 3, 4, one, one, one, one, 1 << 30, None) == -1
    assert call(one, one, 8, 2, 50, None, one, one, None, 3, 4, 4, one, one, one, one, 16, None) == -1
    assert b"workspace too small" in lib.vocr_last_error()
