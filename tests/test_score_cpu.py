"""CPU: the reference of the edit statistics (tests/score_ref.py) against the package's own host metric (textutils.edit_distance,
compute_cer_wer), its two forms against each other, the known answer of the reference's edit_dist_trace.py, and the argument checks of
vocr_edit_stats / ops.edit_stats that need no device."""
import ctypes

import numpy as np
import pytest
import torch

from tests import score_ref as sr
from vistaocr_amd import english_alphabet
from vistaocr_amd.textutils import compute_cer_wer, edit_distance, form_tokenized_words, utf8_to_uxxxx

ALPHA = english_alphabet()


def random_pair(rng, la, lb, v):
    a = rng.integers(1, v, la).tolist()
    b = list(a[:lb]) + rng.integers(1, v, max(lb - la, 0)).tolist()
    for k in range(len(b)):
        if rng.random() < 0.3:
            b[k] = int(rng.integers(1, v))
    return a, b


@pytest.mark.parametrize("v", [3, 6, 40])
def test_plain_and_antidiagonal_forms_agree(v):
    rng = np.random.default_rng(v)
    for la, lb in [(0, 0), (0, 5), (5, 0), (1, 1), (7, 3), (3, 7), (20, 20), (33, 17), (40, 70)]:
        a, b = random_pair(rng, la, lb, v)
        D0, op0 = sr.plain_table(a, b)
        D1, op1 = sr.antidiagonal_table(a, b)
        assert np.array_equal(D0, D1) and np.array_equal(op0, op1), (la, lb)
        d, counts, steps = sr.trace(a, b)
        assert (d, counts, steps) == sr.trace(a, b, sr.antidiagonal_table)
        # the trace is complete and consistent: it consumes both sequences and its edits add up to the distance
        assert sum(1 for o, _, _ in steps if o != sr.DEL) == la and sum(1 for o, _, _ in steps if o != sr.INS) == lb
        assert sum(counts) == d


def test_distances_equal_textutils_edit_distance():
    rng = np.random.default_rng(7)
    for _ in range(60):
        la, lb = int(rng.integers(0, 30)), int(rng.integers(0, 30))
        a, b = random_pair(rng, la, lb, 30)
        stats, ops, conf = sr.pair_stats(a, b, ALPHA)
        ac, bc = [ALPHA.idx_to_char[k] for k in a], [ALPHA.idx_to_char[k] for k in b]
        assert stats[0] == edit_distance(ac, bc)
        assert stats[6] == edit_distance(form_tokenized_words(ac), form_tokenized_words(bc))
        assert stats[1] + stats[2] + stats[3] == stats[0] and stats[7] + stats[8] + stats[9] == stats[6]
        assert len(ops) == stats[0] + int((ops == sr.COPY).sum()) and conf.sum() == len(ops)
        assert conf[0, :].sum() == stats[2] and conf[:, 0].sum() == stats[3]


def _labels(text):
    return [ALPHA.char_to_idx[t] for t in utf8_to_uxxxx(text, output_array=True)]


@pytest.mark.parametrize("hyp, ref", [
    ("the quick brown fox", "the quick brown fox"), ("the quick brwn fox", "the quick brown fox"), ("", "a line, with 2 marks."),
    ("a line", ""), ("", ""), ("  lead and trail  ", "lead and trail"), ("a,b", "a, b"), ("x", "y"), ("word", "words"), ("no1se", "noise"),
])
def test_rates_equal_compute_cer_wer_bitwise(hyp, ref):
    h, r = _labels(hyp), _labels(ref)
    stats, _, _ = sr.pair_stats(h, r, ALPHA)
    want = compute_cer_wer(utf8_to_uxxxx(hyp), utf8_to_uxxxx(ref))
    assert sr.rates(stats) == want, (stats, want)                 # the very floats: exact comparison


def test_score_rates_are_the_reference_rates():
    """ErrorScorer's host arithmetic (score._rates) on the reference's integers gives compute_cer_wer's floats."""
    from vistaocr_amd.score import _rates
    rng = np.random.default_rng(3)
    rows, want = [], []
    for _ in range(20):
        a, b = random_pair(rng, int(rng.integers(0, 25)), int(rng.integers(1, 25)), len(ALPHA))
        b[0] = ALPHA.char_to_idx["u0061"]                          # at least one word in the reference
        rows.append(sr.pair_stats(a, b, ALPHA)[0])
        want.append(compute_cer_wer(" ".join(ALPHA.idx_to_char[k] for k in a), " ".join(ALPHA.idx_to_char[k] for k in b)))
    cer, wer = _rates(np.array(rows, dtype=np.int32))
    assert [(c, w) for c, w in zip(cer.tolist(), wer.tolist())] == want
    bad = np.full((1, 12), -1, dtype=np.int32)
    assert np.isnan(_rates(bad)[0]).all() and np.isnan(_rates(bad)[1]).all()


def test_known_answer_of_edit_dist_trace():
    """The pair the reference's src/edit_dist_trace.py prints, hypothesis as A: distance 13; the complete trace has 64 operations (the
    script stops at the first edge and drops the leading INS: its printed 63 are the suffix)."""
    ref = "\" McNamara's Band , \" \" Greensleeves \" and \" English Rose . \""
    hyp = " ' He Namarod's Layd , \" \" breensleeres \" and \" English hose . '"
    for table in (sr.plain_table, sr.antidiagonal_table):
        d, (sub, ins, dele), steps = sr.trace(list(hyp), list(ref), table)
        ops = [o for o, _, _ in steps]
        assert d == 13 and (ops.count(sr.COPY), sub, ins, dele, len(ops)) == (51, 10, 3, 0, 64)
        assert ops[0] == sr.INS and ops[1:4] == [sr.SUB, sr.COPY, sr.INS]           # the printed trace starts SUB, COPY, INS


def test_confusions_listing():
    from vistaocr_amd import ErrorScorer
    sc = ErrorScorer(ALPHA)
    m = np.zeros((len(ALPHA), len(ALPHA)), dtype=np.int64)
    a, b, c = ALPHA.char_to_idx["u0061"], ALPHA.char_to_idx["u0062"], ALPHA.char_to_idx["u0063"]
    m[a, a], m[a, b], m[0, c], m[b, 0], m[c, b] = 50, 3, 7, 3, 1
    assert sc.confusions(m) == [("<ins>", "u0063", 7), ("u0061", "u0062", 3), ("u0062", "<del>", 3), ("u0063", "u0062", 1)]
    assert sc.confusions(m, top=1) == [("<ins>", "u0063", 7)]


def test_shape_answers_without_a_device():
    from vistaocr_amd import _lib, build
    build.build()
    lib = _lib.load()
    ws = lib.vocr_edit_stats_workspace_bytes
    assert ws(32, 32, 32, 96, 128, 128, 3) > 0 and ws(4096, 32, 4096, 96, 300, 300, 1) > 0 and ws(1, 1, 1, 2, 0, 0, 1) > 0
    # the back pointers live per resident workgroup: the workspace stops growing with the number of pairs
    assert ws(1 << 20, 32, 1 << 20, 96, 2048, 2048, 7) == ws(1 << 12, 32, 1 << 12, 96, 2048, 2048, 7) > (1 << 20)
    assert ws(1 << 20, 32, 1 << 20, 96, 2048, 2048, 1) == ws(1, 1, 1, 96, 1, 1, 1)
    one = ctypes.c_void_p(16)

    def call(na=4, sa=8, ma=8, nb=4, sb=8, mb=8, np_=4, v=96, want=1, a=one, stats=one, conf=None, ops=None, stride=16, wsb=1 << 30):
        return lib.vocr_edit_stats(a, one, na, sa, ma, one, one, nb, sb, mb, one, np_, None, None, v, want, stats, conf, ops, stride, one,
                                   wsb, None)
    bad = [dict(v=1), dict(v=257), dict(np_=0), dict(na=0), dict(nb=0), dict(ma=2049, sa=2049), dict(mb=2049, sb=2049), dict(ma=-1),
           dict(want=0), dict(want=4), dict(want=8), dict(want=9)]
    for kw in bad:
        args = dict(na=4, nb=4, np_=4, v=96, ma=8, mb=8, want=1)
        args.update({k: v for k, v in kw.items() if k in args})
        assert ws(args["na"], args["nb"], args["np_"], args["v"], args["ma"], args["mb"], args["want"]) == 0, kw
        assert call(**kw) == -1 and b"vocr_edit_stats" in lib.vocr_last_error(), kw
    assert call(sa=7) == -1 and b"a_stride" in lib.vocr_last_error()               # a stride below the longest sequence
    assert call(a=None) == -1 and b"null pointer" in lib.vocr_last_error()
    assert call(stats=None) == -1
    assert call(want=5, ops=one, stride=15) == -1 and b"ops_stride" in lib.vocr_last_error()
    assert call(want=1, ops=one) == -1 and call(want=1, conf=one) == -1              # the trace's outputs without the trace
    assert call(want=2) == -1 and b"kinds" in lib.vocr_last_error()                 # words alone, and no kinds
    assert call(want=7, ma=2048, sa=2048, mb=2048, sb=2048, stride=4096, wsb=1 << 20) == -1 and b"workspace too small" in lib.vocr_last_error()


def test_ops_edit_stats_validates_before_it_needs_a_device():
    from vistaocr_amd import ops
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    ok = dict(a_labels=i32(4, 8), a_lens=i32(4), b_labels=i32(2, 8), b_lens=i32(2), pairs=i32(4, 2), v=96)
    cases = [(dict(a_labels=torch.zeros(4, 8, dtype=torch.int64)), "a_labels must be int32"), (dict(a_lens=i32(3)), "a_labels must be"),
             (dict(b_lens=i32(2, 1)), "b_labels must be"), (dict(pairs=i32(4, 3)), "pairs must be"), (dict(pairs=i32(0, 2)), "pairs must be"),
             (dict(want=0), "want=0"), (dict(want=4), "want=4"), (dict(want=2), "needs kinds"), (dict(ops=True), "need EDIT_TRACE"),
             (dict(confusion=i32(96, 96)), "need EDIT_TRACE")]
    for kw, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            ops.edit_stats(**dict(ok, **kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                      # valid arguments: only the device is missing
        ops.edit_stats(**ok)
