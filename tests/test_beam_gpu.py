"""GPU: vocr_ctc_beam_search (vistaocr_amd/csrc/ctc_beam.hip) through ops.ctc_beam_search / BeamDecoder, against brute force on
exact cases, the fp64 restatement (tests/beam_ref.py) on bench-shaped peaky logits, the greedy decode where both must agree, itself
(determinism), and decode_dataset's file format."""
import os

import numpy as np
import pytest
import torch

import vistaocr_amd as va
from tests import beam_data as bd
from tests import beam_ref as br
from tests.test_beam_cpu import ALPHA, ARPA
from vistaocr_amd import ops
from vistaocr_amd.decoder import greedy_label_sequences

pytestmark = pytest.mark.gpu

TAU = 2e-4          # a line is compared only where every decision of the fp64 restatement won by at least this much
T1, B1, V1 = 294, 32, 96           # configs[1]'s logits shape


def _run(x, lens, K, nbest, canon=None, lm=None, alpha=0.0, beta=0.0, prune=None):
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda() if canon is not None else None
    lab, ln, sc = ops.ctc_beam_search(xd, lens, cd, K, nbest, lm.to("cuda") if lm is not None else None, alpha, beta, prune)
    torch.cuda.synchronize()
    return lab.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()


def _hyps(lab, ln, sc, b):
    return [(list(lab[b, q, :ln[b, q]]), sc[b, q]) for q in range(lab.shape[1]) if np.isfinite(sc[b, q, 0])]


@pytest.fixture(scope="module")
def english():
    al = va.english_alphabet()
    canon = np.array(al.canonical_indices())
    return al, canon, np.nonzero(canon == np.arange(len(al)))[0][1:]


@pytest.fixture(scope="module")
def lm5(tmp_path_factory, english):
    al = english[0]
    path = str(tmp_path_factory.mktemp("lm") / "char5.arpa")
    bd.write_char_arpa(path, [al.idx_to_char[c] for c in range(1, 40)], order=5, seed=3)
    return va.CharNgramLM.from_arpa(path, al)


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("T,ncls,K", [(5, 2, 64), (4, 3, 128)])
def test_exact_against_brute_force(tmp_path, with_lm, T, ncls, K):
    """No pruning and K >= the number of prefixes (63 / 121): nothing is ever pruned, so every listed hypothesis is the brute-force one,
    in the brute-force order, with the brute-force CTC log-probability."""
    lm = None
    if with_lm:
        (tmp_path / "lm3.arpa").write_text(ARPA[3])
        lm = va.CharNgramLM.from_arpa(str(tmp_path / "lm3.arpa"), ALPHA)
    alpha, beta = (0.7, 0.3) if with_lm else (0.0, 0.2)
    rng = np.random.default_rng(T * 10 + ncls)
    V = len(ALPHA)
    logits = rng.normal(0, 1.5, size=(T, V))
    logits[:, ncls + 1:] = -np.inf
    brute = br.brute_force(logits, list(range(1, ncls + 1)), lm=lm, alpha=alpha, beta=beta)
    totals = np.array([h[1] for h in brute])
    assert len(brute) > 20 and np.min(totals[:-1] - totals[1:]) > 1e-4       # the fixed seed has no near ties: the order is testable
    nbest = min(len(brute), K)
    lab, ln, sc = _run(logits[:, None, :], [T], K, nbest, lm=lm, alpha=alpha, beta=beta)
    got = _hyps(lab, ln, sc, 0)
    assert len(got) == len(brute)
    for (glab, gsc), (blab, btot, bac, blm) in zip(got, brute):
        assert glab == blab
        assert abs(gsc[1] - bac) <= 1e-5 * abs(bac) + 1e-6, (blab, gsc, bac)
        assert abs(gsc[0] - btot) <= 1e-5 * abs(btot) + 1e-5 and abs(gsc[2] - blm) <= 1e-5 * abs(blm) + 1e-5


def _compare_to_restatement(x, lens, K, nbest, canon, lm, alpha, beta, prune=None, min_lines=None):
    lab, ln, sc = _run(x, lens, K, nbest, canon=canon, lm=lm, alpha=alpha, beta=beta, prune=prune)
    used = 0
    for b in range(x.shape[1]):
        ref, gap = br.beam_search(x[:, b], lens[b], K, nbest=nbest, canon=canon, lm=lm, alpha=alpha, beta=beta, prune=prune)
        if gap < TAU:
            continue
        used += 1
        got = _hyps(lab, ln, sc, b)
        assert [g[0] for g in got] == [r[0] for r in ref], (b, K)
        for g, r in zip(got, ref):
            assert np.allclose(g[1], r[1:], atol=1e-3, rtol=0), (b, K, g[1], r[1:])
    if min_lines is not None:
        assert used >= min_lines, "only %d of %d lines are decided by more than %g" % (used, x.shape[1], TAU)
    return used


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("K", [1, 8, 16, 64])
def test_bench_shape_against_restatement(english, lm5, K, with_lm):
    al, canon, cls = english
    x = bd.peaky_logits(np.random.default_rng(7), T1, B1, V1, classes=cls)
    lm = lm5 if with_lm else None
    _compare_to_restatement(x, [T1] * B1, K, min(K, 4), canon, lm, 0.8 if with_lm else 0.0, 1.0 if with_lm else 0.0, min_lines=24)


def test_ragged_lengths_and_odd_batch(english, lm5):
    al, canon, cls = english
    B = 7
    x = bd.peaky_logits(np.random.default_rng(11), 60, B, V1, classes=cls)
    lens = [0, 1, 60, 17, 2, 59, 33]
    used = _compare_to_restatement(x, lens, 16, 3, canon, lm5, 0.5, 0.5)
    assert used >= 5
    lab, ln, sc = _run(x, lens, 16, 3, canon=canon, lm=lm5, alpha=0.5, beta=0.5)
    assert ln[0, 0] == 0 and np.isfinite(sc[0, 0, 0]) and sc[0, 0, 1] == 0.0          # no frames: the empty labelling, P = 1
    assert abs(sc[0, 0, 2] - lm5.eos[lm5.start]) < 1e-5
    assert not np.isfinite(sc[0, 1, 0]) and ln[0, 1] == 0                              # and nothing else
    assert ln[1, 0] <= 1


def test_arabic_alphabet():
    al = va.arabic_alphabet()
    V = len(al)
    assert V == 166
    canon = np.array(al.canonical_indices())
    cls = np.nonzero(canon == np.arange(V))[0][1:]
    x = bd.peaky_logits(np.random.default_rng(5), 120, 9, V, classes=cls)
    assert _compare_to_restatement(x, [120] * 9, 16, 2, canon, None, 0.0, 0.0) >= 7


def test_duplicate_english_classes_merge(english):
    """'u002d' sits at 73 and 91: their probabilities add, and the emitted label is the canonical 73."""
    al, canon, cls = english
    assert al.idx_to_char[73] == al.idx_to_char[91] and canon[91] == 73
    x = np.full((3, 1, V1), -np.inf, dtype=np.float32)
    x[:, 0, 0] = 0.0
    x[1, 0, 73] = np.log(0.3)
    x[1, 0, 91] = np.log(0.3)
    x[1, 0, 5] = np.log(0.4)                    # each half of the hyphen alone loses to class 5; together they win
    x[1, 0, 0] = -np.inf
    x[[0, 2], 0, 0] = 0.0
    lab, ln, sc = _run(x, [3], 4, 2, canon=canon)
    assert list(lab[0, 0, :ln[0, 0]]) == [73] and list(lab[0, 1, :ln[0, 1]]) == [5]
    assert abs(sc[0, 0, 1] - np.log(0.6)) < 1e-5
    lab, ln, sc = _run(x, [3], 4, 2, canon=None)                   # without classes the columns compete
    assert list(lab[0, 0, :ln[0, 0]]) == [5]


def test_pruning_against_restatement(english, lm5):
    al, canon, cls = english
    x = bd.peaky_logits(np.random.default_rng(9), T1, 8, V1, classes=cls)
    for prune in (-10.0, -25.0):
        assert _compare_to_restatement(x, [T1] * 8, 16, 2, canon, lm5, 0.8, 1.0, prune=prune) >= 6


def test_agrees_with_greedy_on_confident_logits(english):
    """Frame maxima above 0.99 probability and raw maxima above 3/V: the best path is the best labelling, so K = 1 and K = 16 give
    the greedy decode (labels compared through the classes: greedy emits the argmax column, the search the canonical one)."""
    al, canon, cls = english
    rng = np.random.default_rng(3)
    B, T = 12, 150
    x = rng.normal(0, 1, size=(T, B, V1)).astype(np.float32)
    dom = np.where(rng.random((T, B)) < 0.4, rng.choice(np.arange(1, V1), size=(T, B)), 0)
    np.put_along_axis(x, dom[:, :, None], 14.0 + rng.random((T, B, 1)).astype(np.float32), axis=2)
    p = np.exp(br.log_softmax(x))
    assert p.max(axis=2).min() > 0.99 and x.max(axis=2).min() > 3.0 / V1
    xd = torch.from_numpy(x).cuda()
    lens = torch.tensor([T - 7 * b for b in range(B)])
    greedy = greedy_label_sequences(xd, lens, al)[1]             # CnnOcrModel.decode_labels
    strings = va.ArgmaxDecoder(al).decode(xd, lens)
    for K in (1, 16):
        dec = va.BeamDecoder(al, beam=K, nbest=1)
        got = dec.decode_nbest(xd, lens)
        assert [h[0][0] for h in got] == [[int(canon[k]) for k in g] for g in greedy]
        assert dec.decode(xd, lens) == strings
        assert dec.decode(xd, lens, uxxxx=True) == va.ArgmaxDecoder(al).decode(xd, lens, uxxxx=True)


def test_bit_identical_runs(english, lm5):
    al, canon, cls = english
    x = bd.peaky_logits(np.random.default_rng(13), T1, B1, V1, classes=cls)
    x[np.isinf(x)] = -30.0                      # dense candidates: many near ties, the total order must still decide them alike
    x += np.random.default_rng(14).normal(0, 0.5, size=x.shape).astype(np.float32)
    a = _run(x, [T1] * B1, 64, 8, canon=canon, lm=lm5, alpha=0.8, beta=1.0)
    b = _run(x, [T1] * B1, 64, 8, canon=canon, lm=lm5, alpha=0.8, beta=1.0)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


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


def test_decode_dataset_with_beam_decoder(tmp_path, lm5):
    from vistaocr_amd.loop import SortByWidthCollater, decode_dataset
    from vistaocr_amd.textutils import uxxxx_to_utf8
    al = va.english_alphabet()
    model = _tiny_model(al)
    r = np.random.RandomState(0)
    items = [(torch.from_numpy(r.uniform(0, 1, size=(1, 30, w)).astype(np.float32)), [1], {"width": w, "utt-id": "doc7_line_%d" % i})
             for i, w in enumerate([140, 96, 201, 64])]
    loader = [SortByWidthCollater(items[:2]), SortByWidthCollater(items[2:])]

    def files(d):
        return [open(os.path.join(d, f), "rb").read() for f in ("hyp-chars.txt", "hyp-chars.txt.utf8")]

    assert decode_dataset(model, loader, str(tmp_path / "default")) == 4
    assert decode_dataset(model, loader, str(tmp_path / "argmax"), decoder=va.ArgmaxDecoder(al)) == 4
    assert files(tmp_path / "default") == files(tmp_path / "argmax")            # the default call is the greedy decode, byte for byte
    dec = va.BeamDecoder(al, beam=16, lm=lm5, lm_weight=0.5, insertion_bonus=0.5)
    assert decode_dataset(model, loader, str(tmp_path / "beam"), decoder=dec) == 4
    a, b = [f.decode().splitlines() for f in files(tmp_path / "beam")]
    assert len(a) == len(b) == 4
    for la, lb in zip(a, b):
        ux, uid = la.rsplit(" (", 1)
        u8, uid8 = lb.rsplit(" (", 1)
        assert uid.rstrip(")").startswith("doc7_line_") and uid8.rstrip(")") == "doc7_line"
        assert uxxxx_to_utf8(ux) == u8
        assert all(tok.startswith("u") and len(tok) == 5 for tok in ux.split()) or ux == ""
