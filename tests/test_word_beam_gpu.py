"""GPU: vocr_ctc_word_beam_search (vistaocr_amd/csrc/ctc_word_beam.hip) through ops.ctc_word_beam_search / WordBeamDecoder, against
brute force on exact cases, the fp64 restatement (tests/word_beam_ref.py) on bench-shaped sentence logits, the lexicon and score
identities of its n-best, the character search without an LM (bit for bit where both rank alike), itself (determinism), edge shapes,
the greedy decode's WER and decode_dataset's file format."""
import os

import numpy as np
import pytest
import torch

import vistaocr_amd as va
from tests import beam_data as bd
from tests import word_beam_data as wd
from tests import word_beam_ref as wr
from tests.test_beam_gpu import _tiny_model
from tests.test_word_beam_cpu import ALPHA, ARPA3, CASES
from vistaocr_amd import ops
from vistaocr_amd.lm import _parse_arpa
from vistaocr_amd.textutils import _DIGITS, _PUNCT, compute_cer_wer, form_tokenized_words

pytestmark = pytest.mark.gpu

TAU = 2e-4          # a line is compared only where every decision of the fp64 restatement won by at least this much
T1, B1, V1 = 294, 32, 96           # configs[1]'s logits shape


def _run(x, lens, K, nbest, lm, canon=None, alpha=0.8, beta=0.0, oov=None):
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda() if canon is not None else None
    lab, ln, sc = ops.ctc_word_beam_search(xd, lens, cd, lm.to("cuda"), K, nbest, alpha, beta, oov)
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
def corpus(tmp_path_factory, english):
    """A 400-word Zipf lexicon, a word 3-gram estimated from 1500 sentences, 32 held-out sentences and their logits."""
    al = english[0]
    rng = np.random.default_rng(1)
    words, wts = wd.make_lexicon(rng, 400)
    sents = wd.make_sentences(rng, words, wts, 1532, max_words=6)
    path = str(tmp_path_factory.mktemp("wlm") / "word3.arpa")
    wd.write_word_arpa(path, words, wts, sents[:1500], seed=2)
    lm = va.WordNgramLM.from_arpa(path, al)
    x, lens = wd.sentence_logits(np.random.default_rng(3), sents[1500:], al, T1)
    return lm, _parse_arpa(path), sents[1500:], x, lens


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tiny") / "w3.arpa")
    open(path, "w").write(ARPA3)
    return va.WordNgramLM.from_arpa(path, ALPHA), _parse_arpa(path)


@pytest.mark.parametrize("oov", [None, -2.5])
@pytest.mark.parametrize("T,cls", CASES)
def test_exact_against_brute_force(tiny, T, cls, oov):
    """K = 128 holds every prefix: every listed hypothesis is the brute-force one, in the brute-force order, with its scores."""
    lm, grams = tiny
    rng = np.random.default_rng(T * 100 + sum(cls) + 7)
    V = len(ALPHA)
    logits = rng.normal(0, 1.5, size=(T, V))
    mask = np.ones(V, dtype=bool)
    mask[[0] + cls] = False
    logits[:, mask] = -np.inf
    brute = wr.brute_force(logits, cls, ALPHA, grams, alpha=0.9, beta=0.4, oov=oov)
    totals = np.array([h[1] for h in brute])
    assert len(brute) >= 5 and np.min(totals[:-1] - totals[1:]) > 1e-3          # no near ties: the order is testable
    nbest = min(len(brute), 128)
    lab, ln, sc = _run(logits[:, None, :], [T], 128, nbest, lm, alpha=0.9, beta=0.4, oov=oov)
    got = _hyps(lab, ln, sc, 0)
    assert len(got) == len(brute)
    for (glab, gsc), (blab, btot, bac, blm) in zip(got, brute):
        assert glab == blab
        assert abs(gsc[1] - bac) <= 1e-5 * abs(bac) + 1e-5, (blab, gsc, bac)
        assert abs(gsc[0] - btot) <= 1e-5 * abs(btot) + 1e-5 and abs(gsc[2] - blm) <= 1e-5 * abs(blm) + 1e-5


def _compare_to_restatement(x, lens, K, nbest, canon, lm, alpha, beta, oov=None, min_lines=None):
    lab, ln, sc = _run(x, lens, K, nbest, lm, canon=canon, alpha=alpha, beta=beta, oov=oov)
    used = 0
    for b in range(x.shape[1]):
        ref, gap = wr.beam_search(x[:, b], lens[b], K, lm, nbest=nbest, canon=canon, alpha=alpha, beta=beta, oov=oov)
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


@pytest.mark.parametrize("oov", [None, -3.0])
@pytest.mark.parametrize("K", [1, 8, 16, 64])
def test_bench_shape_against_restatement(english, corpus, K, oov):
    al, canon, _ = english
    lm, _, _, x, lens = corpus
    _compare_to_restatement(x, lens, K, min(K, 4), canon, lm, 0.8, 1.0, oov=oov, min_lines=24)


def test_closed_vocabulary_nbest_identities(english, corpus):
    """Closed mode: every letter-word of every n-best hypothesis is a lexicon word; totals do not increase down the list; and
    total = acoustic + alpha * lm + word_bonus * n_tokens."""
    al, canon, _ = english
    lm, _, _, x, lens = corpus
    alpha, wb = 0.8, 0.5
    lab, ln, sc = _run(x, lens, 16, 8, lm, canon=canon, alpha=alpha, beta=wb)
    checked = 0
    for b in range(x.shape[1]):
        hyps = _hyps(lab, ln, sc, b)
        assert hyps
        tot = [h[1][0] for h in hyps]
        assert all(a >= c for a, c in zip(tot[:-1], tot[1:]))
        for labels, s in hyps:
            toks = form_tokenized_words([al.idx_to_char[int(c)] for c in labels])
            for w in toks:
                assert w in _PUNCT or w in _DIGITS or w in lm.lexicon, w
            assert abs(s[0] - (s[1] + alpha * s[2] + wb * len(toks))) <= 1e-5 * abs(s[0]) + 1e-3
            checked += 1
    assert checked > 32


def test_equivalence_with_character_search(tmp_path, english):
    """lm_weight = word_bonus = 0 and oov_penalty = 0: every candidate the character search has exists with the same score, so
    labels, lengths and acoustic scores equal BeamDecoder(lm=None)'s bit for bit."""
    al, canon, cls = english
    rng = np.random.default_rng(21)
    words, wts = wd.make_lexicon(rng, 300)
    sents = wd.make_sentences(rng, words, wts, 600)
    tmp = str(tmp_path / "eq.arpa")
    wd.write_word_arpa(tmp, words, wts, sents, seed=4)
    lm = va.WordNgramLM.from_arpa(tmp, al)
    x = bd.peaky_logits(np.random.default_rng(7), T1, B1, V1, classes=cls)
    xd = torch.from_numpy(x).cuda()
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda()
    for K, nbest in ((1, 1), (16, 4), (64, 8)):
        a = [t.cpu().numpy() for t in ops.ctc_beam_search(xd, [T1] * B1, cd, K, nbest)]
        w = [t.cpu().numpy() for t in ops.ctc_word_beam_search(xd, [T1] * B1, cd, lm.to("cuda"), K, nbest, 0.0, 0.0, 0.0)]
        assert a[0].tobytes() == w[0].tobytes() and a[1].tobytes() == w[1].tobytes(), K
        assert a[2][..., 1].tobytes() == w[2][..., 1].tobytes(), K


def test_bit_identical_runs(english, corpus):
    al, canon, _ = english
    lm = corpus[0]
    x = bd.peaky_logits(np.random.default_rng(13), T1, B1, V1, classes=english[2])
    x[np.isinf(x)] = -30.0                      # dense candidates: many near ties, the total order must still decide them alike
    x += np.random.default_rng(14).normal(0, 0.5, size=x.shape).astype(np.float32)
    a = _run(x, [T1] * B1, 64, 8, lm, canon=canon, alpha=0.8, beta=0.5, oov=-4.0)
    b = _run(x, [T1] * B1, 64, 8, lm, canon=canon, alpha=0.8, beta=0.5, oov=-4.0)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_edge_shapes(english, corpus, tiny):
    al, canon, _ = english
    lm, _, _, x, lens = corpus
    # T = 1, B = 1, K = 1
    lab, ln, sc = _run(x[:1, :1], [1], 1, 1, lm, canon=canon, oov=-2.0)
    ref, _ = wr.beam_search(x[:1, 0], 1, 1, lm, nbest=1, canon=canon, alpha=0.8, oov=-2.0)
    assert _hyps(lab, ln, sc, 0)[0][0] == ref[0][0]
    # a line of length 0: the empty labelling with ln P(</s> | <s>); nbest = K
    lab, ln, sc = _run(x[:, :3], [0, T1, 5], 4, 4, lm, canon=canon)
    assert ln[0, 0] == 0 and sc[0, 0, 1] == 0.0 and abs(sc[0, 0, 2] - lm.lookup(lm.start, lm.eos)[0]) < 1e-5
    assert not np.isfinite(sc[0, 1, 0]) and ln[0, 1] == 0
    for b, L in ((1, T1), (2, 5)):
        ref, gap = wr.beam_search(x[:, b], L, 4, lm, nbest=4, canon=canon, alpha=0.8)
        assert gap < TAU or [h[0] for h in _hyps(lab, ln, sc, b)] == [r[0] for r in ref]
    # every beam ends inside a word that cannot close ('c a' is only a prefix of 'cab'): no output, total -inf
    tlm, _ = tiny
    lg = np.full((2, 2, len(ALPHA)), -np.inf, dtype=np.float32)
    lg[0, :, 3] = 0.0
    lg[1, :, 1] = 0.0
    lab, ln, sc = _run(lg, [2, 2], 8, 2, tlm, oov=None)
    assert (ln == 0).all() and not np.isfinite(sc[:, :, 0]).any() and (lab == 0).all()
    lab, ln, sc = _run(lg, [2, 2], 8, 2, tlm, oov=-1.0)
    assert list(lab[0, 0, :ln[0, 0]]) == [3, 1] and np.isfinite(sc[0, 0, 0])


def test_wer_against_greedy_and_character_search(english, corpus):
    """The synthetic sentences (fixed seed): the word decode at least halves the greedy decode's WER and is no worse than the
    character search without an LM."""
    al, canon, _ = english
    lm, _, sents, x, lens = corpus
    xd = torch.from_numpy(x).cuda()
    refs = [" ".join(s) for s in sents]

    def wer(hyps):
        return float(np.mean([compute_cer_wer(h, r)[1] for h, r in zip(hyps, refs)]))

    greedy = wer(va.ArgmaxDecoder(al).decode(xd, lens, uxxxx=True))
    beam = wer(va.BeamDecoder(al, beam=16).decode(xd, lens, uxxxx=True))
    word = wer(va.WordBeamDecoder(al, lm, beam=16, lm_weight=0.8).decode(xd, lens, uxxxx=True))
    assert greedy > 0.05, greedy
    assert word <= 0.5 * greedy and word <= beam, (word, greedy, beam)


def test_decode_dataset_with_word_beam_decoder(tmp_path, corpus):
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

    assert decode_dataset(model, loader, str(tmp_path / "greedy")) == 4
    dec = va.WordBeamDecoder(al, corpus[0], beam=16, lm_weight=0.5, word_bonus=0.5, oov_penalty=-5.0)
    assert decode_dataset(model, loader, str(tmp_path / "word"), decoder=dec) == 4
    g = [f.decode().splitlines() for f in files(tmp_path / "greedy")]
    a, b = [f.decode().splitlines() for f in files(tmp_path / "word")]
    assert len(a) == len(b) == 4
    for la, lb, ga, gb in zip(a, b, *g):
        ux, uid = la.rsplit(" (", 1)
        u8, uid8 = lb.rsplit(" (", 1)
        assert uid == ga.rsplit(" (", 1)[1] and uid8 == gb.rsplit(" (", 1)[1]
        assert uid.rstrip(")").startswith("doc7_line_") and uid8.rstrip(")") == "doc7_line"
        assert uxxxx_to_utf8(ux) == u8
        assert all(tok.startswith("u") and len(tok) == 5 for tok in ux.split()) or ux == ""
