"""GPU: MinErrorRateLoss (vistaocr_amd/risk.py), the expected number of edit errors over a beam search's n-best list.  The list and the
error counts are taken from the device as the criterion sees them; the risk and its gradient with respect to the logits are then
computed in fp64 by tests/nbest_ref.py (risk_reference) and compared under the bars derived at its head."""
import numpy as np
import pytest
import torch

import vistaocr_amd as va
from tests import align_ref as ar
from tests import beam_data as bd
from tests import ctc_ref as cr
from tests import nbest_ref as nr
from vistaocr_amd import ops
from vistaocr_amd import risk as rk

pytestmark = pytest.mark.gpu

T, B, V = 48, 6, 96
AL = va.english_alphabet()                                    # 96 columns, u002d twice: a class of two members
CANON = np.array(AL.canonical_indices())
CLS = np.nonzero(CANON == np.arange(V))[0][1:]
LENS = [48, 45, 40, 33, 17, 9]


def _data(seed=3):
    """peaky logits with a competitor on half of the frames and a blank that is always possible; the references are the greedy
    labellings with one label replaced (line 3: as it is, so its reference is a likely labelling), so the hypotheses of a list differ in
    their error counts"""
    rng = np.random.default_rng(seed)
    x = bd.peaky_logits(rng, T, B, V, classes=CLS, p_char=0.3)
    x[:, :, 0] = np.where(np.isinf(x[:, :, 0]), x.max(axis=2) - 12.0, x[:, :, 0])
    x = np.where(np.isinf(x), x.max(axis=2, keepdims=True) - 25.0, x).astype(np.float32)     # a finite CTC loss for any reference
    refs = []
    for b in range(B):
        lab = ar.greedy_labels(x[:, b], LENS[b]) or [int(CLS[3])]
        if b != 3:                                                                           # line 3: the greedy labelling itself
            lab[int(rng.integers(len(lab)))] = int(CLS[int(rng.integers(len(CLS)))])
        if b == 1:
            lab = lab + [int(AL.char_to_idx["u0020"]), int(CLS[5])]                          # another word at the end
        refs.append(lab)
    targets = torch.tensor([v for l in refs for v in l], dtype=torch.int32)
    return torch.from_numpy(x), targets, torch.tensor(LENS, dtype=torch.int32), torch.tensor([len(l) for l in refs], dtype=torch.int32), refs


class _Blanked:
    """a decoder whose search found nothing for some lines (total -inf on every rank), whatever the logits: a test double"""

    def __init__(self, dec, lines):
        self.dec, self.lines, self.beam = dec, list(lines), dec.beam

    def _search_device(self, x, lens, nbest):
        labels, lengths, scores = self.dec._search_device(x, lens, nbest)
        scores = scores.clone()
        scores[self.lines] = float("-inf")
        return labels, lengths, scores


def _host_list(crit, xd, targets, act, tl):
    """the list as the criterion sees it, on the host: hyps[b][q], errors, filled, member"""
    labels, lengths, errors, ctc, member, canon = rk.nbest_list(xd, targets, act, tl, crit.decoder, crit.scorer, crit.nbest, crit.unit,
                                                                crit.add_reference)
    _, _, sc = crit.decoder._search_device(xd, act, crit.nbest)
    filled = (sc[:, :, 0] > float("-inf")).cpu().numpy()
    if crit.add_reference:
        filled = np.concatenate([filled, np.ones((filled.shape[0], 1), dtype=bool)], axis=1)
    lab, ln = labels.cpu().numpy(), lengths.cpu().numpy()
    hyps = [[[int(v) for v in lab[b, q, :ln[b, q]]] if ln[b, q] >= 0 else None for q in range(lab.shape[1])] for b in range(lab.shape[0])]
    return hyps, errors.cpu().numpy().astype(np.float64), filled, member.cpu().numpy(), ctc.cpu().numpy()


def _against_restatement(crit, x, targets, act, tl, what):
    xd = x.cuda().requires_grad_(True)
    loss = crit(xd, targets, act, tl)
    assert tuple(loss.shape) == (1,) and loss.is_cuda
    loss.backward()
    hyps, errors, filled, member, ctc = _host_list(crit, xd.detach(), targets, act, tl)
    risk, rbar, c, g, gbar, scores, mem = nr.risk_reference(x, [int(v) for v in act], hyps, CANON, errors, filled, max_label_len=x.shape[0])
    assert (mem == member).all(), what
    got = float(loss.detach().cpu())
    tol = rbar.sum() + (len(risk) + 2) * nr.U * risk.sum() + 2.0 ** -126                  # the fp32 batch sum on top of the per-line bars
    gfrac = float(cr.ratio(xd.grad.cpu(), g, gbar))
    print("risk-errors %-22s lists %s  risk %.6f fp64 %.6f  |diff| / bar %.3f  grad diff / bar %.3f  max |grad| %.3g"
          % (what, member.sum(1).tolist(), got, risk.sum(), abs(got - risk.sum()) / tol, gfrac, float(g.abs().max())))
    if not gfrac <= 1.0:                                                                  # say where
        gg = xd.grad.cpu().double()
        r = torch.where(gg == g, torch.zeros_like(g), (gg - g).abs() / gbar)
        r = torch.nan_to_num(r, nan=float("inf"))
        i = tuple(int(v) for v in np.unravel_index(int(torch.argmax(r)), r.shape))
        print("risk-errors %s: worst element [t, b, v] = %s got %.9g fp64 %.9g bar %.3g; NaN in the gradient: %d; errors of that line %s, c %s"
              % (what, i, float(gg[i]), float(g[i]), float(gbar[i]), int(torch.isnan(gg).sum()), errors[i[1]].tolist(), c[i[1]].tolist()))
    assert abs(got - risk.sum()) <= tol and gfrac <= 1.0, what
    assert member.sum() >= len(risk) and float(g.abs().max()) > 1e-4, what         # lists worth the name, a gradient worth comparing
    return risk, c, g, gbar, hyps, errors, filled, xd.grad.detach().cpu()


def test_loss_and_gradient_against_restatement():
    x, targets, act, tl, _ = _data()
    for unit in ("char", "word"):
        crit = va.MinErrorRateLoss(AL, decoder=va.BeamDecoder(AL, beam=16), nbest=4, unit=unit, ctc_weight=0.0)
        _against_restatement(crit, x, targets, act, tl, "beam16 n4 " + unit)
    _against_restatement(va.MinErrorRateLoss(AL, nbest=8, ctc_weight=0.0), x, targets, act, tl, "default decoder n8")


def test_directional_derivative_of_the_fixed_list():
    """needs no restatement of the gradient: with the list held fixed, f(x) = sum_b risk_b evaluated in fp64 on the host satisfies
    (f(x - eps g) - f(x)) / eps = -|g|^2 - <grad f - g, g> + eps / 2 g'Hg + O(eps^2) for the device's gradient g.  eps moves no logit by
    more than 1e-3; the second-order term is MEASURED in fp64 by the second difference k = (f(x - 2 eps g) - 2 f(x - eps g) + f(x)) /
    eps^2 ~ g'Hg, and the tolerance is eps |k| (twice that term) + sum |g| gbar (the gradient's own bars) + the fp64 rounding of the
    difference quotient; it must come out below 5% of |g|^2 for the check to mean anything."""
    x, targets, act, tl, _ = _data()
    crit = va.MinErrorRateLoss(AL, decoder=va.BeamDecoder(AL, beam=16), nbest=4, ctc_weight=0.0)
    risk, c, g64, gbar, hyps, errors, filled, g = _against_restatement(crit, x, targets, act, tl, "directional")
    g = g.double()
    lens = [int(v) for v in act]

    def f(xx):
        sc, _ = nr.nbest(xx, lens, hyps, CANON, None, x.shape[0])
        s = sc.numpy()
        return nr.risk_terms(s, errors, filled & np.isfinite(s))[0].sum()
    eps = 1e-3 / float(g.abs().max())
    x64 = x.double()
    f0, f1, f2 = f(x64), f(x64 - eps * g), f(x64 - 2 * eps * g)
    k = (f2 - 2 * f1 + f0) / eps ** 2
    gg = float((g * g).sum())
    tol = eps * abs(k) + float((g.abs() * gbar).sum()) + 64 * 2.0 ** -52 * max(abs(f0), 1.0) / eps
    d = (f1 - f0) / eps
    print("risk-errors directional: eps %.3g  quotient %.9g  -|g|^2 %.9g  second-order eps k / 2 %.3g  tolerance %.3g (%.2f%% of |g|^2)"
          % (eps, d, -gg, eps * k / 2, tol, 100 * tol / gg))
    assert tol <= 0.05 * gg and abs(d + gg) <= tol


def test_error_counts_are_the_scorers():
    x, targets, act, tl, _ = _data()
    xd = x.cuda()
    dec = va.BeamDecoder(AL, beam=16)
    scorer = va.ErrorScorer(AL)
    labels, lengths, _ = dec._search_device(xd, act, 4)
    want = scorer.score(labels, lengths, targets, tl)
    for unit, w in (("char", want.char_dist), ("word", want.word_dist)):
        _, _, errors, _, member, _ = rk.nbest_list(xd, targets, act, tl, dec, scorer, 4, unit)
        assert member.all() and np.array_equal(errors.cpu().numpy(), w.astype(np.float32)), unit
    assert (want.char_dist != want.word_dist).any() and want.char_dist.max() >= 2 and (want.char_dist.min(1) < want.char_dist.max(1)).any()
    r, top = rk.expected_errors(xd, targets, act, tl, AL, decoder=dec, nbest=4)
    assert tuple(r.shape) == (B,) and r.is_cuda and np.array_equal(top.cpu().numpy(), want.char_dist[:, 0].astype(np.float32))
    assert (r.cpu().numpy() <= want.char_dist.max(1) + 1e-4).all() and (r.cpu().numpy() >= want.char_dist.min(1) - 1e-4).all()


def test_empty_lists_contribute_nothing():
    x, targets, act, tl, _ = _data()
    dec = va.BeamDecoder(AL, beam=16)
    full = va.MinErrorRateLoss(AL, decoder=dec, nbest=4, ctc_weight=0.0)
    some = va.MinErrorRateLoss(AL, decoder=_Blanked(dec, [1, 4]), nbest=4, ctc_weight=0.0)
    xa, xb = x.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    full(xa, targets, act, tl).backward()
    lb = some(xb, targets, act, tl)
    lb.backward()
    keep = [0, 2, 3, 5]
    assert torch.equal(xb.grad[:, keep], xa.grad[:, keep]) and float(xb.grad[:, [1, 4]].abs().max()) == 0.0
    per_line, _ = rk.expected_errors(x.cuda(), targets, act, tl, AL, decoder=dec, nbest=4)
    assert abs(float(lb.detach()) - float(per_line[keep].sum())) <= 1e-5 * max(float(lb.detach()), 1.0)
    r, top = rk.expected_errors(x.cuda(), targets, act, tl, AL, decoder=_Blanked(dec, [1, 4]), nbest=4)
    assert r[[1, 4]].tolist() == [0.0, 0.0] and bool(torch.isnan(top[[1, 4]]).all()) and not bool(torch.isnan(top[keep]).any())
    # only such lines: what is left is ctc_weight * CTC, in value and in gradient
    none = va.MinErrorRateLoss(AL, decoder=_Blanked(dec, range(B)), nbest=4, ctc_weight=0.25)
    xc, xe = x.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    ln = none(xc, targets, act, tl)
    ln.backward()
    lc = va.CTCLoss()(xe, targets, act, tl)
    lc.backward()
    assert np.isfinite(float(lc.detach())) and float(ln.detach()) == np.float32(0.25) * np.float32(float(lc.detach()))
    assert torch.equal(xc.grad, 0.25 * xe.grad)


def test_add_reference():
    x, targets, act, tl, refs = _data()
    xd = x.cuda()
    dec, scorer = va.BeamDecoder(AL, beam=16), va.ErrorScorer(AL)
    labels, lengths, errors, ctc, member, _ = rk.nbest_list(xd, targets, act, tl, dec, scorer, 4, "char", add_reference=True)
    assert tuple(labels.shape) == (B, 5, T) and errors[:, 4].tolist() == [0.0] * B and bool(member[:, 4].all())
    assert [labels[b, 4, :len(refs[b])].tolist() for b in range(B)] == refs and lengths[:, 4].tolist() == [len(r) for r in refs]
    without, _ = rk.expected_errors(xd, targets, act, tl, AL, decoder=dec, nbest=4)
    with_ref, _ = rk.expected_errors(xd, targets, act, tl, AL, decoder=dec, nbest=4, add_reference=True)
    # a zero-error member takes probability from the others: risk' = risk Z / (Z + P_ref) <= risk; both are fp32 softmaxes of <= 5 terms
    assert bool((with_ref <= without * (1 + 16 * nr.U)).all()) and bool((with_ref < without).any())
    crit = va.MinErrorRateLoss(AL, decoder=dec, nbest=4, ctc_weight=0.0, add_reference=True)
    _against_restatement(crit, x, targets, act, tl, "add_reference")
    with pytest.raises(ValueError, match="nbest"):
        va.MinErrorRateLoss(AL, decoder=va.BeamDecoder(AL, beam=128), nbest=128, add_reference=True)


def test_both_decoders_with_language_models(tmp_path):
    from tests import word_beam_data as wd
    x, targets, act, tl, _ = _data()
    path = bd.write_char_arpa(str(tmp_path / "char5.arpa"), [AL.idx_to_char[c] for c in range(1, 40)], order=5, seed=3)
    lm = va.CharNgramLM.from_arpa(path, AL)
    crit = va.MinErrorRateLoss(AL, decoder=va.BeamDecoder(AL, beam=16, lm=lm, lm_weight=0.5), nbest=4, ctc_weight=0.0)
    _against_restatement(crit, x, targets, act, tl, "beam + char LM")
    rng = np.random.default_rng(1)
    words, wts = wd.make_lexicon(rng, 200)
    sents = wd.make_sentences(rng, words, wts, 806, max_words=4)
    wpath = str(tmp_path / "word3.arpa")
    wd.write_word_arpa(wpath, words, wts, sents[:800], seed=2)
    wlm = va.WordNgramLM.from_arpa(wpath, AL)
    xs, slens = wd.sentence_logits(np.random.default_rng(3), sents[800:], AL, 160)
    wt = [[AL.char_to_idx[u] for u in s] for s in sents[800:]]
    wtargets = torch.tensor([v for l in wt for v in l], dtype=torch.int32)
    crit = va.MinErrorRateLoss(AL, decoder=va.WordBeamDecoder(AL, wlm, beam=16, lm_weight=0.8), nbest=4, unit="word", ctc_weight=0.0)
    _against_restatement(crit, torch.from_numpy(xs), wtargets, torch.tensor(slens, dtype=torch.int32),
                         torch.tensor([len(l) for l in wt], dtype=torch.int32), "word beam + word LM")


def test_ctc_weight_adds_the_two_gradients():
    x, targets, act, tl, _ = _data()
    dec = va.BeamDecoder(AL, beam=16)
    grads, losses = [], []
    for crit in (va.MinErrorRateLoss(AL, decoder=dec, nbest=4, ctc_weight=0.0), va.CTCLoss(),
                 va.MinErrorRateLoss(AL, decoder=dec, nbest=4, ctc_weight=0.3)):
        xd = x.cuda().requires_grad_(True)
        loss = crit(xd, targets, act, tl)
        loss.backward()
        grads.append(xd.grad.double().cpu())
        losses.append(float(loss.detach()))
    w = float(np.float32(0.3))
    # the same kernels computed both parts: what differs is the fp32 scaling by 0.3 and the fp32 sum of the two tensors
    bound = 4 * nr.U * (grads[0].abs() + w * grads[1].abs()) + 2.0 ** -126
    assert bool(((grads[2] - (grads[0] + w * grads[1])).abs() <= bound).all())
    assert abs(losses[2] - (losses[0] + w * losses[1])) <= 4 * nr.U * (abs(losses[0]) + w * abs(losses[1]))
    assert float(grads[0].abs().max()) > 1e-4 and float(grads[1].abs().max()) > 1e-2


def _tiny_model():
    torch.manual_seed(0)
    model = va.CnnOcrModel(alphabet=AL, verbose=False, input_line_height=30, rds_line_height=30, lstm_input_dim=32, num_lstm_layers=1,
                           num_lstm_hidden_units=32, p_lstm_dropout=0.0, num_in_channels=1)
    model.train()
    return model


@pytest.mark.parametrize("step", ["train", "train_async"])
def test_training_step_with_the_criterion(step):
    model = _tiny_model()
    opt = va.make_optimizer(model, lr=1e-3)
    crit = va.MinErrorRateLoss(AL, nbest=4, ctc_weight=0.05, add_reference=True)
    g = torch.Generator().manual_seed(5)
    nb, width, L = 4, 200, 5
    batch = (torch.rand(nb, 1, 30, width, generator=g), torch.randint(1, len(AL), (nb * L,), generator=g).to(torch.int32),
             torch.full((nb,), width, dtype=torch.int32), torch.full((nb,), L, dtype=torch.int32), {})
    before = torch.cat([p.detach().reshape(-1).clone() for p in model.parameters()])
    out = (va.train if step == "train" else va.train_async)(batch, model, crit, opt)
    value = out if step == "train" else float(out.reshape(-1)[0].cpu())
    assert isinstance(value, float) and np.isfinite(value) and value > 0
    after = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert bool(torch.isfinite(after).all()) and float((after - before).abs().max()) > 0
    ops.check_health_sync(torch.device("cuda", torch.cuda.current_device()))
