"""Minimum-error-rate training (Prabhavalkar et al. 2018, MWER; here over characters or words): the expected number of edit errors of
the n-best list the TEST-TIME search returns, under the model's own probabilities renormalised over that list.

    list      = decoder's n-best for the line (its LM decides which hypotheses are in it, and nothing else)
    W_q       = edit errors of hypothesis q against the ground truth (vocr_edit_stats: char_dist or word_dist)
    s_q       = ln P_ctc(hypothesis q | x), exact (vocr_ctc_nbest_grad; the search's acoustic score is only a lower bound)
    p_q       = softmax over the list of s_q
    risk      = sum_q p_q W_q
    d risk    = sum_q c_q d s_q,   c_q = p_q (W_q - risk)          (the c_q of a line sum to 0)

and the sum over q of c_q * d s_q / d logits is ONE call of vocr_ctc_nbest_grad with weights = c.  The list, the error counts, the
scores, the coefficients and the gradient stay on the device; the criterion waits for the device nowhere CTCLoss does not."""
import torch
import torch.nn as nn

from . import ops
from ._lib import call
from .ctc import CTCLoss
from .decoder import BeamDecoder, _line_lengths
from .score import ErrorScorer

_UNITS = {"char": (ops.EDIT_CHARS, 0), "word": (ops.EDIT_WORDS, 6)}      # what to ask of vocr_edit_stats, the column of the distance


def nbest_list(logits, targets, act_lens, target_lens, decoder, scorer, nbest, unit="char", add_reference=False):
    """The n-best list of every line with what the risk needs, all on the device: (labels int32 [B,n,T], lengths int32 [B,n],
    errors fp32 [B,n], ctc fp32 [B,n] = exact ln P_ctc, member bool [B,n], canon).  A hypothesis is a member iff the search filled
    its rank (total > -inf) and its exact score is finite.  `add_reference` appends the ground truth as hypothesis n (0 errors; a
    member iff it can be scored); a ground truth the search found as well is then in the list twice and counts twice."""
    if unit not in _UNITS:
        raise ValueError("unit must be 'char' or 'word' (got %r)" % (unit,))
    T, B, V = logits.shape
    dev = logits.device
    lens = _line_lengths(act_lens)
    labels, lengths, scores = decoder._search_device(logits, act_lens, int(nbest))
    canon, kinds = scorer.tables(dev)
    ref_labels, ref_lens = scorer.references(targets, target_lens, dev)
    if ref_lens.numel() != B:
        raise RuntimeError("MinErrorRateLoss: %d references for %d lines" % (ref_lens.numel(), B))
    filled = scores[:, :, 0] > float("-inf")
    if add_reference:
        if int(nbest) + 1 > 128:
            raise ValueError("add_reference needs nbest + 1 <= 128 (nbest=%d)" % nbest)
        width = int(ref_labels.shape[1])
        ref_row = ref_labels[:, :T] if width >= T else torch.nn.functional.pad(ref_labels, (0, T - width))
        labels = torch.cat([labels, ref_row.unsqueeze(1)], dim=1)          # a reference longer than T has no score: never a member
        lengths = torch.cat([lengths, ref_lens.reshape(B, 1)], dim=1)
        filled = torch.cat([filled, torch.ones(B, 1, dtype=torch.bool, device=dev)], dim=1)
    n = int(labels.shape[1])
    rows = torch.arange(B * n, dtype=torch.int32, device=dev)
    pairs = torch.stack([rows, torch.div(rows, n, rounding_mode="floor")], dim=1)
    want, col = _UNITS[unit]
    stats = ops.edit_stats(labels, lengths, ref_labels, ref_lens, pairs, V, canon, kinds if unit == "word" else None, want)
    dist = stats[:, col].view(B, n)
    ctc, _ = ops.ctc_nbest(logits.detach(), lens, labels, lengths, canon)
    member = filled & torch.isfinite(ctc) & (dist >= 0)
    return labels, lengths, dist.to(torch.float32), ctc, member, canon


def risk_terms(errors, ctc, member):
    """(risk [B], coefficients c [B,n], p [B,n]) from the list's error counts, exact scores and membership, in torch on the device.
    A line with an empty list has risk 0 and coefficients 0."""
    neg = torch.full_like(ctc, float("-inf"))
    s = torch.where(member, ctc, neg)
    top = s.max(dim=1, keepdim=True).values
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
    e = torch.where(member, torch.exp(s - top), torch.zeros_like(s))
    z = e.sum(dim=1, keepdim=True)
    p = e / torch.where(z > 0, z, torch.ones_like(z))
    w = torch.where(member, errors, torch.zeros_like(errors))
    risk = (p * w).sum(dim=1)
    return risk, p * (w - risk[:, None]), p


class _RiskFn(torch.autograd.Function):
    """The batch-summed risk of a fixed list; the gradient with respect to the logits is one vocr_ctc_nbest_grad call."""

    @staticmethod
    def forward(ctx, logits, lens, labels, lengths, canon, errors, ctc, member):
        risk, c, _ = risk_terms(errors, ctc, member)
        _, dlogits = ops.ctc_nbest(logits, lens, labels, lengths, canon, weights=c)
        ctx.save_for_backward(dlogits)
        return risk.sum().reshape(1)

    @staticmethod
    def backward(ctx, dloss):
        (dlogits,) = ctx.saved_tensors
        dloss = ops._f32c(dloss)
        out = torch.empty_like(dlogits)
        call("vocr_scale_dev", ops._p(dlogits), ops._p(dloss), ops._p(out), dlogits.numel(), ops._stream())
        return (out,) + (None,) * 7


def expected_errors(logits, targets, act_lens, target_lens, alphabet, decoder=None, nbest=8, unit="char", add_reference=False):
    """For logging: (risk fp32 [B] = the expected errors of each line's list, errors of rank 0 fp32 [B] = what the 1-best costs, nan
    where the search found nothing), device tensors, no gradient."""
    decoder = decoder if decoder is not None else BeamDecoder(alphabet, beam=max(16, int(nbest)), nbest=int(nbest))
    with torch.no_grad():
        _, _, errors, ctc, member, _ = nbest_list(logits, targets, act_lens, target_lens, decoder, ErrorScorer(alphabet), nbest, unit,
                                                  add_reference)
        risk, _, _ = risk_terms(errors, ctc, member)
        return risk, torch.where(member[:, 0], errors[:, 0], torch.full_like(risk, float("nan")))


class MinErrorRateLoss(nn.Module):
    """criterion(logits [T,B,V] on the GPU, targets IntTensor [sum L] (CPU), act_lens IntTensor [B] (CPU), target_lens IntTensor [B]
    (CPU)) -> Tensor (1,) = sum over the batch of the expected `unit` errors of `decoder`'s `nbest` list + ctc_weight * CTCLoss,
    supporting .backward(): CTCLoss's signature and contract, so it goes wherever CTCLoss goes (train, train_async, loop.fit).

    `decoder`: the BeamDecoder or WordBeamDecoder used at test time (default BeamDecoder(alphabet, beam=16, nbest=nbest)); its LM
    picks the list and does not enter the probabilities.  `ctc_weight` keeps the likelihood of the ground truth in the objective (the
    risk alone is indifferent to hypotheses outside the list); 0 switches it off.  `add_reference` appends the ground truth to the list
    (see nbest_list).  Meant for fine-tuning a model trained with CTCLoss, at a lower learning rate."""

    def __init__(self, alphabet, decoder=None, nbest=8, unit="char", ctc_weight=0.01, add_reference=False):
        super().__init__()
        if unit not in _UNITS:
            raise ValueError("MinErrorRateLoss: unit must be 'char' or 'word' (got %r)" % (unit,))
        nbest = int(nbest)
        if decoder is None:
            decoder = BeamDecoder(alphabet, beam=max(16, nbest), nbest=nbest)
        if not 1 <= nbest <= decoder.beam or nbest + (1 if add_reference else 0) > 128:
            raise ValueError("MinErrorRateLoss: need 1 <= nbest <= the decoder's beam, and nbest + 1 <= 128 with add_reference "
                             "(nbest=%d beam=%d)" % (nbest, decoder.beam))
        self.alphabet, self.decoder, self.nbest, self.unit = alphabet, decoder, nbest, unit
        self.ctc_weight, self.add_reference = float(ctc_weight), bool(add_reference)
        self.scorer = ErrorScorer(alphabet)
        self.ctc = CTCLoss()

    def forward(self, acts, labels, act_lens, label_lens):
        if not acts.is_cuda:
            raise RuntimeError("vistaocr_amd.MinErrorRateLoss needs activations on the MI355X; there is no CPU fallback")
        hyp, lengths, errors, ctc, member, canon = nbest_list(acts, labels, act_lens, label_lens, self.decoder, self.scorer, self.nbest,
                                                              self.unit, self.add_reference)
        loss = _RiskFn.apply(acts, _line_lengths(act_lens), hyp, lengths, canon, errors, ctc, member)
        if self.ctc_weight != 0.0:
            loss = loss + self.ctc_weight * self.ctc(acts, labels, act_lens, label_lens)
        return loss
