"""Entropy-regularised CTC training (maximum conditional entropy, EnCTC: Liu, Jin and Zhang, NeurIPS 2018).  CTCLoss drives the
posterior over a line's feasible frame alignments onto a single spiky path; this criterion pays for that:

    loss = sum_b ( nll_b - beta * H_b ),      nll = -ln P_ctc(labels | x),   H = - sum_pi (p(pi) / P) ln (p(pi) / P)  >= 0

H the entropy of the posterior over the alignments pi of the ground truth.  It is an expectation over all alignments of the
log-probability of the alignment, which needs a second quantity carried through the alpha / beta recursion; vocr_ctc_entropy
(csrc/ctc_entropy.hip) does that, and score, entropy and the gradient of the whole criterion are ONE call of it with the constant
coefficients (w_ctc, w_ent) = (-1, -beta).  Symbol classes are the alphabet's only if a canon is given; like CTCLoss the criterion
takes label indices as they are.  No claim about accuracy is made here: beta is the user's to tune (the paper uses 0.1 .. 0.2)."""
import torch
import torch.nn as nn

from . import ops
from ._lib import call


class _EntropyCtcFn(torch.autograd.Function):
    """sum_b (nll_b - beta H_b); the gradient with respect to the logits is saved by the forward call and scaled in the backward."""

    @staticmethod
    def forward(ctx, logits, lens_dev, labels_dev, label_lens_dev, coeff, beta, keep):
        ctc, ent, dlogits = ops.ctc_entropy(logits, lens_dev, labels_dev, label_lens_dev, None, coeff)
        keep.last_nll, keep.last_entropy = -ctc, ent
        ctx.save_for_backward(dlogits)
        return ops.colsum((keep.last_nll - beta * ent).reshape(-1, 1))         # shape (1,): fixed order; +inf for a line with no path

    @staticmethod
    def backward(ctx, dloss):
        (dlogits,) = ctx.saved_tensors
        dloss = ops._f32c(dloss)
        out = torch.empty_like(dlogits)
        call("vocr_scale_dev", ops._p(dlogits), ops._p(dloss), ops._p(out), dlogits.numel(), ops._stream())
        return (out,) + (None,) * 6


class EntropyRegularizedCTCLoss(nn.Module):
    """criterion(logits [T,B,V] on the GPU, targets IntTensor [sum L] (CPU), act_lens IntTensor [B] (CPU), target_lens IntTensor [B]
    (CPU)) -> Tensor (1,) = sum over the batch of nll - beta * (alignment entropy), supporting .backward(): CTCLoss's signature and
    contract, so it goes wherever CTCLoss goes (train, train_async, loop.fit).  A line that cannot be aligned gives +inf, as with
    CTCLoss (its gradient rows are zeros).  `last_nll` and `last_entropy`: fp32 [B] device tensors of the last call, for logging."""

    def __init__(self, beta):
        super().__init__()
        beta = float(beta)
        if not beta >= 0.0 or beta == float("inf"):
            raise ValueError("EntropyRegularizedCTCLoss: need a finite beta >= 0 (beta=%r)" % (beta,))
        self.beta = beta
        self.last_nll = self.last_entropy = None

    def forward(self, acts, labels, act_lens, label_lens):
        if not acts.is_cuda:
            raise RuntimeError("vistaocr_amd.EntropyRegularizedCTCLoss needs activations on the MI355X; there is no CPU fallback")
        dev = acts.device
        T, B = int(acts.shape[0]), int(acts.shape[1])
        labels = torch.as_tensor(labels).to(torch.int32).reshape(-1).cpu()
        label_lens_c = torch.as_tensor(label_lens).to(torch.int32).reshape(-1).cpu()
        act_lens_c = torch.as_tensor(act_lens).to(torch.int32).reshape(-1).cpu()
        if label_lens_c.numel() != B or act_lens_c.numel() != B:
            raise RuntimeError("EntropyRegularizedCTCLoss: act_lens / label_lens must have one entry per batch element")
        if int(label_lens_c.sum()) != labels.numel() or int(label_lens_c.min()) < 0:
            raise RuntimeError("EntropyRegularizedCTCLoss: sum(label_lens) != len(labels)")
        if int(act_lens_c.max()) > T:
            raise RuntimeError("EntropyRegularizedCTCLoss: act_lens exceeds the time dimension")
        # the kernel takes one padded row of labels per line; a labelling longer than T has no path and keeps its first T labels and its
        # true length, which the kernel refuses (-inf, hence +inf here)
        width = max(1, min(int(label_lens_c.max()), T))
        rows = torch.zeros(B, width, dtype=torch.int32)
        cols = torch.arange(width, dtype=torch.int64).unsqueeze(0)
        take = cols < label_lens_c.to(torch.int64).unsqueeze(1)
        offsets = torch.cumsum(label_lens_c.to(torch.int64), 0) - label_lens_c.to(torch.int64)
        if labels.numel():
            rows[take] = labels[(offsets.unsqueeze(1) + cols)[take]]
        coeff = torch.tensor([-1.0, -self.beta], dtype=torch.float32).repeat(B, 1)
        # one host->device copy for the small integer arrays and the coefficients, as CTCLoss packs its four
        packed = torch.cat([rows.reshape(-1), label_lens_c, act_lens_c, coeff.reshape(-1).view(torch.int32)]).pin_memory().to(dev, non_blocking=True)
        nl = B * width
        return _EntropyCtcFn.apply(acts, packed[nl + B:nl + 2 * B], packed[:nl].view(B, width), packed[nl:nl + B],
                                   packed[nl + 2 * B:].view(torch.float32).view(B, 2), self.beta, self)
