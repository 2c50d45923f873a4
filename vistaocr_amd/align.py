"""CTC forced alignment on the GPU (vocr_ctc_align): where in the line each character and word of a transcript sits and how sure the
network was of it; and CTC edit scores (vocr_ctc_edit_scores): how likely each character is to be wrong and what would stand there
instead.  Stands in for what the reference's confidence experiment needs and never shipped
(conf_utils.form_confidence_gt of src/conf_test.py): the best CTC alignment of a known label sequence to the frames.  It gives
positions and per-character scores read off the network's own posteriors; it is not a trained confidence head."""
import math
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .textutils import _DIGITS, _PUNCT

CharAlignment = namedtuple("CharAlignment", "label uxxxx first_frame last_frame peak_logp mean_logp")
WordAlignment = namedtuple("WordAlignment", "token first_frame last_frame min_conf mean_logp")
LineAlignment = namedtuple("LineAlignment", "viterbi_logp ctc_logp chars")
CharAlternatives = namedtuple("CharAlternatives", "label uxxxx posterior alternatives")
LineAlternatives = namedtuple("LineAlternatives", "ctc_logp chars gaps")


def one_copy(tensors):
    """Device tensors of shape [B, n, ...] (int32 or fp32) as host arrays, through ONE device-to-host copy."""
    B, n = tensors[0].shape[:2]
    flat = [t.contiguous().view(torch.int32).reshape(B, n, -1) for t in tensors]
    host = torch.cat(flat, dim=2).cpu().numpy()
    out, o = [], 0
    for t, f in zip(tensors, flat):
        w = f.shape[2]
        a = np.ascontiguousarray(host[:, :, o:o + w])
        o += w
        out.append((a.view(np.float32) if t.dtype == torch.float32 else a).reshape(tuple(t.shape)))
    return out


def lines_from_arrays(labels, lengths, scores, spans, label_scores, alphabet):
    """Host arrays of ops.ctc_align ([B,n,L], [B,n], [B,n,2], [B,n,M,2], [B,n,M,2]) as a [B][n] nest of LineAlignment / None."""
    idx_to_char = alphabet.idx_to_char
    out = []
    for b in range(labels.shape[0]):
        row = []
        for q in range(labels.shape[1]):
            if not np.isfinite(scores[b, q, 0]):
                row.append(None)
                continue
            chars = []
            for p in range(int(lengths[b, q])):
                first, last = int(spans[b, q, p, 0]), int(spans[b, q, p, 1])
                k = int(labels[b, q, p])
                chars.append(CharAlignment(k, idx_to_char[k], first, last, float(label_scores[b, q, p, 0]),
                                           float(label_scores[b, q, p, 1]) / (last - first + 1)))
            row.append(LineAlignment(float(scores[b, q, 0]), float(scores[b, q, 1]), chars))
        out.append(row)
    return out


def edit_posteriors(ctc, sub, dele, ins, labels, canon, topk):
    """The reduction of ops.ctc_edit_scores' outputs ([B,n], [B,n,M,V], [B,n,M], [B,n,M+1,V]) on the device.  At position p a softmax
    over the scores of {every canonical class (the label's own class: keep), deletion}; at gap q over {the unedited labelling, every
    canonical class inserted}.  Returns fp32 / int32 device tensors: keep [B,n,M], alt_post and alt_idx [B,n,M,k] (the k most probable
    other outcomes, best first; index V = deletion), nothing_missing [B,n,M+1], ins_post and ins_idx [B,n,M+1,k].  The softmax runs in
    fp64; a place where every score is -inf gives zeros."""
    B, n, M, V = sub.shape
    dev = sub.device
    cols = torch.arange(V, device=dev)
    classes = (canon.long() == cols) & (cols > 0) if canon is not None else cols > 0
    own = torch.zeros(B, n, M, dtype=torch.long, device=dev)
    own[:, :, :labels.shape[2]] = labels[:, :, :M].long().clamp(0, V - 1)       # labels may be narrower than M (no label at all)
    if canon is not None:
        own = canon.long()[own]
    neg = float("-inf")
    chars = torch.cat([sub.double().masked_fill(~classes, neg), dele.double().unsqueeze(-1)], dim=-1)
    gaps = torch.cat([ins.double().masked_fill(~classes, neg), ctc.double()[:, :, None, None].expand(B, n, M + 1, 1)], dim=-1)
    chars, gaps = torch.softmax(chars, dim=-1).nan_to_num(0.0), torch.softmax(gaps, dim=-1).nan_to_num(0.0)
    keep = chars.gather(3, own.unsqueeze(-1)).squeeze(-1)
    k = max(1, min(int(topk), V - 1))
    alt_post, alt_idx = chars.scatter(3, own.unsqueeze(-1), -1.0).topk(k, dim=-1)
    ins_post, ins_idx = gaps[..., :V].topk(k, dim=-1)
    return (keep.float(), alt_post.float(), alt_idx.int(), gaps[..., V].float().contiguous(), ins_post.float(), ins_idx.int())


def alternatives_from_device(model_output, lens, labels, lengths, canon, alphabet, topk, extra=()):
    """vocr_ctc_edit_scores on device labellings [B,n,L] / [B,n], the reduction on the device, ONE device-to-host copy, formatting.
    Returns (a [B][n] nest of LineAlternatives, None for a rank with a negative length or an index outside the alphabet; the host
    arrays of labels, lengths and of every tensor of `extra`, which share the copy)."""
    ctc, sub, dele, ins = ops.ctc_edit_scores(model_output.detach(), lens, labels, lengths, canon)
    reduced = edit_posteriors(ctc, sub, dele, ins, labels, canon, topk)
    host = one_copy([labels, lengths, ctc.unsqueeze(-1)] + list(reduced) + list(extra))
    lab, ln, ctc, keep, alt_post, alt_idx, nothing, ins_post, ins_idx = host[:9]
    idx_to_char = alphabet.idx_to_char
    V, M = int(sub.shape[3]), int(sub.shape[2])

    def ranked(post, idx):
        return [(idx_to_char[int(i)] if i < V else None, float(v)) for v, i in zip(post, idx) if v > 0]

    out = []
    for b in range(lab.shape[0]):
        row = []
        for q in range(lab.shape[1]):
            L = int(ln[b, q])
            if L < 0 or L > M or any(k <= 0 or k >= V for k in lab[b, q, :L]):
                row.append(None)
                continue
            chars = [CharAlternatives(int(lab[b, q, p]), idx_to_char[int(lab[b, q, p])], float(keep[b, q, p]),
                                      ranked(alt_post[b, q, p], alt_idx[b, q, p])) for p in range(L)]
            gaps = [(float(nothing[b, q, g]), ranked(ins_post[b, q, g], ins_idx[b, q, g])) for g in range(L + 1)]
            row.append(LineAlternatives(float(ctc[b, q, 0]), chars, gaps))
        out.append(row)
    return out, [lab, ln] + host[9:]


class CtcAligner:
    """Aligns transcripts (ground truth or any decoder's output) to the model's output frames."""

    def __init__(self, alphabet):
        self.alphabet = alphabet
        self._canon = {}

    def canon(self, dev):
        key = str(dev)
        if key not in self._canon:
            self._canon[key] = torch.as_tensor(self.alphabet.canonical_indices(), dtype=torch.int32).to(dev)
        return self._canon[key]

    def _labels(self, line):
        if isinstance(line, str):
            return [self.alphabet.char_to_idx[tok] for tok in line.split()]
        return [int(v) for v in line]

    def _pack(self, labels):
        """align's `labels` forms as (per line the list of labellings, whether the input was n-best, int32 [B,n,L], int32 [B,n])."""
        nbest = any(len(line) > 0 and isinstance(line[0], tuple) for line in labels if not isinstance(line, str))
        hyps = [[self._labels(h[0]) for h in line] for line in labels] if nbest else [[self._labels(line)] for line in labels]
        B, n = len(hyps), max([len(h) for h in hyps] + [1])
        L = max([len(x) for h in hyps for x in h] + [1])
        lab = np.zeros((B, n, L), dtype=np.int32)
        ln = np.full((B, n), -1, dtype=np.int32)               # a rank the line does not have: no alignment
        for b, h in enumerate(hyps):
            for q, x in enumerate(h):
                lab[b, q, :len(x)] = x
                ln[b, q] = len(x)
        return hyps, nbest, lab, ln

    def align(self, model_output, lens, labels):
        """`labels`: per line a list of alphabet indices or a string of space-joined uxxxx tokens; or, per line, the n-best list of
        BeamDecoder.decode_nbest ((labels, scores) pairs).  Returns per line a LineAlignment(viterbi_logp, ctc_logp, chars), chars a list
        of CharAlignment(label, uxxxx, first_frame, last_frame, peak_logp, mean_logp) with inclusive frames and natural-log
        probabilities of the character's class; None where the line has no alignment (the labelling does not fit the frames, or holds
        an index outside the alphabet).  For n-best input: per line a list with one entry per hypothesis."""
        hyps, nbest, lab, ln = self._pack(labels)
        dev = model_output.device
        lab_d, ln_d = torch.from_numpy(lab).to(dev), torch.from_numpy(ln).to(dev)
        scores, spans, lsc = ops.ctc_align(model_output.detach(), lens, lab_d, ln_d, self.canon(dev))
        scores, spans, lsc = one_copy([scores, spans, lsc])
        rows = lines_from_arrays(lab, ln, scores, spans, lsc, self.alphabet)
        return [row[:len(h)] for row, h in zip(rows, hyps)] if nbest else [row[0] for row in rows]

    def alternatives(self, model_output, lens, labels, topk=3):
        """How likely each character of a transcript is to be wrong, and what would stand there instead.  `labels` as for align().
        Returns per line (for n-best input: per hypothesis) a LineAlternatives(ctc_logp, chars, gaps), or None for a labelling with an
        index outside the alphabet:
          chars[p] = CharAlternatives(label, uxxxx, posterior, alternatives), alternatives the up to `topk` most probable other
                     outcomes at p as (uxxxx, posterior), best first, uxxxx None for "no character here" (deletion);
          gaps[q]  = (posterior_nothing_missing, [(uxxxx, posterior), ...]) for q = 0 .. len(chars): a character missing before
                     chars[q] (q = len(chars): at the end).
        WHAT THE POSTERIOR IS: vocr_ctc_edit_scores gives the exact CTC score ln P_ctc(labelling' | x) of every labelling one edit away
        from the transcript.  The posterior at p is exp(score) normalised over the labellings that differ from the transcript AT THAT
        ONE PLACE only - p kept, p replaced by each other symbol, p deleted (a gap: nothing inserted, each symbol inserted) - with all
        other characters held fixed.  It is exact under the CTC model for that conditional question.  It is not a lattice posterior over
        all labellings (two neighbouring errors are never weighed together), and it is not a trained confidence head.  A symbol is an
        alphabet string: indices with the same string are one outcome.  A labelling that does not fit its frames has posterior 0 at
        every kept character and may have a deletion with posterior 1.  The scores are reduced and ranked on the device; one
        device-to-host copy."""
        hyps, nbest, lab, ln = self._pack(labels)
        dev = model_output.device
        rows, _ = alternatives_from_device(model_output, lens, torch.from_numpy(lab).to(dev), torch.from_numpy(ln).to(dev),
                                           self.canon(dev), self.alphabet, topk)
        return [row[:len(h)] for row, h in zip(rows, hyps)] if nbest else [row[0] for row in rows]

    def entropy(self, model_output, lens, labels):
        """How far the spans of align() can be trusted: per line (ln P_ctc, H, H / len), H the entropy in nats of the posterior over
        the transcript's feasible frame alignments (vocr_ctc_entropy, scores only) and len the line's frames.  H = 0: one alignment holds
        all the mass and the Viterbi spans are the only reading; H / len near ln 2 or above: the frames are spread over many alignments
        and a span is good to several frames at best.  `labels`: per line a list of alphabet indices or a string of space-joined uxxxx
        tokens (no n-best lists).  A transcript without an alignment gives (-inf, 0.0, 0.0).  One device-to-host copy."""
        hyps, nbest, lab, ln = self._pack(labels)
        if nbest:
            raise ValueError("CtcAligner.entropy takes one transcript per line, not n-best lists")
        dev = model_output.device
        T = int(model_output.shape[0])
        ctc, ent, _ = ops.ctc_entropy(model_output.detach(), lens, torch.from_numpy(lab[:, 0]).to(dev), torch.from_numpy(ln[:, 0]).to(dev),
                                      self.canon(dev))
        ctc, ent = one_copy([ctc.reshape(-1, 1, 1), ent.reshape(-1, 1, 1)])
        frames = [min(max(int(v), 0), T) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
        return [(float(c), float(h), float(h) / n if n else 0.0) for c, h, n in zip(ctc.reshape(-1), ent.reshape(-1), frames)]

    def words(self, alignment):
        """The tokens of textutils.form_tokenized_words over the line's characters (u0020 separates words and is no token, every
        punctuation mark and digit is a token of its own), each a WordAlignment(token, first_frame, last_frame, min_conf, mean_logp):
        the frames from its first character's first to its last character's last, min_conf the minimum over its characters of
        exp(peak_logp), mean_logp the mean frame log-probability over its characters' frames."""
        out, cur = [], []

        def close():
            if cur:
                frames = sum(c.last_frame - c.first_frame + 1 for c in cur)
                total = sum(c.mean_logp * (c.last_frame - c.first_frame + 1) for c in cur)
                out.append(WordAlignment("_".join(c.uxxxx for c in cur), cur[0].first_frame, cur[-1].last_frame,
                                         min(math.exp(c.peak_logp) for c in cur), total / frames))
                del cur[:]

        for c in alignment.chars:
            if c.uxxxx == "u0020":
                close()
            elif c.uxxxx in _PUNCT or c.uxxxx in _DIGITS:
                close()
                cur.append(c)
                close()
            else:
                cur.append(c)
        close()
        return out

    def pixel_spans(self, alignment, input_width, n_frames):
        """(x0, x1) in input pixels for every character of a LineAlignment, or for every item of a list of CharAlignment /
        WordAlignment.  Frame t of a line with n frames and w input pixels is taken to cover [t*w/n, (t+1)*w/n), so a span is
        (floor(first*w/n), ceil((last+1)*w/n)).  This is the MEAN geometry of the stack only: the FractionalMaxPool regions are drawn
        per forward pass and the recurrent layers see the whole line, so a box is good to about one frame width (w/n pixels), not
        better."""
        items = alignment.chars if isinstance(alignment, LineAlignment) else alignment
        w, n = int(input_width), int(n_frames)
        return [((it.first_frame * w) // n, -((-(it.last_frame + 1) * w) // n)) for it in items]
