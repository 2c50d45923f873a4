"""CTC forced alignment on the GPU (vocr_ctc_align): where in the line each character and word of a transcript sits and how sure the
network was of it.  Stands in for what the reference's confidence experiment needs and never shipped
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

    def align(self, model_output, lens, labels):
        """`labels`: per line a list of alphabet indices or a string of space-joined uxxxx tokens; or, per line, the n-best list of
        BeamDecoder.decode_nbest ((labels, scores) pairs).  Returns per line a LineAlignment(viterbi_logp, ctc_logp, chars), chars a list
        of CharAlignment(label, uxxxx, first_frame, last_frame, peak_logp, mean_logp) with inclusive frames and natural-log
        probabilities of the character's class; None where the line has no alignment (the labelling does not fit the frames, or holds
        an index outside the alphabet).  For n-best input: per line a list with one entry per hypothesis."""
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
        dev = model_output.device
        lab_d, ln_d = torch.from_numpy(lab).to(dev), torch.from_numpy(ln).to(dev)
        scores, spans, lsc = ops.ctc_align(model_output.detach(), lens, lab_d, ln_d, self.canon(dev))
        scores, spans, lsc = one_copy([scores, spans, lsc])
        rows = lines_from_arrays(lab, ln, scores, spans, lsc, self.alphabet)
        return [row[:len(h)] for row, h in zip(rows, hyps)] if nbest else [row[0] for row in rows]

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
