"""Scoring hypotheses against references on the GPU (vocr_edit_stats): the CER / WER of compute_cer_wer (textutils), the oracle error
rate of an n-best list and the COPY / SUB / INS / DEL trace that error analysis starts from - without the hypotheses leaving the
device and without a Python loop over characters.

Characters are compared as the alphabet's symbol strings (indices with the same string are one character, as everywhere in this
package); words are form_tokenized_words' tokens.  The hypothesis is always the first sequence and the reference the second: an INS is a
hypothesis element the reference does not have, a DEL a reference element the hypothesis lacks.  Everything is integer arithmetic and
equals the cell-by-cell DP bit for bit."""
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .align import one_copy
from .lm import class_kinds

ErrorStats = namedtuple("ErrorStats", ops.EDIT_FIELDS + ("cer", "wer", "ops", "confusion"))
OracleStats = namedtuple("OracleStats", "rank char_dist oracle_cer oracle_wer top_cer top_wer mean_oracle_cer mean_oracle_wer "
                                        "mean_top_cer mean_top_wer")


def _rates(stats):
    """(cer, wer) float64 of int stats [..., 12]; nan where the pair was invalid."""
    with np.errstate(invalid="ignore"):
        cer = stats[..., 0].astype(np.float64) / np.maximum(stats[..., 5], 1)
        wer = stats[..., 6].astype(np.float64) / np.maximum(stats[..., 11], 1)
    cer[stats[..., 0] < 0] = np.nan
    wer[stats[..., 6] < 0] = np.nan
    return cer, wer


class ErrorScorer:
    """Edit statistics of hypotheses against references for one alphabet."""

    def __init__(self, alphabet):
        self.alphabet = alphabet
        self._tables = {}

    def tables(self, dev):
        """(canon, kinds) int32 [V] on `dev`, made once per device."""
        key = str(dev)
        if key not in self._tables:
            self._tables[key] = (torch.as_tensor(self.alphabet.canonical_indices(), dtype=torch.int32).to(dev),
                                 torch.from_numpy(class_kinds(self.alphabet)).to(dev))
        return self._tables[key]

    def references(self, targets, target_lens, dev):
        """References as (int32 [B,L] labels, int32 [B] lengths) on `dev`: from the collate's form (flat `targets` + `target_lens`,
        packed on the host) or from padded [B,L] labels (taken as they are).  The flat form is packed from host values: `targets` and
        `target_lens` on the device are copied to the host first, which waits for the device - pass padded labels to avoid that."""
        lens = torch.as_tensor(target_lens).reshape(-1).to(torch.int32)
        targets = torch.as_tensor(targets)
        if targets.dim() == 2:
            if targets.shape[0] != lens.numel():
                raise RuntimeError("ErrorScorer: %d reference rows for %d lengths" % (targets.shape[0], lens.numel()))
            return targets.to(device=dev, dtype=torch.int32).contiguous(), lens.to(dev)
        if targets.dim() != 1:
            raise RuntimeError("ErrorScorer: targets must be flat [sum of target_lens] or padded [B,L] (got %s)" % (tuple(targets.shape),))
        ln = lens.cpu().numpy().astype(np.int64)
        flat = targets.cpu().numpy()
        if int(ln.sum()) != flat.size or (ln < 0).any():
            raise RuntimeError("ErrorScorer: target_lens sum to %d, targets holds %d labels" % (int(ln.sum()), flat.size))
        B, L = ln.size, max(int(ln.max()) if ln.size else 0, 1)
        pad = np.zeros((B, L), dtype=np.int32)
        pad[np.arange(L)[None, :] < ln[:, None]] = flat            # row-major: line after line
        return torch.from_numpy(pad).to(dev), lens.to(dev)

    def _stats(self, hyp_labels, hyp_lens, ref_labels, ref_lens, pairs, trace):
        dev = hyp_labels.device
        canon, kinds = self.tables(dev)
        V = len(self.alphabet)
        want = ops.EDIT_CHARS | ops.EDIT_WORDS | (ops.EDIT_TRACE if trace else 0)
        if not trace:
            return ops.edit_stats(hyp_labels, hyp_lens, ref_labels, ref_lens, pairs, V, canon, kinds, want), None, None
        conf = torch.zeros(V, V, dtype=torch.int32, device=dev)
        stats, tr = ops.edit_stats(hyp_labels, hyp_lens, ref_labels, ref_lens, pairs, V, canon, kinds, want, confusion=conf, ops=True)
        return stats, tr, conf

    def score(self, hyp_labels, hyp_lens, targets, target_lens, trace=False):
        """Hypotheses `hyp_labels` int32 [B,T] or [B,n,T] and `hyp_lens` int32 [B] or [B,n] on the device (vocr_greedy_collapse's or a
        beam search's outputs as they are) against line b's reference: `targets` flat with `target_lens` (the collate's form) or
        padded [B,L].  Returns ErrorStats of host arrays shaped [B] or [B,n] after ONE device-to-host copy: the twelve integers
        (ops.EDIT_FIELDS; the sub / ins / del counts are -1 without `trace`), cer = char_dist / max(ref_chars, 1) and wer likewise over
        words (float64; nan for an invalid pair).

        For every reference with at least one word these are the very floats compute_cer_wer returns; so they are for an empty
        reference against any hypothesis that holds a word or nothing at all (the reference's "".split(" ") quirk gives the same
        quotient).  Where compute_cer_wer divides by zero (a reference of spaces only) this returns the distance over 1; and an empty
        reference against a hypothesis of spaces only has WER 0 here, where the quirk's one empty word makes it 1 there.

        With `trace` also: ops = uint8 [B(,n),S] the character trace from the front (1 COPY, 2 SUB, 3 INS, 4 DEL, 0 past the end) and
        confusion = int32 [V,V] over all pairs ([reference class][hypothesis class]; INS in row 0, DEL in column 0)."""
        if hyp_labels.dim() not in (2, 3) or tuple(hyp_lens.shape) != tuple(hyp_labels.shape[:-1]):
            raise RuntimeError("ErrorScorer.score: hyp_labels must be [B,T] or [B,n,T] and hyp_lens [B] or [B,n] (got %s, %s)"
                               % (tuple(hyp_labels.shape), tuple(hyp_lens.shape)))
        ops._need_gpu(hyp_labels, hyp_lens)
        dev = hyp_labels.device
        squeeze = hyp_labels.dim() == 2
        B = int(hyp_labels.shape[0])
        n = 1 if squeeze else int(hyp_labels.shape[1])
        ref_labels, ref_lens = self.references(targets, target_lens, dev)
        if ref_lens.numel() != B:
            raise RuntimeError("ErrorScorer.score: %d references for %d lines" % (ref_lens.numel(), B))
        rows = torch.arange(B * n, dtype=torch.int32, device=dev)
        pairs = torch.stack([rows, torch.div(rows, n, rounding_mode="floor")], dim=1)
        stats, tr, conf = self._stats(hyp_labels.reshape(B * n, int(hyp_labels.shape[-1])), hyp_lens.reshape(-1), ref_labels, ref_lens,
                                      pairs, trace)
        return self._result(stats, tr, conf, (B,) if squeeze else (B, n))

    def _result(self, stats, tr, conf, shape):
        if tr is None:
            st, = one_copy([stats.view(1, 1, -1)])
            tr_h = conf_h = None
        else:
            S, nbytes = int(tr.shape[1]), tr.numel()
            packed = torch.nn.functional.pad(tr.reshape(-1), (0, -nbytes % 4)).view(torch.int32)    # the bytes as they are, 4 to a word
            st, tr_h, conf_h = one_copy([stats.view(1, 1, -1), packed.view(1, 1, -1), conf.view(1, 1, -1)])
            tr_h = np.ascontiguousarray(tr_h).view(np.uint8).reshape(-1)[:nbytes].reshape(shape + (S,))
            conf_h = conf_h.reshape(tuple(conf.shape))
        st = st.reshape(shape + (12,))
        cer, wer = _rates(st)
        return ErrorStats(*([np.ascontiguousarray(st[..., k]) for k in range(12)] + [cer, wer, tr_h, conf_h]))

    def labels(self, text):
        """A uxxxx string ("u0061 u0020 u0062"; "" is the empty line) as alphabet indices."""
        toks = text.split()
        missing = [t for t in toks if t not in self.alphabet.char_to_idx]
        if missing:
            raise ValueError("not in the alphabet: " + " ".join(missing))
        return [self.alphabet.char_to_idx[t] for t in toks]

    def score_strings(self, hyps, refs, trace=False, device="cuda"):
        """score() for callers that hold uxxxx strings instead of labels: `hyps` and `refs`, two lists of the same length, are packed
        on the host and scored by the same kernel.  Returns ErrorStats shaped [len(hyps)]."""
        hyps, refs = list(hyps), list(refs)
        if len(hyps) != len(refs) or not hyps:
            raise ValueError("score_strings: need as many hypotheses as references, and at least one (%d, %d)" % (len(hyps), len(refs)))
        hl, rl = [self.labels(h) for h in hyps], [self.labels(r) for r in refs]
        pad = np.zeros((len(hl), max([len(h) for h in hl] + [1])), dtype=np.int32)
        for i, h in enumerate(hl):
            pad[i, :len(h)] = h
        dev = torch.device(device)
        return self.score(torch.from_numpy(pad).to(dev), torch.as_tensor([len(h) for h in hl], dtype=torch.int32).to(dev),
                          torch.as_tensor([v for r in rl for v in r], dtype=torch.int32), torch.as_tensor([len(r) for r in rl],
                                                                                                         dtype=torch.int32), trace=trace)

    def oracle(self, labels, lengths, scores, targets, target_lens):
        """The oracle error rate of an n-best list: `labels` [B,n,T], `lengths` [B,n], `scores` [B,n,3] as a beam search returns them
        (on the device), references as for score().  Per line the rank with the lowest character distance (ties go to the better
        rank; ranks the search did not fill - total -inf - are never chosen; a line with none filled answers rank 0).  Returns OracleStats
        of host values: rank [B], char_dist [B,n] (every rank's), that rank's and rank 0's cer / wer [B], and the four batch means.  All n * B
        pairs are scored for distances only; words are counted for the 2 * B pairs reported.  One device-to-host copy."""
        if labels.dim() != 3 or tuple(lengths.shape) != tuple(labels.shape[:2]) or tuple(scores.shape[:2]) != tuple(labels.shape[:2]):
            raise RuntimeError("ErrorScorer.oracle: labels [B,n,T], lengths [B,n], scores [B,n,3] (got %s, %s, %s)"
                               % (tuple(labels.shape), tuple(lengths.shape), tuple(scores.shape)))
        ops._need_gpu(labels, lengths, scores)
        dev = labels.device
        B, n = int(labels.shape[0]), int(labels.shape[1])
        canon, kinds = self.tables(dev)
        V = len(self.alphabet)
        ref_labels, ref_lens = self.references(targets, target_lens, dev)
        if ref_lens.numel() != B:
            raise RuntimeError("ErrorScorer.oracle: %d references for %d lines" % (ref_lens.numel(), B))
        rows = torch.arange(B * n, dtype=torch.int32, device=dev)
        pairs = torch.stack([rows, torch.div(rows, n, rounding_mode="floor")], dim=1)
        a, al = labels.reshape(B * n, int(labels.shape[-1])), lengths.reshape(-1)
        dist = ops.edit_stats(a, al, ref_labels, ref_lens, pairs, V, canon, None, ops.EDIT_CHARS)[:, 0].view(B, n)
        filled = (scores[:, :, 0] != float("-inf")) & (dist >= 0)
        big = torch.iinfo(torch.int32).max
        key = torch.where(filled, dist.to(torch.int64), torch.full_like(dist, big, dtype=torch.int64)) * n \
            + torch.arange(n, device=dev, dtype=torch.int64)[None, :]
        rank = torch.argmin(key, dim=1)                            # the keys of a line are all different
        rank = torch.where(filled.any(dim=1), rank, torch.zeros_like(rank)).to(torch.int32)
        line = torch.arange(B, dtype=torch.int32, device=dev)
        two = torch.cat([torch.stack([line * n + rank, line], dim=1), torch.stack([line * n, line], dim=1)], dim=0)
        st2 = ops.edit_stats(a, al, ref_labels, ref_lens, two, V, canon, kinds, ops.EDIT_CHARS | ops.EDIT_WORDS)
        rank_h, dist_h, st2_h = one_copy([rank.view(1, 1, -1), dist.reshape(1, 1, -1), st2.view(1, 1, -1)])
        st2_h = st2_h.reshape(2, B, 12)
        cer, wer = _rates(st2_h)
        return OracleStats(rank_h.reshape(B), dist_h.reshape(B, n), cer[0], wer[0], cer[1], wer[1],
                           float(np.mean(cer[0])), float(np.mean(wer[0])), float(np.mean(cer[1])), float(np.mean(wer[1])))

    def confusions(self, matrix, top=None):
        """The non-zero off-diagonal cells of a confusion matrix as (reference uxxxx or "<ins>", hypothesis uxxxx or "<del>", count),
        largest count first (then by reference and hypothesis index); `top`: at most that many."""
        m = np.asarray(matrix)
        r, h = np.nonzero(m)
        cells = sorted(((-int(m[i, j]), int(i), int(j)) for i, j in zip(r, h) if i != j))
        idx = self.alphabet.idx_to_char
        out = [("<ins>" if i == 0 else idx[i], "<del>" if j == 0 else idx[j], -c) for c, i, j in cells]
        return out if top is None else out[:int(top)]
