"""Greedy (best-path) CTC decoding: ArgmaxDecoder (src/decoder.py:112-185) == CnnOcrModel.decode_without_lm
(src/models/cnnlstm.py:479-541).  The per-frame argmax/max runs on the GPU (vocr_argmax_rows); one D2H copy of
int32[T,B] + float32[T,B] replaces the reference's T per-frame copies of the full logits."""
import numpy as np
import torch

from . import ops
from .align import alternatives_from_device, lines_from_arrays, one_copy
from .grammar import Grammar, pack_dense_grammars
from .textutils import uxxxx_to_utf8


def _frame_argmax(model_output):
    idx, mx = ops.argmax_rows(model_output.detach())
    return idx.cpu().numpy(), mx.cpu().numpy()


def greedy_label_sequences(model_output, batch_actual_timesteps, alphabet):
    """Integer label sequences (the emitted argmax indices) and uxxxx strings, with the reference's rules:
    blank resets; a maximum below 3/len(alphabet) (RAW activation) resets; repeats collapse by comparing the
    alphabet strings."""
    min_prob_thresh = 3 * 1 / len(alphabet)
    T, B = model_output.size()[0], model_output.size()[1]
    argmax_idxs, argmaxs = _frame_argmax(model_output)
    lens = [int(v) for v in batch_actual_timesteps]
    labels = [[] for _ in range(B)]
    result = ["" for _ in range(B)]
    idx_to_char = alphabet.idx_to_char
    for b in range(B):
        n = min(lens[b], T)
        ks = argmax_idxs[:n, b]
        low = argmaxs[:n, b] < min_prob_thresh          # same numpy float32-vs-python-float comparison as the reference
        prev = ""
        toks = []
        for t in range(n):
            k = int(ks[t])
            if k == 0 or low[t]:
                prev = ""
                continue
            ch = idx_to_char[k]
            if prev == ch:
                continue
            toks.append(ch)
            labels[b].append(k)
            prev = ch
        result[b] = " ".join(toks)
    return result, labels


def decode_greedy(model_output, batch_actual_timesteps, alphabet, uxxxx=False):
    result, _ = greedy_label_sequences(model_output, batch_actual_timesteps, alphabet)
    if uxxxx == False:  # noqa: E712  (mirrors the reference's comparison)
        result = [uxxxx_to_utf8(r) for r in result]
    return result


def greedy_labels_device(model_output, batch_actual_timesteps, alphabet):
    """Device-side collapse (vocr_greedy_collapse): returns a list of int lists without any host loop over T.
    The threshold is applied in float32 on the device."""
    dev = model_output.device
    idx, mx = ops.argmax_rows(model_output.detach())
    lens_dev = torch.as_tensor([int(v) for v in batch_actual_timesteps], dtype=torch.int32).to(dev)
    canon = torch.as_tensor(alphabet.canonical_indices(), dtype=torch.int32).to(dev)
    labels, counts = ops.greedy_collapse(idx, mx, lens_dev, canon, np.float32(3 * 1 / len(alphabet)))
    labels, counts = labels.cpu().numpy(), counts.cpu().numpy()
    return [[int(v) for v in labels[b, :counts[b]]] for b in range(labels.shape[0])]


class ArgmaxDecoder:
    def __init__(self, alphabet):
        self.alphabet = alphabet

    def decode(self, model_output, batch_actual_timesteps, uxxxx=False, lang=None):
        alphabet = self.alphabet if lang is None else self.alphabet[lang]
        return decode_greedy(model_output, batch_actual_timesteps, alphabet, uxxxx=uxxxx)

    def decode_aligned(self, model_output, batch_actual_timesteps, uxxxx=False, lang=None):
        """(hypotheses as decode() returns them, per line a LineAlignment of that hypothesis: vistaocr_amd.align).  The collapse runs on
        the device (vocr_greedy_collapse) and its labels go to vocr_ctc_align without leaving it; one device-to-host copy at the end."""
        alphabet = self.alphabet if lang is None else self.alphabet[lang]
        dev = model_output.device
        lens = _line_lengths(batch_actual_timesteps)
        idx, mx = ops.argmax_rows(model_output.detach())
        lens_dev = torch.as_tensor(lens, dtype=torch.int32).to(dev)
        canon = torch.as_tensor(alphabet.canonical_indices(), dtype=torch.int32).to(dev)
        labels, counts = ops.greedy_collapse(idx, mx, lens_dev, canon, np.float32(3 * 1 / len(alphabet)))
        labels, counts = labels.unsqueeze(1), counts.unsqueeze(1)
        return _aligned(model_output, lens_dev, labels, counts, None, canon, alphabet, uxxxx, 1)

    def decode_alternatives(self, model_output, batch_actual_timesteps, topk=3, uxxxx=False, lang=None):
        """(hypotheses as decode() returns them, per line a LineAlternatives of that hypothesis: CtcAligner.alternatives says what its
        posteriors are).  The collapse's labels go to vocr_ctc_edit_scores on the device; one device-to-host copy at the end."""
        alphabet = self.alphabet if lang is None else self.alphabet[lang]
        dev = model_output.device
        lens_dev = torch.as_tensor(_line_lengths(batch_actual_timesteps), dtype=torch.int32).to(dev)
        idx, mx = ops.argmax_rows(model_output.detach())
        canon = torch.as_tensor(alphabet.canonical_indices(), dtype=torch.int32).to(dev)
        labels, counts = ops.greedy_collapse(idx, mx, lens_dev, canon, np.float32(3 * 1 / len(alphabet)))
        return _alternatives(model_output, lens_dev, labels.unsqueeze(1), counts.unsqueeze(1), None, canon, alphabet, uxxxx, topk)


class _SearchDecoder:
    """What the three beam-search decoders share: the beam limits, the alphabet's symbol classes on each device, and the output formats
    of one search.  A decoder adds its constructor and _search_device(model_output, batch_actual_timesteps, nbest, ...) -> the device
    tensors (labels [B,nbest,T], lengths [B,nbest], scores [B,nbest,3]) of its ops.ctc_*_search; what a public method gets beyond its
    own arguments goes to _search_device as it came (GrammarBeamDecoder: which=)."""

    def __init__(self, alphabet, beam, nbest):
        if not 1 <= int(beam) <= 128 or not 1 <= int(nbest) <= int(beam):
            raise ValueError("%s: need 1 <= nbest <= beam <= 128 (beam=%s nbest=%s)" % (type(self).__name__, beam, nbest))
        self.alphabet = alphabet
        self.beam, self.nbest = int(beam), int(nbest)
        self._canon = {}

    def _canon_on(self, dev):
        """(the alphabet's canonical indices as an int32 tensor on `dev`, made once per device; whether this call made it)"""
        key = str(dev)
        new = key not in self._canon
        if new:
            self._canon[key] = torch.as_tensor(self.alphabet.canonical_indices(), dtype=torch.int32).to(dev)
        return self._canon[key], new

    def _search(self, model_output, batch_actual_timesteps, nbest, *more, **kw):
        labels, lengths, scores = self._search_device(model_output, batch_actual_timesteps, nbest, *more, **kw)
        return labels.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy()

    def decode_aligned(self, model_output, batch_actual_timesteps, uxxxx=False, nbest=1, *more, **kw):
        """(hypotheses as decode() returns them, alignments): the search, then vocr_ctc_align on its device outputs, one device-to-host
        copy at the end.  nbest = 1: per line the LineAlignment (vistaocr_amd.align) of the best hypothesis, None where the search
        found none.  nbest > 1: per line a list of (labels, (total, acoustic, lm), LineAlignment), best first, as decode_nbest lists
        them.  An alignment's ctc_logp is the full forward score of the labelling; the search's acoustic score sums only the paths its
        beam kept, so it is a lower bound of it and equals it when the beam pruned nothing of weight."""
        labels, lengths, scores = self._search_device(model_output, batch_actual_timesteps, int(nbest), *more, **kw)
        return _aligned(model_output, _line_lengths(batch_actual_timesteps), labels, lengths, scores,
                        self._canon[str(model_output.device)], self.alphabet, uxxxx, int(nbest))

    def decode_alternatives(self, model_output, batch_actual_timesteps, topk=3, uxxxx=False, *more, **kw):
        """(hypotheses as decode() returns them, per line a LineAlternatives of the best hypothesis, None where the search found none):
        the search, then vocr_ctc_edit_scores on its device outputs, one device-to-host copy at the end.  The posteriors
        (CtcAligner.alternatives says what they are) are those of the CTC model alone: the LM and the grammar rank the search, not the
        edits, so an alternative may leave the grammar's language."""
        labels, lengths, scores = self._search_device(model_output, batch_actual_timesteps, 1, *more, **kw)
        return _alternatives(model_output, _line_lengths(batch_actual_timesteps), labels, lengths, scores,
                             self._canon[str(model_output.device)], self.alphabet, uxxxx, topk)

    def decode_nbest(self, model_output, batch_actual_timesteps, nbest=None, *more, **kw):
        """Per line, a list of up to `nbest` (labels, (total, acoustic, lm)) best first, an empty list where the search found none;
        labels are canonical alphabet indices, acoustic the CTC log-probability of the labelling, lm the LM log-probability including
        </s> (0 without an LM; WordBeamDecoder: of the tokens, and a line whose every beam ends inside a word that cannot close has no
        hypothesis; GrammarBeamDecoder: every labelling is accepted by the line's grammar)."""
        nbest = self.nbest if nbest is None else int(nbest)
        return _nbest_lists(*self._search(model_output, batch_actual_timesteps, nbest, *more, **kw))

    def decode(self, model_output, batch_actual_timesteps, uxxxx=False, lang=None, *more, **kw):
        """The best hypothesis of each line in decode_greedy's format: space-joined uxxxx tokens, converted to utf8 unless uxxxx ("" for
        a line without one)."""
        if lang is not None:
            raise ValueError("%s: one alphabet per decoder (lang is not supported)" % type(self).__name__)
        return _best_strings(*self._search(model_output, batch_actual_timesteps, 1, *more, **kw), self.alphabet, uxxxx)


class BeamDecoder(_SearchDecoder):
    """CTC prefix beam search on the GPU (vocr_ctc_beam_search), optionally with a character n-gram LM (vistaocr_amd.lm.CharNgramLM):
    the stand-in for the reference's LM decode (decode_with_lm, src/decoder.py:11-109).  Hypotheses are ranked by
    ln P_ctc(y | x) + lm_weight * ln P_lm(y </s>) + insertion_bonus * |y|; `prune_logp` (None: off) skips extensions by symbols whose
    frame log-probability is below it.  Symbols with the same alphabet string are one symbol, as in the greedy decode."""

    def __init__(self, alphabet, beam=16, nbest=1, lm=None, lm_weight=0.0, insertion_bonus=0.0, prune_logp=None):
        super().__init__(alphabet, beam, nbest)
        if lm is not None and lm.logp.shape[1] != len(alphabet):
            raise ValueError("BeamDecoder: the LM was resolved for %d symbols, the alphabet has %d" % (lm.logp.shape[1], len(alphabet)))
        self.lm, self.lm_weight, self.insertion_bonus, self.prune_logp = lm, float(lm_weight), float(insertion_bonus), prune_logp

    def _search_device(self, model_output, batch_actual_timesteps, nbest):
        dev = model_output.device
        return ops.ctc_beam_search(model_output.detach(), _line_lengths(batch_actual_timesteps), self._canon_on(dev)[0], self.beam, nbest,
                                   self.lm.to(dev) if self.lm is not None else None, self.lm_weight, self.insertion_bonus,
                                   self.prune_logp)


class GrammarBeamDecoder(_SearchDecoder):
    """Grammar-constrained CTC prefix beam search on the GPU (vocr_ctc_grammar_beam_search): what the line READS, given that it is a
    date, an amount or one of these part numbers.  BeamDecoder's search, LM, ranking and output formats, restricted to the labellings a
    Grammar (vistaocr_amd.grammar) accepts: each beam carries its automaton state, and a prefix that the frames left cannot complete
    leaves the beam at once.  `grammars`: one Grammar or a list; `which=` on the public methods takes one index into the list per line
    (None: grammar 0 for every line).  A line whose language nothing in the beam reaches (or that needs more symbols than the line has
    frames) has no hypothesis: "" / None / an empty n-best list, as with the other decoders.  It is a beam search: not exact beyond
    the beam; the automata are deterministic.  WEIGHTED grammars (Grammar.boost: hot words; Grammar.from_words(log_weights=): a prior
    over a lexicon; Grammar.from_ngram) add grammar_weight * (the weight of the labelling under its grammar) to a hypothesis's rank,
    prefix by prefix, next to the LM term (vocr_ctc_grammar_beam_search_weighted); decode_nbest(grammar_scores=True) lists that weight
    as a fourth score.  The sweep kernels' 8192 cells do not apply: the dense tables are bounded by `max_table_bytes` alone."""

    def __init__(self, alphabet, grammars, beam=16, nbest=1, lm=None, lm_weight=0.0, insertion_bonus=0.0, prune_logp=None,
                 max_table_bytes=1 << 30, grammar_weight=1.0):
        super().__init__(alphabet, beam, nbest)
        if lm is not None and lm.logp.shape[1] != len(alphabet):
            raise ValueError("GrammarBeamDecoder: the LM was resolved for %d symbols, the alphabet has %d"
                             % (lm.logp.shape[1], len(alphabet)))
        self.grammars = [grammars] if isinstance(grammars, Grammar) else list(grammars)
        if not self.grammars:
            raise ValueError("GrammarBeamDecoder: no grammar")
        for g in self.grammars:
            if len(g.alphabet) != len(alphabet):
                raise ValueError("GrammarBeamDecoder: %s is over an alphabet of %d symbols, the decoder's has %d"
                                 % (g.name, len(g.alphabet), len(alphabet)))
        self.lm, self.lm_weight, self.insertion_bonus, self.prune_logp = lm, float(lm_weight), float(insertion_bonus), prune_logp
        self.max_table_bytes = int(max_table_bytes)
        self.grammar_weight = float(grammar_weight)
        if not np.isfinite(self.grammar_weight):
            raise ValueError("GrammarBeamDecoder: grammar_weight must be finite")
        self._packed = {}

    def decode_nbest(self, model_output, batch_actual_timesteps, nbest=None, which=None, grammar_scores=False):
        """_SearchDecoder.decode_nbest; with grammar_scores every hypothesis's scores are (total, acoustic, lm, grammar): the raw weight
        of its labelling under the line's grammar (0 for an unweighted one), which total holds grammar_weight times."""
        nbest = self.nbest if nbest is None else int(nbest)
        return _nbest_lists(*self._search(model_output, batch_actual_timesteps, nbest, which=which, grammar_scores=grammar_scores))

    def _search_device(self, model_output, batch_actual_timesteps, nbest, which=None, grammar_scores=False):
        dev = model_output.device
        canon, new = self._canon_on(dev)
        if new:
            self._packed[str(dev)] = pack_dense_grammars(self.grammars, dev, self.max_table_bytes)
        if which is not None:
            which = [int(k) for k in (which.tolist() if torch.is_tensor(which) else which)]
            if len(which) != int(model_output.shape[1]):
                raise ValueError("GrammarBeamDecoder: %d entries of which for %d lines" % (len(which), int(model_output.shape[1])))
            if min(which) < 0 or max(which) >= len(self.grammars):
                raise ValueError("GrammarBeamDecoder: which must index the %d grammars" % len(self.grammars))
        out = ops.ctc_grammar_beam_search(model_output.detach(), _line_lengths(batch_actual_timesteps), self._packed[str(dev)], which,
                                          canon, self.beam, nbest, self.lm.to(dev) if self.lm is not None else None,
                                          self.lm_weight, self.insertion_bonus, self.prune_logp, self.grammar_weight, grammar_scores)
        if not grammar_scores:
            return out
        return out[0], out[1], torch.cat([out[2], out[3].unsqueeze(-1)], dim=-1)      # the grammar's share as a fourth score


def _line_lengths(batch_actual_timesteps):
    lens = batch_actual_timesteps
    if torch.is_tensor(lens):
        lens = lens.detach().cpu()
    return [int(v) for v in lens]


def _aligned(model_output, lens, labels, lengths, scores, canon, alphabet, uxxxx, nbest):
    """decode_aligned's common end: align the device labellings [B,n,T] / [B,n] (scores [B,n,3] or None: every rank is a hypothesis),
    copy everything to the host once, format."""
    a_scores, spans, lsc = ops.ctc_align(model_output.detach(), lens, labels, lengths, canon)
    if scores is None:
        scores = torch.zeros(labels.shape[0], labels.shape[1], 3, dtype=torch.float32, device=labels.device)
    labels, lengths, scores, a_scores, spans, lsc = one_copy([labels, lengths, scores, a_scores, spans, lsc])
    rows = lines_from_arrays(labels, lengths, a_scores, spans, lsc, alphabet)
    hyps = _best_strings(labels, lengths, scores, alphabet, uxxxx)
    if nbest == 1:
        return hyps, [row[0] if np.isfinite(scores[b, 0, 0]) else None for b, row in enumerate(rows)]
    lists = _nbest_lists(labels, lengths, scores)
    return hyps, [[(h[0], h[1], row[q]) for q, h in enumerate(lst)] for lst, row in zip(lists, rows)]


def _alternatives(model_output, lens, labels, lengths, scores, canon, alphabet, uxxxx, topk):
    """decode_alternatives' common end for the device labellings [B,1,T] / [B,1] (scores [B,1,3] or None: every line has a hypothesis)."""
    if scores is None:
        scores = torch.zeros(labels.shape[0], 1, 3, dtype=torch.float32, device=labels.device)
    rows, (labels, lengths, scores) = alternatives_from_device(model_output, lens, labels, lengths, canon, alphabet, topk, extra=[scores])
    hyps = _best_strings(labels, lengths, scores, alphabet, uxxxx)
    return hyps, [row[0] if np.isfinite(scores[b, 0, 0]) else None for b, row in enumerate(rows)]


def _nbest_lists(labels, lengths, scores):
    """The beam searches' outputs (host arrays [B,nbest,T], [B,nbest], [B,nbest,3]) as per-line lists of (labels, scores), best
    first, up to the first rank the search did not fill (total -inf)."""
    out = []
    for b in range(labels.shape[0]):
        hyps = []
        for q in range(labels.shape[1]):
            if not np.isfinite(scores[b, q, 0]):
                break
            hyps.append(([int(v) for v in labels[b, q, :lengths[b, q]]], tuple(float(s) for s in scores[b, q])))
        out.append(hyps)
    return out


def _best_strings(labels, lengths, scores, alphabet, uxxxx):
    """Rank 0 of every line as space-joined uxxxx tokens (an unfilled rank: ""), converted to utf8 unless uxxxx."""
    idx_to_char = alphabet.idx_to_char
    result = []
    for b in range(labels.shape[0]):
        n = int(lengths[b, 0]) if np.isfinite(scores[b, 0, 0]) else 0
        result.append(" ".join(idx_to_char[int(k)] for k in labels[b, 0, :n]))
    if uxxxx == False:  # noqa: E712  (decode_greedy's comparison)
        result = [uxxxx_to_utf8(r) for r in result]
    return result


class WordBeamDecoder(_SearchDecoder):
    """CTC prefix beam search on the GPU scored by a word n-gram with a lexicon (vocr_ctc_word_beam_search, WordNgramLM): the stand-in
    for the reference's TLG.fst decode (decode_with_lm, src/decoder.py:11-109).  Hypotheses are ranked by ln P_ctc(y | x) +
    lm_weight * ln P_lm(tokens of y, </s>) + word_bonus * |tokens of y|, the tokens those of form_tokenized_words.  Letter-words are
    limited to the LM's lexicon; with `oov_penalty` (a ln penalty, None: closed vocabulary) any other word is scored as <unk> plus the
    penalty.  Output formats as BeamDecoder's."""

    def __init__(self, alphabet, lm, beam=16, nbest=1, lm_weight=0.8, word_bonus=0.0, oov_penalty=None):
        super().__init__(alphabet, beam, nbest)
        if lm.trie_next.shape[1] != len(alphabet):
            raise ValueError("WordBeamDecoder: the LM was resolved for %d symbols, the alphabet has %d" % (lm.trie_next.shape[1], len(alphabet)))
        self.lm = lm
        self.lm_weight, self.word_bonus = float(lm_weight), float(word_bonus)
        self.oov_penalty = None if oov_penalty is None else float(oov_penalty)

    def _search_device(self, model_output, batch_actual_timesteps, nbest):
        dev = model_output.device
        return ops.ctc_word_beam_search(model_output.detach(), _line_lengths(batch_actual_timesteps), self._canon_on(dev)[0],
                                        self.lm.to(dev), self.beam, nbest, self.lm_weight, self.word_bonus, self.oov_penalty)
