"""Grammar-constrained CTC training (graph-based temporal classification: GTC, Moritz et al. 2021; STC, Pratap et al. 2022; W-CTC, Cai
et al. 2022).  CTCLoss trains against exactly one transcript per line; this criterion trains against a SET of acceptable transcripts,
a regular language per line:

    loss = sum_b -ln P_b,      P_b = the probability under the CTC model that line b's text is accepted by the line's automaton

the exact sum over all frame paths through the product of the CTC topology with the automaton (vocr_ctc_grammar_grad,
csrc/ctc_grammar.hip: score and gradient in one call).  A partial transcript ("known words", anything, "known words"), alternatives at a
position, an unknown single character, or no transcript at all ("this field is a date") become targets.  The chain automaton of one
labelling gives CTCLoss's value.

A WEIGHTED grammar from `to_grammar` (Grammar.from_dfa(arc_weights=, final_weights=), from_words(log_weights=): "probably O, possibly
0") makes P_b the weighted sum Z_b (vocr_ctc_grammar_grad_weighted); the weights themselves get no gradient.

WHAT IT IS NOT: the automata are built on the host in Python (`to_grammar`, once per distinct target,
kept in a bounded LRU cache) and their tables copied to the device with every batch; an automaton has at most 8192 states + arcs; the
kernel stores frames x (largest states + largest arcs of the batch) x 4 bytes of forward rows per line (a batch beyond 2 GiB is cut
into chunks); and no claim about accuracy is made here."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import call
from .grammar import Grammar, grammar_grad_chunked
from .textutils import utf8_to_uxxxx


def pack_batch(grammars, which, act_lens, device):
    """pack_grammars' tables plus `which` and the lines' frame counts in ONE host-to-device copy: (packed dict, which_dev, lens_dev).
    The weight tables of a batch with a weighted grammar travel in the same copy, as the bits of their floats."""
    s_off = np.cumsum([0] + [g.n_states for g in grammars]).astype(np.int32)
    a_off = np.cumsum([0] + [g.n_arcs for g in grammars]).astype(np.int32)
    parts = [s_off, a_off] + [np.concatenate([getattr(g, n) for g in grammars]).astype(np.int32) for n in ("arc_src", "arc_cls", "arc_dst", "accept")]
    parts += [np.asarray(which, dtype=np.int32), np.asarray(act_lens, dtype=np.int32)]
    weighted = any(g.weighted for g in grammars)
    if weighted:                                                    # (one word of padding: the arc table is never empty)
        aw = [g.arc_logw if g.weighted else np.zeros(g.n_arcs, dtype=np.float32) for g in grammars] + [np.zeros(1, dtype=np.float32)]
        fw = [g.final_logw if g.weighted else np.zeros(g.n_states, dtype=np.float32) for g in grammars]
        parts += [np.concatenate(aw).astype(np.float32).view(np.int32), np.concatenate(fw).astype(np.float32).view(np.int32)]
    host = torch.from_numpy(np.concatenate(parts))
    if device.type == "cuda":
        host = host.pin_memory()
    dev = host.to(device, non_blocking=True)
    views, at = [], 0
    for p in parts:
        views.append(dev[at:at + p.size])
        at += p.size
    packed = {"state_off": views[0], "arc_off": views[1], "src": views[2], "cls": views[3], "dst": views[4], "accept": views[5],
              "max_states": max(g.n_states for g in grammars), "max_arcs": max(g.n_arcs for g in grammars)}
    if weighted:
        packed["arc_logw"], packed["final_logw"] = views[8].view(torch.float32), views[9].view(torch.float32)
    return packed, views[6], views[7]


class _GrammarCtcFn(torch.autograd.Function):
    """sum_b -ln P_b; the gradient with respect to the logits is saved by the forward call and scaled in the backward."""

    @staticmethod
    def forward(ctx, logits, lens_dev, packed, which_dev, canon, max_lattice_bytes, keep):
        logp, dlogits = grammar_grad_chunked(logits, lens_dev, packed, which_dev, canon, -1.0, max_lattice_bytes)
        keep.last_logp = logp
        ctx.save_for_backward(dlogits)
        return ops.colsum((-logp).reshape(-1, 1))                  # shape (1,): fixed order; +inf for a line with no accepted path

    @staticmethod
    def backward(ctx, dloss):
        (dlogits,) = ctx.saved_tensors
        dloss = ops._f32c(dloss)
        out = torch.empty_like(dlogits)
        call("vocr_scale_dev", ops._p(dlogits), ops._p(dloss), ops._p(out), dlogits.numel(), ops._stream())
        return (out,) + (None,) * 6


class GrammarCTCLoss(nn.Module):
    """criterion(logits [T,B,V] on the GPU, targets IntTensor [sum L] (CPU), act_lens IntTensor [B] (CPU), target_lens IntTensor [B]
    (CPU)) -> Tensor (1,) = sum over the batch of -ln P(the line's text is accepted by to_grammar(the line's target)), supporting
    .backward(): CTCLoss's signature and contract, so it goes wherever CTCLoss goes (train, train_async, loop.fit).  A line with no
    accepted path gives +inf, as with CTCLoss (its gradient rows are zeros).

    `to_grammar(labels: tuple of int) -> Grammar` is called once per distinct target and its result kept in an LRU cache of
    `cache_size` grammars (default 4096); equal targets of a batch share one automaton.  Symbol classes are the alphabet's, as with
    GrammarMatcher.  `last_logp`: fp32 [B] device tensor of ln P_b of the last call, for logging.  `max_lattice_bytes`: see
    GrammarMatcher.line_log_prob."""

    def __init__(self, alphabet, to_grammar, cache_size=4096, max_lattice_bytes=None):
        super().__init__()
        if not callable(to_grammar):
            raise TypeError("GrammarCTCLoss: to_grammar must be callable (labels: tuple of int) -> Grammar")
        if int(cache_size) < 1:
            raise ValueError("GrammarCTCLoss: need cache_size >= 1 (cache_size=%r)" % (cache_size,))
        self.alphabet, self.to_grammar = alphabet, to_grammar
        self.cache_size, self.max_lattice_bytes = int(cache_size), max_lattice_bytes
        self._cache = OrderedDict()
        self._canon = {}
        self.cache_hits = self.cache_misses = 0
        self.last_logp = None

    @classmethod
    def exact(cls, alphabet, **kw):
        """The chain of the target's labels: CTCLoss's value, through the grammar kernel."""
        return cls(alphabet, lambda labels: Grammar.from_labels(alphabet, labels), **kw)

    @classmethod
    def with_gaps(cls, alphabet, gap, any_char=None, **kw):
        """Targets with holes: the label `gap` (an alphabet index or one utf-8 character that the user reserves; it then appears on no
        arc) stands for Grammar.GAP, any string; `any_char`, if given, likewise for Grammar.ANY, exactly one symbol."""
        def index(v, what):
            if isinstance(v, str):
                k = alphabet.char_to_idx.get(utf8_to_uxxxx(v, output_array=True)[0]) if len(v) == 1 else None
            else:
                k = int(v) if 0 < int(v) < len(alphabet) else None
            if k is None:
                raise ValueError("GrammarCTCLoss.with_gaps: %s=%r is not a non-blank symbol of the alphabet" % (what, v))
            return k

        gi = index(gap, "gap")
        ai = None if any_char is None else index(any_char, "any_char")
        if ai == gi:
            raise ValueError("GrammarCTCLoss.with_gaps: gap and any_char must differ")
        reserved = [gi] if ai is None else [gi, ai]

        def to_grammar(labels):
            items = [Grammar.GAP if v == gi else Grammar.ANY if v == ai else v for v in labels]
            return Grammar.from_template(alphabet, items, exclude=reserved)

        return cls(alphabet, to_grammar, **kw)

    def canon(self, dev):
        key = str(dev)
        if key not in self._canon:
            self._canon[key] = torch.as_tensor(self.alphabet.canonical_indices(), dtype=torch.int32).to(dev)
        return self._canon[key]

    def grammar_for(self, labels):
        """The cached Grammar of one target (a tuple of int)."""
        g = self._cache.get(labels)
        if g is not None:
            self._cache.move_to_end(labels)
            self.cache_hits += 1
            return g
        self.cache_misses += 1
        g = self.to_grammar(labels)
        if not isinstance(g, Grammar):
            raise TypeError("GrammarCTCLoss: to_grammar%r returned %s, not a Grammar" % (labels, type(g).__name__))
        if g.n_states + g.n_arcs > ops.GRAMMAR_CELLS_MAX:
            raise ValueError("GrammarCTCLoss: the grammar of target %r has %d states + %d arcs, more than the kernel's %d cells"
                             % (labels, g.n_states, g.n_arcs, ops.GRAMMAR_CELLS_MAX))
        self._cache[labels] = g
        if len(self._cache) > self.cache_size:
            self._cache.popitem(last=False)
        return g

    def batch_grammars(self, labels, label_lens):
        """(the distinct grammars of a batch in order of first appearance, which[b])."""
        grammars, index, which, at = [], {}, [], 0
        for n in label_lens:
            key = tuple(labels[at:at + n])
            at += n
            if key not in index:
                index[key] = len(grammars)
                grammars.append(self.grammar_for(key))
            which.append(index[key])
        return grammars, which

    def forward(self, acts, labels, act_lens, label_lens):
        if not acts.is_cuda:
            raise RuntimeError("vistaocr_amd.GrammarCTCLoss needs activations on the MI355X; there is no CPU fallback")
        T, B = int(acts.shape[0]), int(acts.shape[1])
        labels = torch.as_tensor(labels).to(torch.int32).reshape(-1).cpu()
        label_lens_c = torch.as_tensor(label_lens).to(torch.int32).reshape(-1).cpu()
        act_lens_c = torch.as_tensor(act_lens).to(torch.int32).reshape(-1).cpu()
        if label_lens_c.numel() != B or act_lens_c.numel() != B:
            raise RuntimeError("GrammarCTCLoss: act_lens / label_lens must have one entry per batch element")
        if int(label_lens_c.sum()) != labels.numel() or int(label_lens_c.min()) < 0:
            raise RuntimeError("GrammarCTCLoss: sum(label_lens) != len(labels)")
        if int(act_lens_c.max()) > T:
            raise RuntimeError("GrammarCTCLoss: act_lens exceeds the time dimension")
        grammars, which = self.batch_grammars(labels.tolist(), label_lens_c.tolist())
        ms, ma = max(g.n_states for g in grammars), max(g.n_arcs for g in grammars)
        if ms + ma > ops.GRAMMAR_CELLS_MAX:
            raise ValueError("GrammarCTCLoss: the batch's largest state count %d plus its largest arc count %d exceed the kernel's %d cells"
                             % (ms, ma, ops.GRAMMAR_CELLS_MAX))
        packed, which_dev, lens_dev = pack_batch(grammars, which, act_lens_c.numpy(), acts.device)
        return _GrammarCtcFn.apply(acts, lens_dev, packed, which_dev, self.canon(acts.device), self.max_lattice_bytes, self)
