"""CTC grammar search on the GPU (vocr_ctc_grammar_scores): what is the probability that this line's text belongs to a given regular
language - a date, an amount, one of these 500 part numbers, "contains the word X" - and what is the best reading that does, asked of
the network's output itself.

WHAT THE NUMBER IS: for a line and a grammar (a deterministic finite automaton over the alphabet's symbol classes), the probability
under the CTC model that the line's collapsed labelling is accepted: the exact sum over ALL frame paths, no beam, no hypothesis, no
pruning.  WEIGHTED GRAMMARS (from_words(log_weights=), boost, from_ngram, from_dfa(arc_weights=, final_weights=)) carry a natural-log
weight on every arc and every accepting state; the number is then ln Z = ln of the sum of P(path) * exp(weight of the labelling), a
probability only when the weights normalise.  WHAT IT IS NOT: the "best" result is
the best single PATH through the grammar (frame path and state sequence), not the most probable accepted LABELLING (which would sum the
paths of each labelling first: decoder.GrammarBeamDecoder searches for that, over the dense tables of Grammar.dense_tables /
pack_dense_grammars).  Characters are compared as the alphabet's symbol strings: indices with the same string are one class
and share an arc.  An automaton of more than 8192 states + arcs does not fit the sweep kernels; larger lexicons stay with
WordBeamDecoder or go to GrammarBeamDecoder, whose tables have no such limit.
The gradient of a line's ln P under ITS OWN grammar (vocr_ctc_grammar_grad) is GrammarMatcher.line_log_prob; the training criterion
built on it is grammar_loss.GrammarCTCLoss."""
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .align import one_copy
from .textutils import utf8_to_uxxxx, uxxxx_to_utf8

GrammarHits = namedtuple("GrammarHits", "logp prob best_logp best_labels best_text")


def _classes(alphabet):
    """(canon list, sorted list of the non-blank classes)."""
    canon = alphabet.canonical_indices()
    return canon, sorted({c for c in canon[1:] if c != 0})


def _class_of_char(alphabet, canon, ch, where):
    tok = utf8_to_uxxxx(ch, output_array=True)[0]
    k = alphabet.char_to_idx.get(tok)
    if k is None or canon[k] == 0:
        raise ValueError("%s: the symbol %r (%s) is not in the alphabet" % (where, ch, tok))
    return canon[k]


def _labels(alphabet, canon, text, where):
    """A string (utf-8) or a sequence of alphabet indices as a list of classes."""
    if isinstance(text, str):
        return [_class_of_char(alphabet, canon, ch, where) for ch in text]
    out = []
    for v in text:
        v = int(v)
        if v <= 0 or v >= len(canon) or canon[v] == 0:
            raise ValueError("%s: %d is not a non-blank alphabet index" % (where, v))
        out.append(canon[v])
    return out


# ---- the regular-expression parser: pattern -> tree.  Nodes: ("set", frozenset of classes), ("cat", [nodes]), ("alt", [nodes]),
# ("rep", node, lo, hi or None)
class _Parser(object):
    def __init__(self, alphabet, pattern):
        self.alphabet, self.p, self.i = alphabet, pattern, 0
        self.canon, self.all = _classes(alphabet)
        self.where = "regex %r" % pattern

    def fail(self, what):
        raise ValueError("%s: %s at position %d" % (self.where, what, self.i))

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def cls(self, ch):
        return _class_of_char(self.alphabet, self.canon, ch, self.where)

    def digits(self):
        d = [self.alphabet.char_to_idx.get("u%04x" % (0x30 + k)) for k in range(10)]
        d = frozenset(self.canon[k] for k in d if k is not None)
        if not d:
            self.fail("\\d: the alphabet has no digits")
        return d

    def parse(self):
        node = self.alt()
        if self.i != len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        parts = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            parts.append(self.cat())
        return parts[0] if len(parts) == 1 else ("alt", parts)

    def cat(self):
        parts = []
        while self.peek() is not None and self.peek() not in "|)":
            parts.append(self.repeat())
        return ("cat", parts)

    def number(self):
        j = self.i
        while self.peek() is not None and self.peek().isdigit():
            self.i += 1
        if j == self.i:
            self.fail("a number is expected in {m,n}")
        return int(self.p[j:self.i])

    def repeat(self):
        node = self.atom()
        while self.peek() is not None and self.peek() in "*+?{":
            ch = self.peek()
            self.i += 1
            if ch == "*":
                node = ("rep", node, 0, None)
            elif ch == "+":
                node = ("rep", node, 1, None)
            elif ch == "?":
                node = ("rep", node, 0, 1)
            else:
                lo = hi = self.number()
                if self.peek() == ",":
                    self.i += 1
                    hi = None if self.peek() == "}" else self.number()
                if self.peek() != "}":
                    self.fail("'}' is expected")
                self.i += 1
                if hi is not None and hi < lo:
                    self.fail("{m,n} with n < m")
                node = ("rep", node, lo, hi)
        return node

    def escape(self):
        """The character after a backslash: a set."""
        ch = self.peek()
        if ch is None:
            self.fail("a pattern cannot end in a backslash")
        self.i += 1
        if ch == "d":
            return self.digits()
        if ch.isalnum():
            self.fail("unsupported escape \\%s" % ch)
        return frozenset([self.cls(ch)])

    def atom(self):
        ch = self.peek()
        if ch == "(":
            self.i += 1
            node = self.alt()
            if self.peek() != ")":
                self.fail("')' is expected")
            self.i += 1
            return node
        if ch == "[":
            self.i += 1
            return ("set", self.bracket())
        if ch in "*+?{":
            self.fail("nothing to repeat")
        self.i += 1
        if ch == ".":
            return ("set", frozenset(self.all))
        if ch == "\\":
            return ("set", self.escape())
        if ch in "]}":
            self.fail("unbalanced %r" % ch)
        return ("set", frozenset([self.cls(ch)]))

    def bracket(self):
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        members, first = set(), True
        while True:
            ch = self.peek()
            if ch is None:
                self.fail("']' is expected")
            if ch == "]" and not first:
                self.i += 1
                break
            first = False
            self.i += 1
            if ch == "\\":
                s = self.escape()
                members |= s
                continue
            if self.peek() == "-" and self.i + 1 < len(self.p) and self.p[self.i + 1] != "]":
                self.i += 1
                hi = self.peek()
                self.i += 1
                if hi == "\\":
                    hi = self.peek()
                    self.i += 1
                if ord(hi) < ord(ch):
                    self.fail("bad range %s-%s" % (ch, hi))
                self.cls(ch), self.cls(hi)                              # the ends must be symbols of the alphabet
                for code in range(ord(ch), ord(hi) + 1):
                    k = self.alphabet.char_to_idx.get(utf8_to_uxxxx(chr(code), output_array=True)[0])
                    if k is not None and self.canon[k] != 0:
                        members.add(self.canon[k])
            else:
                members.add(self.cls(ch))
        return frozenset(self.all) - members if negate else frozenset(members)


# ---- Thompson construction: tree -> NFA with epsilon moves
class _Nfa(object):
    def __init__(self):
        self.eps, self.arcs = [], []                       # per state: epsilon targets; (set of classes, target)

    def state(self):
        self.eps.append([])
        self.arcs.append([])
        return len(self.eps) - 1

    def build(self, node):
        """(start, end) of a fresh fragment."""
        kind = node[0]
        if kind == "set":
            a, b = self.state(), self.state()
            if node[1]:
                self.arcs[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = self.state()
            for part in node[1]:
                c, d = self.build(part)
                self.eps[b].append(c)
                b = d
            return a, b
        if kind == "alt":
            a, b = self.state(), self.state()
            for part in node[1]:
                c, d = self.build(part)
                self.eps[a].append(c)
                self.eps[d].append(b)
            return a, b
        _, inner, lo, hi = node
        a = b = self.state()
        for _ in range(lo):
            c, d = self.build(inner)
            self.eps[b].append(c)
            b = d
        if hi is None:                                     # inner*
            c, d = self.build(inner)
            e = self.state()
            self.eps[b] += [c, e]
            self.eps[d] += [c, e]
            b = e
        else:
            e = self.state()
            for _ in range(hi - lo):                       # (inner (inner ...)?)?
                c, d = self.build(inner)
                self.eps[b] += [c, e]
                b = d
            self.eps[b].append(e)
            b = e
        return a, b


def _determinize(nfa, start, end, max_cells=None, what=None):
    """Subset construction.  (per state a dict class -> state, accept flags); state 0 is the start.  max_cells: a ValueError under
    the name `what` once the states + arcs made so far exceed it (before minimisation)."""
    closures = {}

    def closure(states):
        out = set()
        for s in states:
            if s not in closures:
                seen, stack = {s}, [s]
                while stack:
                    for n in nfa.eps[stack.pop()]:
                        if n not in seen:
                            seen.add(n)
                            stack.append(n)
                closures[s] = frozenset(seen)
            out |= closures[s]
        return frozenset(out)

    first = closure([start])
    index, order, trans = {first: 0}, [first], []
    k = arcs = 0
    while k < len(order):
        if max_cells is not None and len(order) + arcs > max_cells:
            raise ValueError("%s: the subset construction has passed %d states + %d arcs, more than %d: too large to build (the kernel "
                             "takes %d cells)" % (what, len(order), arcs, max_cells, ops.GRAMMAR_CELLS_MAX))
        moves = {}
        for n in order[k]:
            for cset, tgt in nfa.arcs[n]:
                for c in cset:
                    moves.setdefault(c, set()).add(tgt)
        row = {}
        for c in sorted(moves):
            nxt = closure(moves[c])
            if nxt not in index:
                index[nxt] = len(order)
                order.append(nxt)
            row[c] = index[nxt]
        trans.append(row)
        arcs += len(row)
        k += 1
    return trans, [end in s for s in order]


def _minimize(trans, accept):
    """Trim (keep the states on a way from the start to an accepting state) and merge equivalent states.  State 0 stays the start;
    states are numbered breadth first, classes ascending, so that equal languages give equal tables."""
    n = len(trans)
    reach, stack = {0}, [0]
    while stack:
        for d in trans[stack.pop()].values():
            if d not in reach:
                reach.add(d)
                stack.append(d)
    back = [[] for _ in range(n)]
    for s in reach:
        for d in trans[s].values():
            back[d].append(s)
    live = {s for s in reach if accept[s]}
    stack = list(live)
    while stack:
        for s in back[stack.pop()]:
            if s not in live:
                live.add(s)
                stack.append(s)
    if 0 not in live:                                      # the empty language: the start state alone
        return [{}], [False]
    keep = sorted(live)
    block = {s: int(bool(accept[s])) for s in keep}
    count = len(set(block.values()))
    while True:
        sig = {s: (block[s], tuple(sorted((c, block[d]) for c, d in trans[s].items() if d in live))) for s in keep}
        ids = {}
        for s in keep:
            ids.setdefault(sig[s], len(ids))
        block = {s: ids[sig[s]] for s in keep}
        if len(ids) == count:
            break
        count = len(ids)
    rep = {}
    for s in keep:
        rep.setdefault(block[s], s)
    number, order = {block[0]: 0}, [block[0]]
    k = 0
    while k < len(order):
        s = rep[order[k]]
        for c in sorted(trans[s]):
            d = trans[s][c]
            if d in live and block[d] not in number:
                number[block[d]] = len(order)
                order.append(block[d])
        k += 1
    out_t, out_a = [], []
    for blk in order:
        s = rep[blk]
        out_t.append({c: number[block[d]] for c, d in trans[s].items() if d in live})
        out_a.append(bool(accept[s]))
    return out_t, out_a


def _minimize_weighted(trans, accept, tw, fw):
    """_minimize for an automaton with weights: tw[s][c] the weight of the arc of s on class c, fw[s] the final weight of an accepting
    state.  Trim, then partition refinement with the final weight in the initial partition and (class -> block, weight) in the
    signature: states are merged only when they agree on every weight, so the language and the weight of every labelling are kept.
    Correct, not claimed minimal: the weights are not pushed.  Returns (trans, accept, tw, fw)."""
    n = len(trans)
    reach, stack = {0}, [0]
    while stack:
        for d in trans[stack.pop()].values():
            if d not in reach:
                reach.add(d)
                stack.append(d)
    back = [[] for _ in range(n)]
    for s in reach:
        for d in trans[s].values():
            back[d].append(s)
    live = {s for s in reach if accept[s]}
    stack = list(live)
    while stack:
        for s in back[stack.pop()]:
            if s not in live:
                live.add(s)
                stack.append(s)
    if 0 not in live:
        return [{}], [False], [{}], [0.0]
    keep = sorted(live)
    first = {}
    block = {s: first.setdefault((bool(accept[s]), float(fw[s]) if accept[s] else 0.0), len(first)) for s in keep}
    count = len(first)
    while True:
        sig = {s: (block[s], tuple(sorted((c, block[d], float(tw[s][c])) for c, d in trans[s].items() if d in live))) for s in keep}
        ids = {}
        for s in keep:
            ids.setdefault(sig[s], len(ids))
        block = {s: ids[sig[s]] for s in keep}
        if len(ids) == count:
            break
        count = len(ids)
    rep = {}
    for s in keep:
        rep.setdefault(block[s], s)
    number, order = {block[0]: 0}, [block[0]]
    k = 0
    while k < len(order):
        s = rep[order[k]]
        for c in sorted(trans[s]):
            d = trans[s][c]
            if d in live and block[d] not in number:
                number[block[d]] = len(order)
                order.append(block[d])
        k += 1
    out_t, out_a, out_w, out_f = [], [], [], []
    for blk in order:
        s = rep[blk]
        out_t.append({c: number[block[d]] for c, d in trans[s].items() if d in live})
        out_w.append({c: float(tw[s][c]) for c, d in trans[s].items() if d in live})
        out_a.append(bool(accept[s]))
        out_f.append(float(fw[s]) if accept[s] else 0.0)
    return out_t, out_a, out_w, out_f


def _check_weights(where, trans, accept, tw, fw):
    """The rules of a weighted automaton's tables: one weight per arc, one final weight per state, every one of them finite."""
    if len(tw) != len(trans) or len(fw) != len(trans):
        raise ValueError("%s: need the arc weights of every state and one final weight per state (%d states, %d rows of arc weights, "
                         "%d final weights)" % (where, len(trans), len(tw), len(fw)))
    for s, row in enumerate(trans):
        if set(tw[s]) != set(row):
            raise ValueError("%s: state %d has arcs on the classes %s but weights on %s" % (where, s, sorted(row), sorted(tw[s])))
        for c in row:
            if not np.isfinite(float(tw[s][c])):
                raise ValueError("%s: the weight of state %d's arc on class %d is %r: weights must be finite" % (where, s, c, tw[s][c]))
        if accept[s] and not np.isfinite(float(fw[s])):
            raise ValueError("%s: the final weight of state %d is %r: weights must be finite" % (where, s, fw[s]))


def _check_trimmed(where, trans, accept):
    """What as_given promises: every state is reached from state 0 and reaches an accepting state."""
    n = len(trans)
    reach, stack = {0}, [0]
    back = [[] for _ in range(n)]
    for s, row in enumerate(trans):
        for d in row.values():
            back[d].append(s)
    while stack:
        for d in trans[stack.pop()].values():
            if d not in reach:
                reach.add(d)
                stack.append(d)
    live = {s for s in range(n) if accept[s]}
    stack = list(live)
    while stack:
        for s in back[stack.pop()]:
            if s not in live:
                live.add(s)
                stack.append(s)
    if len(reach) != n or len(live) != n:
        raise ValueError("%s: as_given needs trimmed tables, but %d of %d states are unreachable and %d cannot reach an accepting state"
                         % (where, n - len(reach), n, n - len(live)))


class _Marker(object):
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "Grammar." + self.name


class Grammar(object):
    """A minimised deterministic automaton over the alphabet's symbol classes: dead and unreachable states removed, state 0 the start,
    the arcs in the kernel's order (dst, class, src).  Build one with from_regex, from_words, contains, from_dfa, from_template or
    from_labels."""

    ANY = _Marker("ANY")                                    # from_template: exactly one arbitrary symbol
    GAP = _Marker("GAP")                                    # from_template: any string, the empty one included

    def __init__(self, alphabet, trans, accept, name="grammar", arc_w=None, final_w=None, as_given=False, dense_only=False):
        """arc_w (per state a dict class -> natural-log weight) and final_w (one per state, read for accepting states) make the grammar
        WEIGHTED; they go together.  as_given: the tables are already trimmed (checked: a ValueError otherwise) and are kept state for
        state, neither renumbered nor merged (from_ngram).  dense_only:
        no arc arrays are built, only dense_tables / dense_weights (an automaton beyond the sweep kernels' cells, for the beam)."""
        self.alphabet, self.name = alphabet, name
        self._canon = alphabet.canonical_indices()
        if (arc_w is None) != (final_w is None):
            raise ValueError("Grammar: arc weights and final weights go together")
        self.weighted = arc_w is not None
        if self.weighted:
            _check_weights(name, trans, accept, arc_w, final_w)
            if as_given:
                _check_trimmed(name, trans, accept)
                self._trans, acc = [dict(r) for r in trans], [bool(a) for a in accept]
                self._tw, fw = [dict(r) for r in arc_w], [float(f) if a else 0.0 for f, a in zip(final_w, accept)]
            else:
                self._trans, acc, self._tw, fw = _minimize_weighted(trans, accept, arc_w, final_w)
            self._fw = np.array(fw, dtype=np.float64)
        else:
            self._trans, acc = _minimize(trans, accept)
            self._tw, self._fw = None, None
        self.accept = np.array(acc, dtype=np.int32)
        self.dense_only = bool(dense_only)
        self._n_arcs = sum(len(row) for row in self._trans)
        self.arc_dst = self.arc_cls = self.arc_src = self.arc_logw = self.final_logw = None
        if self.dense_only:
            return
        arcs = sorted((d, c, s) for s, row in enumerate(self._trans) for c, d in row.items())
        self.arc_dst = np.array([a[0] for a in arcs], dtype=np.int32)
        self.arc_cls = np.array([a[1] for a in arcs], dtype=np.int32)
        self.arc_src = np.array([a[2] for a in arcs], dtype=np.int32)
        if self.weighted:                                   # the weights in the kernel's arc order, the final weights per state
            self.arc_logw = np.array([self._tw[a[2]][a[1]] for a in arcs], dtype=np.float32)
            self.final_logw = self._fw.astype(np.float32)

    n_states = property(lambda self: len(self._trans))
    n_arcs = property(lambda self: self._n_arcs)

    @property
    def max_in_degree(self):
        dst = [d for row in self._trans for d in row.values()]
        return int(np.bincount(dst, minlength=1).max()) if dst else 0

    def dfa(self):
        """(per state a dict class -> state, accept flags): the tables from_dfa takes."""
        return [dict(row) for row in self._trans], [bool(a) for a in self.accept]

    def accepts(self, labels):
        """Whether the automaton accepts a labelling: a utf-8 string or a sequence of alphabet indices."""
        try:
            seq = _labels(self.alphabet, self._canon, labels, "accepts")
        except ValueError:
            return False
        s = 0
        for c in seq:
            s = self._trans[s].get(c)
            if s is None:
                return False
        return bool(self.accept[s])

    def weight_of(self, labels):
        """The total weight of a labelling (a utf-8 string or a sequence of alphabet indices) - the sum of its arcs' weights and the
        final weight of the state it ends in, in float64 on the host - or None when the automaton rejects it.  0.0 for an accepted
        labelling of an unweighted grammar."""
        try:
            seq = _labels(self.alphabet, self._canon, labels, "weight_of")
        except ValueError:
            return None
        s, w = 0, 0.0
        for c in seq:
            n = self._trans[s].get(c)
            if n is None:
                return None
            if self.weighted:
                w += self._tw[s][c]
            s = n
        if not self.accept[s]:
            return None
        return w + float(self._fw[s]) if self.weighted else 0.0

    def dense_weights(self):
        """(logw float32 [S,V], final float32 [S]), the weight tables of the weighted grammar beam search in dense_tables' indexing:
        logw[s, c] the weight of the arc of s on class c (0 where there is none), final[s] the final weight (0 for a state that does
        not accept).  Zeros for an unweighted grammar."""
        S, V = self.n_states, len(self._canon)
        logw, fin = np.zeros((S, V), dtype=np.float32), np.zeros(S, dtype=np.float32)
        if self.weighted:
            for s, row in enumerate(self._tw):
                for c, w in row.items():
                    logw[s, c] = w
            fin[:] = self._fw
        return logw, fin

    def dense_tables(self):
        """(next int32 [S,V], dist int32 [S]), the tables of the grammar-constrained beam search (vocr_ctc_grammar_beam_search):
        next[s, c] the state after class c (-1: no arc; non-canonical columns are -1), dist[s] the fewest symbols from s to an
        accepting state (0 exactly for the accepting states; -1 where none can be reached: the start of the empty language)."""
        S, V = self.n_states, len(self._canon)
        nxt = np.full((S, V), -1, dtype=np.int32)
        back = [[] for _ in range(S)]
        for s, row in enumerate(self._trans):
            for c, d in row.items():
                nxt[s, c] = d
                back[d].append(s)
        dist = np.full(S, -1, dtype=np.int32)
        frontier = [s for s in range(S) if self.accept[s]]
        dist[frontier] = 0
        while frontier:
            following = []
            for d in frontier:
                for s in back[d]:
                    if dist[s] < 0:
                        dist[s] = dist[d] + 1
                        following.append(s)
            frontier = following
        return nxt, dist

    @classmethod
    def from_regex(cls, alphabet, pattern):
        """A WHOLE-LINE match of `pattern`: literals (utf-8; a symbol outside the alphabet is a ValueError), `.` (any symbol), `[abc]`,
        `[a-z]`, `[^...]`, `\\d`, `\\` escapes of punctuation, `( )`, `|`, `*`, `+`, `?`, `{m}`, `{m,n}`, `{m,}`.  Thompson NFA, subset
        construction, minimisation."""
        tree = _Parser(alphabet, pattern).parse()
        nfa = _Nfa()
        start, end = nfa.build(tree)
        trans, accept = _determinize(nfa, start, end)
        return cls(alphabet, trans, accept, name="regex %r" % pattern)

    @classmethod
    def from_words(cls, alphabet, words, log_weights=None):
        """Accepts exactly the given words (utf-8 strings or index sequences): a trie, minimised.  log_weights: one natural-log weight
        per word (a prior over the closed set; a word given twice keeps its larger weight).  The weights are pushed towards the root
        as a look-ahead, so that the beam search sees them early: with phi(node) = the largest word weight below the node, the arc
        root -> child carries phi(child), any other arc phi(child) - phi(parent), and a word's end state final = w - phi(node): the
        total of a word is its weight."""
        canon = alphabet.canonical_indices()
        words = list(words)
        if log_weights is not None:
            log_weights = [float(w) for w in log_weights]
            if len(log_weights) != len(words):
                raise ValueError("from_words: %d log_weights for %d words" % (len(log_weights), len(words)))
            if not np.isfinite(log_weights).all():
                raise ValueError("from_words: log_weights must be finite")
        trans, accept, parent, wword = [{}], [False], [-1], [None]
        for k, w in enumerate(words):
            s = 0
            for c in _labels(alphabet, canon, w, "from_words"):
                if c not in trans[s]:
                    trans[s][c] = len(trans)
                    trans.append({})
                    accept.append(False)
                    parent.append(s)
                    wword.append(None)
                s = trans[s][c]
            accept[s] = True
            if log_weights is not None:
                wword[s] = log_weights[k] if wword[s] is None else max(wword[s], log_weights[k])
        name = "a trie of %d words" % sum(accept)
        if log_weights is None:
            return cls(alphabet, trans, accept, name=name)
        phi = [float("-inf") if w is None else w for w in wword]
        for s in range(len(trans) - 1, 0, -1):              # a child has a larger number than its parent
            phi[parent[s]] = max(phi[parent[s]], phi[s])
        tw = [{c: (phi[d] if s == 0 else phi[d] - phi[s]) for c, d in row.items()} for s, row in enumerate(trans)]
        fw = [wword[s] - phi[s] if accept[s] else 0.0 for s in range(len(trans))]
        return cls(alphabet, trans, accept, name="a weighted " + name[2:], arc_w=tw, final_w=fw)

    @classmethod
    def boost(cls, alphabet, phrases, bonus):
        """Contextual biasing (hot words): accepts EVERY labelling, and the weight of a labelling is exactly the sum over the phrases
        of bonus_p * (the occurrences of p in it, overlapping ones included).  `bonus`: a float or one per phrase (natural-log units:
        what a hit adds to the beam search's rank, times grammar_weight).  The Aho-Corasick automaton of the phrases as a TOTAL
        deterministic automaton: every state accepts, so the beam search's distance is 0 everywhere and nothing is pruned.  The weights
        are shaped so that a partial match is rewarded and a broken one pays it back: with the potential psi(state) = the largest
        bonus_p * depth / |p| over the phrases p through the state's trie node, an arc carries psi(next) - psi(state) plus the bonuses of
        the phrases completed on arrival (those reached through suffix links too), and final = -psi(state).  One state per trie node
        times one arc per class: a table for GrammarBeamDecoder, usually far beyond the sweep kernels' 8192 cells."""
        canon, every = _classes(alphabet)
        phrases = [_labels(alphabet, canon, p, "boost") for p in phrases]
        if not phrases or any(not p for p in phrases):
            raise ValueError("boost: need at least one phrase and no empty one")
        bonus = [float(bonus)] * len(phrases) if np.isscalar(bonus) else [float(b) for b in bonus]
        if len(bonus) != len(phrases):
            raise ValueError("boost: %d bonuses for %d phrases" % (len(bonus), len(phrases)))
        if not np.isfinite(bonus).all():
            raise ValueError("boost: bonuses must be finite")
        goto, depth, psi, out = [{}], [0], [0.0], [0.0]     # the trie; out: the bonuses of the phrases that END at the node
        for p, b in zip(phrases, bonus):
            s = 0
            for k, c in enumerate(p):
                if c not in goto[s]:
                    goto[s][c] = len(goto)
                    goto.append({})
                    depth.append(k + 1)
                    psi.append(float("-inf"))
                    out.append(0.0)
                s = goto[s][c]
                psi[s] = max(psi[s], b * (k + 1) / len(p))
            out[s] += b
        n = len(goto)
        fail, order = [0] * n, []
        queue = list(goto[0].values())
        while queue:                                        # breadth first: a node's suffix link is known before its children's
            following = []
            for s in queue:
                order.append(s)
                for c, d in goto[s].items():
                    f = fail[s]
                    while f and c not in goto[f]:
                        f = fail[f]
                    fail[d] = goto[f][c] if c in goto[f] and goto[f][c] != d else 0
                    following.append(d)
            queue = following
        done = list(out)                                    # done[s]: the bonuses of every phrase that ends where s is reached
        for s in order:
            done[s] = out[s] + done[fail[s]]
        trans = [None] * n
        for s in [0] + order:                               # the total transition function, suffix links resolved
            row = {}
            for c in every:
                row[c] = goto[s][c] if c in goto[s] else (trans[fail[s]][c] if s else 0)
            trans[s] = row
        tw = [{c: psi[d] - psi[s] + done[d] for c, d in trans[s].items()} for s in range(n)]
        fw = [-psi[s] for s in range(n)]
        g = cls(alphabet, trans, [True] * n, name="a boost of %d phrases" % len(phrases), arc_w=tw, final_w=fw,
                dense_only=n + n * len(every) > ops.GRAMMAR_CELLS_MAX)
        return g

    @classmethod
    def from_ngram(cls, lm, scale=1.0, dense_only=False, alphabet=None):
        """A character n-gram (lm.CharNgramLM) as a weighted automaton: its states are the LM's histories that can be reached from the
        start, the arc of a state on class c carries scale * ln P(c | history) and leads to the LM's next state, every state accepts
        with final = scale * ln P(</s> | history).  ln Z under it is ln sum_l P(l | x) * P_LM(l)^scale over ALL labellings (the
        denominator of MMI / CTC-CRF training), and GrammarBeamDecoder with it and no LM is BeamDecoder with the LM.  The alphabet is
        the LM's (CharNgramLM.from_arpa keeps it) unless given.  An automaton beyond the sweep kernels' 8192 cells is a ValueError that
        names the sizes, unless dense_only: then only the beam search's tables are built."""
        alphabet = alphabet if alphabet is not None else getattr(lm, "alphabet", None)
        if alphabet is None:
            raise ValueError("from_ngram: the LM does not know its alphabet; pass alphabet=")
        canon, every = _classes(alphabet)
        if lm.logp.shape[1] != len(canon):
            raise ValueError("from_ngram: the LM was resolved for %d symbols, the alphabet has %d" % (lm.logp.shape[1], len(canon)))
        scale = float(scale)
        if not np.isfinite(scale):
            raise ValueError("from_ngram: scale must be finite")
        number, order = {int(lm.start): 0}, [int(lm.start)]
        k = 0
        while k < len(order):                               # the reachable histories, breadth first, the start as state 0
            for c in every:
                d = int(lm.next[order[k], c])
                if d not in number:
                    number[d] = len(order)
                    order.append(d)
            k += 1
        S, E = len(order), len(order) * len(every)
        if S + E > ops.GRAMMAR_CELLS_MAX and not dense_only:
            raise ValueError("from_ngram: %d LM states x %d classes give %d states + %d arcs, more than the kernel's %d cells "
                             "(dense_only=True builds the beam search's tables alone)" % (S, len(every), S, E, ops.GRAMMAR_CELLS_MAX))
        # float32 products, so that scale = 1 hands the beam search the LM's own table entries bit for bit
        lw = (np.float32(scale) * lm.logp.astype(np.float32)).astype(np.float64)
        le = (np.float32(scale) * lm.eos.astype(np.float32)).astype(np.float64)
        trans = [{c: number[int(lm.next[h, c])] for c in every} for h in order]
        tw = [{c: float(lw[h, c]) for c in every} for h in order]
        fw = [float(le[h]) for h in order]
        return cls(alphabet, trans, [True] * S, name="a %d-gram of %d states" % (lm.order, S), arc_w=tw, final_w=fw, as_given=True,
                   dense_only=dense_only)

    @classmethod
    def contains(cls, alphabet, keyword, whole_word=False):
        """Accepts every line in which `keyword` occurs as a contiguous run of characters (.*keyword.*); with whole_word only where it
        is bounded on both sides by a space (u0020) or by the line's ends."""
        canon, every = _classes(alphabet)
        lab = _labels(alphabet, canon, keyword, "contains")
        if not lab:
            raise ValueError("contains: empty keyword")
        any_star = ("rep", ("set", frozenset(every)), 0, None)
        word = [("set", frozenset([c])) for c in lab]
        if whole_word:
            sp = alphabet.char_to_idx.get("u0020")
            if sp is None:
                raise ValueError("contains(whole_word=True): the alphabet has no u0020 (space)")
            sp = ("set", frozenset([canon[sp]]))
            tree = ("cat", [("rep", ("cat", [any_star, sp]), 0, 1)] + word + [("rep", ("cat", [sp, any_star]), 0, 1)])
        else:
            tree = ("cat", [any_star] + word + [any_star])
        nfa = _Nfa()
        start, end = nfa.build(tree)
        trans, accept = _determinize(nfa, start, end)
        return cls(alphabet, trans, accept, name="contains %r%s" % (keyword, " (whole word)" if whole_word else ""))

    @classmethod
    def from_labels(cls, alphabet, labels):
        """Accepts exactly one labelling (a utf-8 string or a sequence of alphabet indices): the linear chain, whose score is the CTC
        score of the labelling."""
        lab = _labels(alphabet, alphabet.canonical_indices(), labels, "from_labels")
        trans = [{c: k + 1} for k, c in enumerate(lab)] + [{}]
        return cls(alphabet, trans, [False] * len(lab) + [True], name="a chain of %d labels" % len(lab))

    @classmethod
    def from_template(cls, alphabet, items, exclude=()):
        """A transcript with holes.  `items` is a sequence of: a symbol (an alphabet index or one utf-8 character); a set, frozenset,
        list or tuple of symbols (alternatives at one position); Grammar.ANY (exactly one arbitrary symbol); Grammar.GAP (any string,
        the empty one included).  `exclude`: symbols that ANY and GAP do not stand for (a reserved placeholder).  Thompson NFA, subset
        construction, minimisation, so the result is the minimal DFA and no labelling is counted twice.  A template whose DFA has
        more than the kernel's 8192 states + arcs is a ValueError that names its sizes."""
        canon, every = _classes(alphabet)

        def sym(v):
            return _labels(alphabet, canon, v if isinstance(v, str) else [v], "from_template")[0]

        every = frozenset(every) - frozenset(sym(v) for v in exclude)
        parts = []
        for it in items:
            if it is cls.ANY:
                parts.append(("set", every))
            elif it is cls.GAP:
                parts.append(("rep", ("set", every), 0, None))
            elif isinstance(it, (set, frozenset, list, tuple)):
                if not len(it):
                    raise ValueError("from_template: an empty set of alternatives")
                parts.append(("set", frozenset(sym(v) for v in it)))
            elif isinstance(it, str) and len(it) != 1:
                raise ValueError("from_template: %r is not one character (a set or list gives alternatives)" % (it,))
            else:
                parts.append(("set", frozenset([sym(it)])))
        nfa = _Nfa()
        start, end = nfa.build(("cat", parts))
        # a set of NFA states never holds more than the template's positions, but ANY behind a GAP can double the DFA per item
        trans, accept = _determinize(nfa, start, end, max_cells=ops.GRAMMAR_CELLS_MAX * 64, what="from_template")
        g = cls(alphabet, trans, accept, name="a template of %d items" % len(parts))
        if g.n_states + g.n_arcs > ops.GRAMMAR_CELLS_MAX:
            raise ValueError("from_template: the template's minimal DFA has %d states + %d arcs, more than the kernel's %d cells"
                             % (g.n_states, g.n_arcs, ops.GRAMMAR_CELLS_MAX))
        return g

    @classmethod
    def from_dfa(cls, alphabet, transitions, accept, arc_weights=None, final_weights=None):
        """Explicit tables: `transitions[s]` a dict symbol -> state (a symbol is an alphabet index or one utf-8 character), `accept[s]`
        flags, state 0 the start.  Two symbols of one class must lead to the same state.  `arc_weights[s]` a dict symbol -> natural-log
        weight with the keys of transitions[s] and `final_weights[s]` one float per state (read for accepting states) make the grammar
        weighted; they go together and must be finite, and two symbols of one class must carry the same weight."""
        canon = alphabet.canonical_indices()
        if len(transitions) != len(accept) or not len(accept):
            raise ValueError("from_dfa: need one accept flag per state and at least one state")
        if (arc_weights is None) != (final_weights is None):
            raise ValueError("from_dfa: arc_weights and final_weights go together")
        tw = None
        if arc_weights is not None:
            if len(arc_weights) != len(accept) or len(final_weights) != len(accept):
                raise ValueError("from_dfa: need the arc weights of every state and one final weight per state (%d states, %d rows of "
                                 "arc weights, %d final weights)" % (len(accept), len(arc_weights), len(final_weights)))
            tw = []
            for s, row in enumerate(arc_weights):
                if set(row) != set(transitions[s]):
                    raise ValueError("from_dfa: state %d has arcs on %s but weights on %s" % (s, sorted(transitions[s], key=str),
                                                                                             sorted(row, key=str)))
                out = {}
                for sym, w in row.items():
                    c = _labels(alphabet, canon, sym if isinstance(sym, str) else [sym], "from_dfa")[0]
                    if out.setdefault(c, float(w)) != float(w) and not (np.isnan(out[c]) and np.isnan(float(w))):
                        raise ValueError("from_dfa: state %d has two weights on class %d" % (s, c))
                tw.append(out)
        trans = []
        for s, row in enumerate(transitions):
            out = {}
            for sym, d in row.items():
                c = _labels(alphabet, canon, sym if isinstance(sym, str) else [sym], "from_dfa")[0]
                d = int(d)
                if d < 0 or d >= len(accept):
                    raise ValueError("from_dfa: state %d has an arc to %d, outside 0 .. %d" % (s, d, len(accept) - 1))
                if out.setdefault(c, d) != d:
                    raise ValueError("from_dfa: state %d is not deterministic on class %d" % (s, c))
            trans.append(out)
        if tw is None:
            return cls(alphabet, trans, list(accept), name="dfa of %d states" % len(accept))
        return cls(alphabet, trans, list(accept), name="weighted dfa of %d states" % len(accept), arc_w=tw,
                   final_w=[float(f) for f in final_weights])


def pack_grammars(grammars, device):
    """The concatenated tables ops.ctc_grammar_scores takes, on `device`.  "arc_logw" / "final_logw" (fp32, the arcs' and the states'
    order) are there only when some grammar of the pack is weighted; its unweighted members get zeros."""
    grammars = list(grammars)
    for g in grammars:
        if g.dense_only:
            raise ValueError("pack_grammars: %s was built with the beam search's dense tables alone (%d states + %d arcs)"
                             % (g.name, g.n_states, g.n_arcs))
    s_off = np.cumsum([0] + [g.n_states for g in grammars]).astype(np.int32)
    a_off = np.cumsum([0] + [g.n_arcs for g in grammars]).astype(np.int32)

    def cat(name):
        return torch.from_numpy(np.concatenate([getattr(g, name) for g in grammars]).astype(np.int32)).to(device)

    out = {"state_off": torch.from_numpy(s_off).to(device), "arc_off": torch.from_numpy(a_off).to(device), "src": cat("arc_src"),
           "cls": cat("arc_cls"), "dst": cat("arc_dst"), "accept": cat("accept"),
           "max_states": max(g.n_states for g in grammars), "max_arcs": max(g.n_arcs for g in grammars)}
    if any(g.weighted for g in grammars):
        aw = np.concatenate([g.arc_logw if g.weighted else np.zeros(g.n_arcs, dtype=np.float32) for g in grammars] +
                            [np.zeros(1, dtype=np.float32)])            # one word of padding: never an empty (NULL) table
        fw = np.concatenate([g.final_logw if g.weighted else np.zeros(g.n_states, dtype=np.float32) for g in grammars])
        out["arc_logw"] = torch.from_numpy(aw.astype(np.float32)).to(device)
        out["final_logw"] = torch.from_numpy(fw.astype(np.float32)).to(device)
    return out


def pack_dense_grammars(grammars, device, max_table_bytes=1 << 30):
    """The concatenated dense tables ops.ctc_grammar_beam_search takes, on `device`: state_off int32 [G+1], next int32 [states, V],
    dist int32 [states]; and, only when some grammar of the pack is weighted, logw fp32 [states, V] and final fp32 [states]
    (Grammar.dense_weights; zeros for its unweighted members).  The sweep kernels' 8192 cells do not bound them; their memory does:
    tables above max_table_bytes are a ValueError that names the sizes."""
    grammars = list(grammars)
    if not grammars:
        raise ValueError("pack_dense_grammars: no grammar")
    V = len(grammars[0]._canon)
    if any(len(g._canon) != V for g in grammars):
        raise ValueError("pack_dense_grammars: the grammars are over alphabets of different sizes (%s)"
                         % sorted({len(g._canon) for g in grammars}))
    states = sum(g.n_states for g in grammars)
    weighted = any(g.weighted for g in grammars)
    nbytes = states * (V + 1) * 4 * (2 if weighted else 1)
    if nbytes > max_table_bytes:
        raise ValueError("pack_dense_grammars: %d states x %d symbols of dense tables take %d bytes, more than max_table_bytes=%d"
                         % (states, V, nbytes, max_table_bytes))
    tabs = [g.dense_tables() for g in grammars]
    s_off = np.cumsum([0] + [g.n_states for g in grammars]).astype(np.int32)
    out = {"state_off": torch.from_numpy(s_off).to(device),
           "next": torch.from_numpy(np.ascontiguousarray(np.concatenate([t[0] for t in tabs], axis=0))).to(device),
           "dist": torch.from_numpy(np.ascontiguousarray(np.concatenate([t[1] for t in tabs]))).to(device),
           "num_grammars": len(grammars), "num_states": int(states)}
    if weighted:
        wt = [g.dense_weights() for g in grammars]
        out["logw"] = torch.from_numpy(np.ascontiguousarray(np.concatenate([t[0] for t in wt], axis=0))).to(device)
        out["final"] = torch.from_numpy(np.ascontiguousarray(np.concatenate([t[1] for t in wt]))).to(device)
    return out


def group_grammars(grammars, T, B, want_best):
    """`grammars` cut, in order, into the fewest consecutive groups that one vocr_ctc_grammar_scores call each can take: the largest state
    count plus the largest arc count of a group within the kernel's cells (the two maxima may come from different grammars), and with
    best paths T * B * group size * that sum * 4 bytes of back pointers within 2 GiB.  A grammar that does not fit a call of its own
    is a ValueError that names it and its sizes."""
    def fits(ms, ma, n):
        return ms + ma <= ops.GRAMMAR_CELLS_MAX and (not want_best or T * B * n * (ms + ma) * 4 <= ops.GRAMMAR_BP_MAX_BYTES)

    groups, ms, ma = [], 0, 0
    for g in grammars:
        if g.n_states + g.n_arcs > ops.GRAMMAR_CELLS_MAX:
            raise ValueError("GrammarMatcher: %s has %d states + %d arcs, more than the kernel's %d cells (larger lexicons: "
                             "WordBeamDecoder)" % (g.name, g.n_states, g.n_arcs, ops.GRAMMAR_CELLS_MAX))
        if not fits(g.n_states, g.n_arcs, 1):
            raise ValueError("GrammarMatcher: %s has %d states + %d arcs; its back pointers for %d frames x %d lines take %d bytes, more "
                             "than %d: use fewer lines per call, or scores without best paths"
                             % (g.name, g.n_states, g.n_arcs, T, B, T * B * (g.n_states + g.n_arcs) * 4, ops.GRAMMAR_BP_MAX_BYTES))
        if groups and fits(max(ms, g.n_states), max(ma, g.n_arcs), len(groups[-1]) + 1):
            groups[-1].append(g)
            ms, ma = max(ms, g.n_states), max(ma, g.n_arcs)
        else:
            groups.append([g])
            ms, ma = g.n_states, g.n_arcs
    return groups


def lattice_chunks(T, B, max_states, max_arcs, max_lattice_bytes=None):
    """The batch cut into the fewest consecutive ranges [b0, b1) of lines whose stored forward rows, T * lines * (max_states + max_arcs)
    * 4 bytes, stay within max_lattice_bytes (None: the kernel's 2 GiB) in one vocr_ctc_grammar_grad call each."""
    limit = ops.GRAMMAR_LATTICE_MAX_BYTES if max_lattice_bytes is None else min(int(max_lattice_bytes), ops.GRAMMAR_LATTICE_MAX_BYTES)
    one = ops.grammar_lattice_bytes(T, 1, max_states, max_arcs)
    per = limit // one
    if per < 1:
        raise ValueError("GrammarMatcher: one line's forward rows, %d frames x (%d states + %d arcs) x 4 = %d bytes, exceed the limit of "
                         "%d bytes" % (T, max_states, max_arcs, one, limit))
    return [(b0, min(b0 + per, B)) for b0 in range(0, B, per)]


def grammar_grad_chunked(logits, lens_dev, packed, which_dev, canon, weight, max_lattice_bytes=None):
    """(logp [B], dlogits [T,B,V]) of ops.ctc_grammar_grad with the constant weight `weight` per line, in as many calls as the stored
    rows need.  Every call gets the same packed tables, so a line's bits do not depend on where the batch is cut."""
    T, B = int(logits.shape[0]), int(logits.shape[1])
    chunks = lattice_chunks(T, B, packed["max_states"], packed["max_arcs"], max_lattice_bytes)
    w = torch.full((B,), float(weight), dtype=torch.float32, device=logits.device)
    if len(chunks) == 1:
        return ops.ctc_grammar_grad(logits, lens_dev, packed, which_dev, canon, w)
    outs = [ops.ctc_grammar_grad(logits[:, b0:b1], lens_dev[b0:b1], packed, which_dev[b0:b1], canon, w[b0:b1]) for b0, b1 in chunks]
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs], dim=1)


class _LineLogProbFn(torch.autograd.Function):
    """ln P [B]; the gradient with respect to the logits is saved by the forward call and scaled per line in the backward."""

    @staticmethod
    def forward(ctx, logits, lens_dev, packed, which_dev, canon, max_lattice_bytes):
        logp, dlogits = grammar_grad_chunked(logits, lens_dev, packed, which_dev, canon, 1.0, max_lattice_bytes)
        ctx.save_for_backward(dlogits)
        return logp

    @staticmethod
    def backward(ctx, dlogp):
        (dlogits,) = ctx.saved_tensors
        # a line with ln P = -inf has zero rows; its incoming gradient may be anything, inf included, and must not make them NaN
        scale = torch.nan_to_num(ops._f32c(dlogp), nan=0.0, posinf=0.0, neginf=0.0).reshape(1, -1, 1)
        return (dlogits * scale,) + (None,) * 5


class GrammarMatcher(object):
    """Scores the model's output frames against grammars."""

    def __init__(self, alphabet):
        self.alphabet = alphabet
        self._canon = {}

    def canon(self, dev):
        key = str(dev)
        if key not in self._canon:
            self._canon[key] = torch.as_tensor(self.alphabet.canonical_indices(), dtype=torch.int32).to(dev)
        return self._canon[key]

    def scores(self, model_output, lens, grammars, want_best=True):
        """Device tensors (logp [B,G], best [B,G], labels [B,G,T], label_lens [B,G]); the last three None without want_best.  Under a
        weighted grammar logp is ln Z, a weighted score that is a probability only when the weights normalise, and best is the best
        path's log-probability plus its weight."""
        grammars = list(grammars)
        dev = model_output.device
        T, B = int(model_output.shape[0]), int(model_output.shape[1])
        groups = group_grammars(grammars, T, B, want_best)
        outs =[ops.ctc_grammar_scores(model_output.detach(), lens, pack_grammars(grp, dev), self.canon(dev), want_best) for grp in groups]
        if len(outs) == 1:
            return outs[0]
        return tuple(torch.cat([o[k] for o in outs], dim=1) if want_best or k == 0 else None for k in range(4))

    def line_log_prob(self, model_output, lens, grammars, which, max_lattice_bytes=None):
        """ln P [B] (fp32 device tensor) that line b's text is in grammars[which[b]], with autograd to `model_output` ([T,B,V] logits on
        the device).  `grammars` a list of Grammar, `which` B indices into it (several lines may share a grammar).  The kernel stores
        T * lines * (largest states + largest arcs) * 4 bytes of forward rows per call; a batch that needs more than max_lattice_bytes
        (default, and at most, the kernel's 2 GiB) is cut into consecutive chunks of lines, with bit-identical results.  Without
        autograd (torch.no_grad, or an output that needs no gradient) only the forward sweep runs."""
        grammars = list(grammars)
        dev = model_output.device
        B = int(model_output.shape[1])
        which = [int(k) for k in (which.tolist() if torch.is_tensor(which) else which)]
        if len(which) != B:
            raise ValueError("GrammarMatcher.line_log_prob: %d entries of which for %d lines" % (len(which), B))
        if not grammars or min(which) < 0 or max(which) >= len(grammars):
            raise ValueError("GrammarMatcher.line_log_prob: which must index the %d grammars" % len(grammars))
        for g in grammars:
            if g.n_states + g.n_arcs > ops.GRAMMAR_CELLS_MAX:
                raise ValueError("GrammarMatcher: %s has %d states + %d arcs, more than the kernel's %d cells"
                                 % (g.name, g.n_states, g.n_arcs, ops.GRAMMAR_CELLS_MAX))
        packed = pack_grammars(grammars, dev)
        if packed["max_states"] + packed["max_arcs"] > ops.GRAMMAR_CELLS_MAX:
            raise ValueError("GrammarMatcher.line_log_prob: the largest state count %d plus the largest arc count %d of the grammars exceed "
                             "the kernel's %d cells: score them in separate calls" % (packed["max_states"], packed["max_arcs"],
                                                                                     ops.GRAMMAR_CELLS_MAX))
        which_dev = torch.as_tensor(which, dtype=torch.int32).to(dev)
        lens_dev = ops._lens_canon("GrammarMatcher.line_log_prob", model_output, lens, None)
        if not (torch.is_grad_enabled() and model_output.requires_grad):
            return ops.ctc_grammar_grad(model_output.detach(), lens_dev, packed, which_dev, self.canon(dev))[0]
        return _LineLogProbFn.apply(model_output, lens_dev, packed, which_dev, self.canon(dev), max_lattice_bytes)

    def match(self, model_output, lens, grammars):
        """`model_output` [T,B,V] logits on the device, `lens` the lines' frame counts, `grammars` a list of Grammar.  Returns
        GrammarHits of host arrays from one device-to-host copy: logp [B,G] (natural log of the probability that the line's text is in
        the language, -inf for 0), prob = exp(logp), best_logp [B,G] (the score of the best single path through the grammar), best_labels
        [B][G] (its labelling as alphabet indices; None where nothing is accepted) and best_text [B][G] (the same as utf-8)."""
        grammars = list(grammars)
        B = int(model_output.shape[1])
        if not grammars:
            z = np.zeros((B, 0), dtype=np.float32)
            return GrammarHits(z, z.astype(np.float64), z, [[] for _ in range(B)], [[] for _ in range(B)])
        logp, best, labels, ln = self.scores(model_output, lens, grammars, True)
        logp, best, labels, ln = one_copy([logp.unsqueeze(-1), best.unsqueeze(-1), labels, ln.unsqueeze(-1)])
        logp, best, ln = logp[..., 0], best[..., 0], ln[..., 0]
        idx_to_char = self.alphabet.idx_to_char
        lab = [[None if ln[b, g] < 0 else [int(v) for v in labels[b, g, :ln[b, g]]] for g in range(len(grammars))] for b in range(B)]
        text = [[None if l is None else uxxxx_to_utf8(" ".join(idx_to_char[v] for v in l)) for l in row] for row in lab]
        return GrammarHits(logp, np.exp(logp.astype(np.float64)), best, lab, text)
