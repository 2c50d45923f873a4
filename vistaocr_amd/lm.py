"""Language models of the CTC prefix beam searches: CharNgramLM (a character n-gram, vocr_ctc_beam_search) below, and WordNgramLM
(a word n-gram with a lexicon, vocr_ctc_word_beam_search) at the end of the module.

The reference decodes its reported results with an eesen WFST built from a lexicon and an LM over `uxxxx` units
(src/decoder.py:11-109); its LmDecoder maps model symbols to LM units one to one by their `uxxxx` strings.  This module keeps that
boundary and replaces the WFST by a character n-gram in ARPA format, resolved into dense tables the kernel reads with one load each:

  states      the LM histories: every listed n-gram of order < N (the model's order) plus the empty history (state 0)
  logp[s][c]  ln P(c | history s) with the ARPA backoff already applied (natural log; ARPA stores log10)
  next[s][c]  the state after c: the longest suffix of history + c that is a state
  eos[s]      ln P(</s> | history s)
  start       the state of <s> (the empty history when the LM does not list <s>)

Reducing a history to its longest listed suffix is exact for ARPA files: a history that is not listed has no listed extensions and a
backoff weight of one.  Model symbols that the LM does not list are scored as <unk> (and continue from the history + <unk>); an LM
without <unk> needs `unk_logp`, a fixed log-probability after which the history starts again from the empty one.  Column 0 (the CTC
blank) is never extended by the search; its entries are 0 and the state itself."""
import math

import numpy as np

LN10 = math.log(10.0)
DEFAULT_MAX_TABLE_BYTES = 1 << 30


def _parse_arpa(path):
    """{order: {tuple(units): (log10 p, log10 backoff)}} of an ARPA file, the \\data\\ counts checked."""
    counts, grams = {}, {}
    section = None
    with open(path, encoding="utf-8") as fh:
        for lineno, raw in enumerate(fh, 1):
            line = raw.strip()
            if not line:
                continue
            if line == "\\data\\":
                section = "data"
                continue
            if line == "\\end\\":
                section = "end"
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                section = int(line[1:-len("-grams:")])
                if section not in counts:
                    raise ValueError("%s:%d: %d-grams section without a \\data\\ count" % (path, lineno, section))
                grams[section] = {}
                continue
            if section == "data":
                if not line.startswith("ngram "):
                    raise ValueError("%s:%d: unexpected line in \\data\\: %r" % (path, lineno, line))
                n, c = line[len("ngram "):].split("=")
                counts[int(n)] = int(c)
            elif isinstance(section, int):
                parts = line.split()
                n = section
                if len(parts) not in (n + 1, n + 2):
                    raise ValueError("%s:%d: a %d-gram line needs %d or %d fields: %r" % (path, lineno, n, n + 1, n + 2, line))
                grams[n][tuple(parts[1:n + 1])] = (float(parts[0]), float(parts[n + 1]) if len(parts) == n + 2 else 0.0)
            elif section is None:
                continue                                          # text before \data\ is allowed
            else:
                raise ValueError("%s:%d: unexpected line %r" % (path, lineno, line))
    if section != "end":
        raise ValueError("%s: no \\end\\ marker" % path)
    if not counts or sorted(counts) != list(range(1, max(counts) + 1)):
        raise ValueError("%s: \\data\\ must count orders 1..N, got %s" % (path, sorted(counts)))
    for n, c in counts.items():
        got = len(grams.get(n, {}))
        if got != c:
            raise ValueError("%s: \\data\\ says ngram %d=%d, the file lists %d" % (path, n, c, got))
    return grams


class CharNgramLM(object):
    """Resolved tables of a character n-gram over the classes of an alphabet (see the module docstring).  numpy arrays:
    `logp` float64 [S, V], `next` int32 [S, V], `eos` float64 [S]; `start` int; `order` N; `states` the history tuples."""

    def __init__(self, logp, nxt, eos, start, order, states, alphabet=None):
        self.logp, self.next, self.eos, self.start, self.order, self.states = logp, nxt, eos, int(start), int(order), states
        self.alphabet = alphabet                          # the alphabet the tables were resolved for (Grammar.from_ngram reads it)
        self._dev = {}

    @property
    def num_states(self):
        return self.logp.shape[0]

    @classmethod
    def from_arpa(cls, path, alphabet, unk_logp=None, max_table_bytes=DEFAULT_MAX_TABLE_BYTES):
        grams = _parse_arpa(path)
        N = max(grams)
        V = len(alphabet)
        uni = grams[1]
        has_unk = ("<unk>",) in uni
        if not has_unk and unk_logp is None:
            missing = [alphabet.idx_to_char[c] for c in range(1, V) if (alphabet.idx_to_char[c],) not in uni]
            if missing or ("</s>",) not in uni:
                raise ValueError("%s lists no <unk> and unk_logp is not given, but the model symbols %s%s are not in the LM"
                                 % (path, missing[:8], " and </s>" if ("</s>",) not in uni else ""))
        # states: the empty history, then every listed n-gram of order < N, order by order
        states = [()]
        for n in range(1, N):
            states.extend(sorted(grams[n]))
        S = len(states)
        if S * V * 8 > max_table_bytes:
            raise ValueError("%s: %d LM states x %d symbols x 8 bytes = %.1f MiB exceeds the table limit of %.1f MiB (max_table_bytes)"
                             % (path, S, V, S * V * 8 / 2.0 ** 20, max_table_bytes / 2.0 ** 20))
        sid = {h: i for i, h in enumerate(states)}

        def suffix_state(h):
            while h not in sid:
                h = h[1:]
            return sid[h]

        # columns: the model classes 1..V-1 through their unit (unknown symbols as <unk>), then </s> as column V
        units = [None] + [alphabet.idx_to_char[c] for c in range(1, V)] + ["</s>"]
        col_unit = []
        fixed = np.zeros(V + 1, dtype=bool)                         # scored by unk_logp (no <unk> in the LM)
        for c, u in enumerate(units):
            if c == 0:
                col_unit.append(None)
            elif (u,) in uni:
                col_unit.append(u)
            elif has_unk:
                col_unit.append("<unk>")
            else:
                col_unit.append(None)
                fixed[c] = True
        unit_cols = {}
        for c, u in enumerate(col_unit):
            if u is not None:
                unit_cols.setdefault(u, []).append(c)
        ncol = V + 1
        logp10 = np.zeros((S, ncol), dtype=np.float64)
        nxt = np.zeros((S, ncol), dtype=np.int64)
        # the empty history: unigrams
        for u, cols in unit_cols.items():
            logp10[0, cols] = uni[(u,)][0]
            if N > 1:
                nxt[0, cols] = sid[(u,)]
        # longer histories, order by order: back off to the longest suffix state, then the listed (n+1)-grams
        for n in range(1, N):
            idx = np.array([sid[h] for h in sorted(grams[n])], dtype=np.int64)
            par = np.array([suffix_state(h[1:]) for h in sorted(grams[n])], dtype=np.int64)
            bo = np.array([grams[n][h][1] for h in sorted(grams[n])], dtype=np.float64)
            logp10[idx] = bo[:, None] + logp10[par]
            nxt[idx] = nxt[par]
            rows, cols, vals, nrows, ncols_, nvals = [], [], [], [], [], []
            for g, (p, _bo) in grams[n + 1].items():
                cs = unit_cols.get(g[-1])
                if not cs:
                    continue
                h = g[:-1]
                if h not in sid:
                    raise ValueError("%s: the %d-gram %s extends %s, which the file does not list" % (path, n + 1, g, h))
                s = sid[h]
                for c in cs:
                    rows.append(s)
                    cols.append(c)
                    vals.append(p)
                    if n + 1 < N:
                        nrows.append(s)
                        ncols_.append(c)
                        nvals.append(sid[g])
            if rows:
                logp10[rows, cols] = vals
            if nrows:
                nxt[nrows, ncols_] = nvals
        logp = logp10 * LN10
        if fixed.any():
            logp[:, fixed] = float(unk_logp)
            nxt[:, fixed] = 0
        logp[:, 0] = 0.0
        nxt[:, 0] = np.arange(S)
        if not np.isfinite(logp).all():
            raise ValueError("%s: the resolved LM has non-finite log-probabilities" % path)
        st = sid[("<s>",)] if ("<s>",) in sid else 0
        return cls(logp[:, :V].copy(), nxt[:, :V].astype(np.int32), logp[:, V].copy(), st, N, states, alphabet)

    def to(self, device):
        """The device tables (cached per device): {'lm_logp': fp32 [S,V], 'lm_next': int32 [S,V], 'lm_eos': fp32 [S], 'start': int}."""
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = {"lm_logp": torch.from_numpy(self.logp.astype(np.float32)).to(device),
                              "lm_next": torch.from_numpy(self.next.astype(np.int32)).to(device),
                              "lm_eos": torch.from_numpy(self.eos.astype(np.float32)).to(device),
                              "start": self.start}
        return self._dev[key]


KIND_LETTER, KIND_SPACE, KIND_SINGLE = 1, 2, 3


def class_kinds(alphabet):
    """int32 [V]: the kind of every column by its uxxxx string (0 for the blank): u0020 a space, textutils' punctuation and digits a
    single (a token of its own), anything else a letter (runs of letters are words): the token rule of form_tokenized_words."""
    from .textutils import _DIGITS, _PUNCT
    kinds = np.zeros(len(alphabet), dtype=np.int32)
    for c in range(1, len(alphabet)):
        u = alphabet.idx_to_char[c]
        kinds[c] = KIND_SPACE if u == "u0020" else KIND_SINGLE if (u in _PUNCT or u in _DIGITS) else KIND_LETTER
    return kinds


class WordNgramLM(object):
    """A word n-gram in the reference's token format (form_tokenized_words: a word is its uxxxx letters joined by "_", every
    punctuation mark and digit a token of its own) resolved for the word beam search (vocr_ctc_word_beam_search) over the classes of
    an alphabet.  Tokens of the ARPA file whose units all map to letter classes are the LEXICON; a one-unit token of a single class is
    that class's token; <s>, </s>, <unk> are special; any other token can never be produced and is counted in `dropped`.  numpy
    tables (token ids index `tokens`):

      kind [V], tok [V]     the class kinds (class_kinds) and the LM token of each single class (<unk> where the LM does not list it)
      trie_next [N, V]      the lexicon trie over letter classes (-1: no child, root 0); trie_tok [N] the word ending at a node or -1;
                            trie_la [N] the largest 1-gram ln P of the lexicon words below the node (the look-ahead)
      off [S+1], succ_tok / succ_logp / succ_next [E], bow [S], back [S]
                            the LM: states are the empty history (0) and every listed history of order < N, by length; state s's
                            successors sit at off[s]..off[s+1], sorted by token, with ln P (natural log) and the longest suffix of
                            h + w that is a state.  State 0's list is dense over all tokens.  On a miss a lookup adds bow[s] (the
                            history's ln backoff weight) and goes on from back[s], the state of the history without its oldest token.

    Reducing a history to its longest listed suffix is exact for ARPA files (an unlisted history has no listed extensions and a
    backoff weight of one).  An LM without <unk> needs `unk_logp`: <unk> then scores unk_logp from every state and continues from the
    empty history, as in CharNgramLM."""

    def __init__(self, **tabs):
        self.__dict__.update(tabs)
        self._dev = {}

    @property
    def num_states(self):
        return len(self.bow)

    @property
    def num_trie_nodes(self):
        return self.trie_next.shape[0]

    @property
    def num_words(self):
        return len(self.lexicon)

    @property
    def table_bytes(self):
        return sum(getattr(self, k).size * 4 for k in ("kind", "tok", "trie_next", "trie_tok", "trie_la", "off", "succ_tok", "succ_logp",
                                                        "succ_next", "bow", "back"))

    @classmethod
    def from_arpa(cls, path, alphabet, unk_logp=None, max_table_bytes=DEFAULT_MAX_TABLE_BYTES):
        grams = _parse_arpa(path)
        N = max(grams)
        V = len(alphabet)
        uni = grams[1]
        has_unk = ("<unk>",) in uni
        if not has_unk and unk_logp is None:
            raise ValueError("%s lists no <unk> and unk_logp is not given" % path)
        canon = alphabet.canonical_indices()
        kinds = class_kinds(alphabet)
        unit_cls = {}
        for c in range(1, V):
            unit_cls.setdefault(alphabet.idx_to_char[c], canon[c])
        # sort the 1-gram tokens: lexicon words, single-class tokens, specials; the rest is dropped
        lexicon, singles, dropped = {}, {}, 0
        for (g,) in uni:
            if g in ("<s>", "</s>", "<unk>"):
                continue
            cs = [unit_cls.get(u) for u in g.split("_")]
            if all(c is not None and kinds[c] == KIND_LETTER for c in cs):
                lexicon[g] = tuple(cs)
            elif len(cs) == 1 and cs[0] is not None and kinds[cs[0]] == KIND_SINGLE:
                singles[g] = cs[0]
            else:
                dropped += 1
        tokens = sorted(g for (g,) in uni if g in ("<s>", "</s>", "<unk>") or g in lexicon or g in singles)
        if not has_unk:
            tokens.append("<unk>")
        tid = {g: i for i, g in enumerate(tokens)}
        W = len(tokens)
        unk = tid["<unk>"]
        eos = tid.get("</s>", unk)

        def kept(g):
            return all(w in tid for w in g)

        # LM states: the empty history, then every kept listed n-gram of order < N, by length
        states = [()]
        for n in range(1, N):
            states.extend(sorted(g for g in grams[n] if kept(g)))
        S = len(states)
        sid = {h: i for i, h in enumerate(states)}

        def suffix_state(h):
            while h not in sid:
                h = h[1:]
            return sid[h]

        bow = np.zeros(S, dtype=np.float64)
        back = np.zeros(S, dtype=np.int32)
        for s in range(1, S):
            h = states[s]
            bow[s] = grams[len(h)][h][1] * LN10
            back[s] = suffix_state(h[1:])
        # successors: state 0 dense over all tokens, the others from the listed (n+1)-grams
        logp0 = np.full(W, -np.inf)
        next0 = np.zeros(W, dtype=np.int64)
        for g, i in tid.items():
            if (g,) in uni:
                logp0[i] = uni[(g,)][0] * LN10
                next0[i] = sid.get((g,), 0) if N > 1 else 0
        if not has_unk:
            logp0[unk] = float(unk_logp)
        es, et, ep, en = [], [], [], []
        for n in range(1, N):
            for g, (p, _bo) in grams[n + 1].items():
                if not kept(g):
                    continue
                h = g[:-1]
                if h not in sid:
                    raise ValueError("%s: the %d-gram %s extends %s, which the file does not list" % (path, n + 1, g, h))
                es.append(sid[h])
                et.append(tid[g[-1]])
                ep.append(p * LN10)
                en.append(sid[g] if n + 1 < N else suffix_state(g[1:]))
        if not has_unk and S > 1:                                  # <unk> from every state: unk_logp, then the empty history
            es.extend(range(1, S))
            et.extend([unk] * (S - 1))
            ep.extend([float(unk_logp)] * (S - 1))
            en.extend([0] * (S - 1))
        es, et = np.asarray(es, dtype=np.int64), np.asarray(et, dtype=np.int64)
        ep, en = np.asarray(ep, dtype=np.float64), np.asarray(en, dtype=np.int64)
        order = np.lexsort((et, es))
        es, et, ep, en = es[order], et[order], ep[order], en[order]
        counts = np.bincount(es, minlength=S)
        counts[0] = W
        off = np.zeros(S + 1, dtype=np.int64)
        off[1:] = np.cumsum(counts)
        succ_tok = np.concatenate([np.arange(W), et]).astype(np.int32)
        succ_logp = np.concatenate([logp0, ep])
        succ_next = np.concatenate([next0, en]).astype(np.int32)
        # the lexicon trie over letter classes
        words = sorted(lexicon.items(), key=lambda kv: kv[1])
        n_nodes = 1 + len({cs[:i] for _, cs in words for i in range(1, len(cs) + 1)})
        nbytes = 4 * (n_nodes * (V + 2) + 2 * V + (S + 1) + 3 * len(succ_tok) + 2 * S)
        if nbytes > max_table_bytes:
            raise ValueError("%s: %d trie nodes x %d symbols and %d LM states / %d successors = %.1f MiB exceed the table limit of "
                             "%.1f MiB (max_table_bytes)" % (path, n_nodes, V, S, len(succ_tok), nbytes / 2.0 ** 20,
                                                              max_table_bytes / 2.0 ** 20))
        trie_next = np.full((n_nodes, V), -1, dtype=np.int32)
        trie_tok = np.full(n_nodes, -1, dtype=np.int32)
        trie_la = np.full(n_nodes, -np.inf)
        parent = np.zeros(n_nodes, dtype=np.int64)
        nn = 1
        for g, cs in words:
            v = 0
            for c in cs:
                nx = trie_next[v, c]
                if nx < 0:
                    nx = trie_next[v, c] = nn
                    parent[nn] = v
                    nn += 1
                v = nx
            trie_tok[v] = tid[g]
            trie_la[v] = uni[(g,)][0] * LN10
        for v in range(n_nodes - 1, 0, -1):                         # children come after their parents
            trie_la[parent[v]] = max(trie_la[parent[v]], trie_la[v])
        tok = np.full(V, -1, dtype=np.int32)
        for c in range(1, V):
            if kinds[c] == KIND_SINGLE:
                u = alphabet.idx_to_char[c]
                tok[c] = tid[u] if u in singles else unk
        if not np.isfinite(succ_logp).all() or not np.isfinite(bow).all():
            raise ValueError("%s: the resolved LM has non-finite log-probabilities" % path)
        st = sid[("<s>",)] if ("<s>",) in sid else 0
        return cls(kind=kinds, tok=tok, trie_next=trie_next, trie_tok=trie_tok, trie_la=trie_la, off=off.astype(np.int32),
                   succ_tok=succ_tok, succ_logp=succ_logp, succ_next=succ_next, bow=bow, back=back, start=int(st), unk=int(unk),
                   eos=int(eos), order=int(N), tokens=tokens, states=states, lexicon=lexicon, dropped=int(dropped))

    def lookup(self, s, w):
        """(ln P(token w | state s), the state after w) through the tables, as the kernel reads them."""
        add = 0.0
        while s > 0:
            lo, hi = int(self.off[s]), int(self.off[s + 1])
            i = lo + int(np.searchsorted(self.succ_tok[lo:hi], w))
            if i < hi and self.succ_tok[i] == w:
                return add + float(self.succ_logp[i]), int(self.succ_next[i])
            add += float(self.bow[s])
            s = int(self.back[s])
        return add + float(self.succ_logp[w]), int(self.succ_next[w])

    def to(self, device):
        """The device tables (cached per device): int32 / fp32 tensors under the names of the attributes, and the ints start, unk,
        eos and num_tokens."""
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            d = {}
            for k in ("kind", "tok", "trie_next", "trie_tok", "off", "succ_tok", "succ_next", "back"):
                d[k] = torch.from_numpy(np.ascontiguousarray(getattr(self, k), dtype=np.int32)).to(device)
            for k in ("trie_la", "succ_logp", "bow"):
                d[k] = torch.from_numpy(np.ascontiguousarray(getattr(self, k), dtype=np.float32)).to(device)
            d.update(start=self.start, unk=self.unk, eos=self.eos, num_tokens=len(self.tokens))
            self._dev[key] = d
        return self._dev[key]
