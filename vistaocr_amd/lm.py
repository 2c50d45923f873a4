"""Character n-gram language model for the CTC prefix beam search (vocr_ctc_beam_search).

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

    def __init__(self, logp, nxt, eos, start, order, states):
        self.logp, self.next, self.eos, self.start, self.order, self.states = logp, nxt, eos, int(start), int(order), states
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
        return cls(logp[:, :V].copy(), nxt[:, :V].astype(np.int32), logp[:, V].copy(), st, N, states)

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
