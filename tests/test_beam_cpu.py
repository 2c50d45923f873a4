"""CPU: the character n-gram LM's resolved tables (vistaocr_amd/lm.py) against a direct ARPA backoff lookup, the fp64 restatement of
the beam search (tests/beam_ref.py) against brute force, and the argument validation of the beam-search entry points (no launch)."""
import ctypes
import math

import numpy as np
import pytest

from tests import beam_ref as br
from vistaocr_amd.alphabet import Alphabet
from vistaocr_amd.lm import CharNgramLM

# blank, a, b, c, d; 'u0064' (d) is not in the LMs below, 'u0065' (e) is in the LMs but not in the alphabet
ALPHA = Alphabet(["<ctc-blank>", "u0061", "u0062", "u0063", "u0064"], left_to_right=True)

ARPA = {
    1: """\\data\\
ngram 1=6

\\1-grams:
-1.0 </s>
-99 <s>
-0.5 u0061
-0.7 u0062
-1.2 u0063
-1.5 u0065

\\end\\
""",
    2: """\\data\\
ngram 1=7
ngram 2=6

\\1-grams:
-1.1 </s>
-99 <s> -0.3
-0.5 u0061 -0.2
-0.7 u0062 -0.4
-1.2 u0063
-1.5 u0065 -0.1
-2.0 <unk>

\\2-grams:
-0.2 <s> u0061
-0.9 <s> u0063
-0.3 u0061 u0062
-0.6 u0061 </s>
-0.4 u0062 u0061
-0.8 u0065 u0061

\\end\\
""",
    3: """\\data\\
ngram 1=7
ngram 2=6
ngram 3=4

\\1-grams:
-1.1 </s>
-99 <s> -0.3
-0.5 u0061 -0.2
-0.7 u0062 -0.4
-1.2 u0063 -0.25
-1.5 u0065
-2.0 <unk> -0.15

\\2-grams:
-0.2 <s> u0061 -0.1
-0.3 u0061 u0062 -0.35
-0.6 u0061 </s>
-0.4 u0062 u0061 -0.05
-0.5 u0062 u0063
-0.7 <unk> u0061

\\3-grams:
-0.1 <s> u0061 u0062
-0.15 u0061 u0062 u0061
-0.45 u0062 u0061 </s>
-0.3 u0061 u0062 <unk>

\\end\\
""",
    4: """\\data\\
ngram 1=7
ngram 2=5
ngram 3=3
ngram 4=2

\\1-grams:
-1.1 </s>
-99 <s> -0.3
-0.5 u0061 -0.2
-0.7 u0062 -0.4
-1.2 u0063 -0.25
-1.5 u0065
-2.0 <unk>

\\2-grams:
-0.2 <s> u0061 -0.1
-0.3 u0061 u0062 -0.35
-0.4 u0062 u0061 -0.05
-0.5 u0062 u0063 -0.2
-0.6 u0061 </s>

\\3-grams:
-0.1 <s> u0061 u0062 -0.12
-0.15 u0061 u0062 u0061 -0.3
-0.25 u0062 u0061 u0062 -0.2

\\4-grams:
-0.05 <s> u0061 u0062 u0061
-0.35 u0061 u0062 u0061 u0062

\\end\\
""",
}


def _write(tmp_path, order, text=None):
    p = tmp_path / ("lm%d.arpa" % order)
    p.write_text(ARPA[order] if text is None else text)
    return str(p)


def _direct(grams, N, hist, w, unk_logp=None):
    """ln P(w | hist) by the ARPA backoff rule, looked up in the parsed n-grams (hist: a tuple of units, any length)."""
    units = {g[0] for g in grams[1]}
    if w not in units:
        if ("<unk>",) not in grams[1]:
            return unk_logp
        w = "<unk>"
    h = tuple(hist[-(N - 1):]) if N > 1 else ()
    total = 0.0
    while True:
        if len(h) + 1 <= N and h + (w,) in grams[len(h) + 1]:
            return (total + grams[len(h) + 1][h + (w,)][0]) * math.log(10)
        if h and h in grams[len(h)]:
            total += grams[len(h)][h][1]
        h = h[1:]


def _parse(text):
    grams, n = {}, None
    for line in text.splitlines():
        line = line.strip()
        if line.endswith("-grams:"):
            n = int(line[1:-len("-grams:")])
            grams[n] = {}
        elif n and line and not line.startswith("\\"):
            f = line.split()
            grams[n][tuple(f[1:n + 1])] = (float(f[0]), float(f[n + 1]) if len(f) == n + 2 else 0.0)
    return grams


def _unit(c):
    return ALPHA.idx_to_char[c]


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_arpa_tables_equal_direct_backoff_lookup(tmp_path, order):
    unk = -3.0 if order == 1 else None                     # the unigram LM lists no <unk>: model symbol d needs unk_logp
    lm = CharNgramLM.from_arpa(_write(tmp_path, order), ALPHA, unk_logp=unk)
    grams = _parse(ARPA[order])
    N = max(grams)
    assert lm.order == N and lm.logp.shape == (lm.num_states, len(ALPHA)) and lm.next.shape == lm.logp.shape
    known = {g[0] for g in grams[1]}

    def hist_units(seq):
        """The LM history after <s> and the model symbols `seq` (unknown symbols as <unk>, or a reset with unk_logp)."""
        h = ["<s>"]
        for c in seq:
            u = _unit(c)
            if u in known:
                h.append(u)
            elif "<unk>" in known:
                h.append("<unk>")
            else:
                h = []
        return tuple(h)

    # every sequence up to length 5 over a, b, c, d: the tables walked from <s> against the direct lookup with the full history
    rng = np.random.default_rng(order)
    for trial in range(300):
        seq = [int(v) for v in rng.integers(1, 5, size=int(rng.integers(0, 6)))]
        s, tab = lm.start, 0.0
        ref = 0.0
        for i, c in enumerate(seq):
            tab += lm.logp[s, c]
            s = lm.next[s, c]
            ref += _direct(grams, N, hist_units(seq[:i]), _unit(c), unk) if _unit(c) in known or "<unk>" in known else unk
        tab += lm.eos[s]
        ref += _direct(grams, N, hist_units(seq), "</s>", unk)
        assert abs(tab - ref) < 1e-9, (seq, tab, ref)
    # every state row against the direct lookup on the state's own history
    for s, h in enumerate(lm.states):
        for c in range(1, len(ALPHA)):
            want = _direct(grams, N, h, _unit(c), unk) if (_unit(c) in known or "<unk>" in known) else unk
            assert abs(lm.logp[s, c] - want) < 1e-9, (h, c)
        assert abs(lm.eos[s] - _direct(grams, N, h, "</s>", unk)) < 1e-9
        assert lm.logp[s, 0] == 0.0 and lm.next[s, 0] == s
    assert lm.states[lm.start] == (("<s>",) if N > 1 else ())


def test_arpa_errors(tmp_path):
    bad = ARPA[2].replace("ngram 2=6", "ngram 2=7")
    with pytest.raises(ValueError, match="ngram 2=7"):
        CharNgramLM.from_arpa(_write(tmp_path, 2, bad), ALPHA)
    with pytest.raises(ValueError, match="unk_logp"):                                    # d is missing and there is no <unk>
        CharNgramLM.from_arpa(_write(tmp_path, 1), ALPHA)
    with pytest.raises(ValueError, match="exceeds the table limit"):
        CharNgramLM.from_arpa(_write(tmp_path, 3), ALPHA, max_table_bytes=64)
    with pytest.raises(ValueError, match="end"):
        CharNgramLM.from_arpa(_write(tmp_path, 2, ARPA[2].replace("\\end\\", "")), ALPHA)


def _tiny_lm(tmp_path):
    return CharNgramLM.from_arpa(_write(tmp_path, 3), ALPHA)


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("T,ncls,K", [(5, 2, 64), (4, 3, 128)])
def test_restatement_equals_brute_force(tmp_path, with_lm, T, ncls, K):
    """With no pruning and K at least the number of prefixes, the search is exact: every hypothesis scored by brute force
    (ln P_ctc from F.ctc_loss in fp64 + alpha ln P_lm(y </s>) + beta |y|) comes out in the same order with the same scores."""
    lm = _tiny_lm(tmp_path) if with_lm else None
    alpha, beta = (0.7, 0.3) if with_lm else (0.0, 0.2)
    rng = np.random.default_rng(T * 10 + ncls)
    V = len(ALPHA)
    logits = rng.normal(0, 1.5, size=(T, V))
    logits[:, ncls + 1:] = -np.inf                                 # only classes 1..ncls can be emitted
    brute = br.brute_force(logits, list(range(1, ncls + 1)), lm=lm, alpha=alpha, beta=beta)
    hyps, gap = br.beam_search(logits, T, K, nbest=len(brute), lm=lm, alpha=alpha, beta=beta)
    assert len(hyps) == len(brute)
    for (lab, tot, ac, lmv), (blab, btot, bac, blm) in zip(hyps, brute):
        assert lab == blab
        assert abs(tot - btot) < 1e-9 * max(1.0, abs(btot)) and abs(ac - bac) < 1e-9 * max(1.0, abs(bac))
        assert abs(lmv - blm) < 1e-9 * max(1.0, abs(blm))


def test_restatement_merges_repeats_and_classes():
    """Repeat rules and duplicate columns: 'a a' needs a blank between, 'aa' collapses; columns 1 and 4 declared one class."""
    V = 5
    lg = np.full((3, V), -np.inf)
    lg[0, 1] = 0.0
    lg[1, 0] = 0.0
    lg[2, 4] = 0.0                                               # frame 3 emits column 4, which is class 1
    hyps, _ = br.beam_search(lg, 3, 8, nbest=1, canon=[0, 1, 2, 3, 1])
    assert hyps[0][0] == [1, 1] and abs(hyps[0][2]) < 1e-12
    lg[1] = -np.inf
    lg[1, 1] = 0.0
    hyps, _ = br.beam_search(lg, 3, 8, nbest=1, canon=[0, 1, 2, 3, 1])
    assert hyps[0][0] == [1] and abs(hyps[0][2]) < 1e-12


def test_beam_argument_validation_without_gpu():
    from vistaocr_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    ninf = float("-inf")
    assert lib.vocr_ctc_beam_workspace_bytes(294, 32, 96, 16, 1) == 294 * 32 * 16 * 8
    assert lib.vocr_ctc_beam_workspace_bytes(294, 32, 257, 16, 1) == 0
    assert lib.vocr_ctc_beam_workspace_bytes(294, 32, 96, 129, 1) == 0
    assert lib.vocr_ctc_beam_workspace_bytes(294, 32, 96, 8, 9) == 0
    assert lib.vocr_ctc_beam_workspace_bytes(0, 32, 96, 8, 1) == 0
    ws = lib.vocr_ctc_beam_workspace_bytes(10, 2, 96, 8, 2)

    def run(logits=one, lens=one, t=10, b=2, v=96, canon=None, beam=8, nbest=2, lm=(None, None, None, 0, 0), w=0.0, ib=0.0,
            prune=ninf, labels=one, olens=one, scores=one, work=one, nbytes=ws):
        return lib.vocr_ctc_beam_search(logits, lens, t, b, v, canon, beam, nbest, *lm, w, ib, prune, labels, olens, scores, work, nbytes,
                                        None)

    def refused(match, **kw):
        assert run(**kw) == -1
        assert match.encode() in lib.vocr_last_error(), lib.vocr_last_error()

    refused("null pointer", logits=None)
    refused("null pointer", lens=None)
    refused("null pointer", labels=None)
    refused("null pointer", scores=None)
    refused("null pointer", work=None)
    refused("1 <= v <= 256", v=257)
    refused("1 <= v <= 256", t=0)
    refused("1 <= beam <= 128", beam=0)
    refused("1 <= beam <= 128", beam=129)
    refused("1 <= nbest <= beam", nbest=0)
    refused("1 <= nbest <= beam", nbest=9)
    refused("go together", lm=(one, None, one, 4, 0))
    refused("lm_start < lm_states", lm=(one, one, one, 4, 4))
    refused("lm_start < lm_states", lm=(one, one, one, 0, 0))
    refused("lm_start < lm_states", lm=(one, one, one, 4, -1))
    refused("finite", w=float("inf"))
    refused("finite", prune=float("nan"))
    refused("workspace too small", nbytes=ws - 1)
