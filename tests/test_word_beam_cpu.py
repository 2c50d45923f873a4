"""CPU: the word n-gram LM's tables (vistaocr_amd/lm.py WordNgramLM) against a direct ARPA backoff lookup, its lexicon trie and
look-ahead, the fp64 restatement of the word beam search (tests/word_beam_ref.py) against brute force, its exact-tie rule and counters
on the pinned inputs of the fp64 seam tests (tests/beam_cases.py), and the argument validation of the word beam-search entry points
(no launch)."""
import ctypes

import numpy as np
import pytest

from tests import beam_cases as bc
from tests import word_beam_ref as wr
from vistaocr_amd.alphabet import Alphabet
from vistaocr_amd.lm import KIND_LETTER, KIND_SINGLE, KIND_SPACE, LN10, WordNgramLM, _parse_arpa

# blank, a, b, c, space, '.', '1': letters a b c, a space, two singles ('1' is not in the LMs below: it scores as <unk>)
ALPHA = Alphabet(["<ctc-blank>", "u0061", "u0062", "u0063", "u0020", "u002e", "u0031"], left_to_right=True)
LEXICON = {"u0061", "u0062", "u0061_u0062", "u0062_u0061", "u0063_u0061_u0062"}
DROPPED = 3          # u0078 (no such symbol), u0061_u002e (a letter and a single), u0020 (spaces are never tokens)

ARPA3 = """\\data\\
ngram 1=12
ngram 2=9
ngram 3=4

\\1-grams:
-1.0 </s>
-99 <s> -0.3
-2.0 <unk> -0.2
-0.8 u0061 -0.25
-1.1 u0062 -0.1
-0.9 u0061_u0062 -0.3
-1.3 u0062_u0061 -0.15
-1.6 u0063_u0061_u0062 -0.2
-1.2 u002e -0.4
-2.5 u0078
-2.2 u0061_u002e
-2.4 u0020

\\2-grams:
-0.3 <s> u0061 -0.1
-0.5 <s> u0061_u0062 -0.2
-0.4 u0061 u0062 -0.15
-0.6 u0061_u0062 u002e -0.05
-0.7 u0062 u0063_u0061_u0062
-0.2 u002e </s>
-0.9 <unk> u0061
-0.5 u0061 u0078
-0.8 u0062_u0061 </s>

\\3-grams:
-0.1 <s> u0061 u0062
-0.2 u0061 u0062 u0063_u0061_u0062
-0.3 <s> u0061_u0062 u002e
-0.25 u0061_u0062 u002e </s>

\\end\\
"""

ARPA3_NO_UNK = (ARPA3.replace("ngram 1=12", "ngram 1=11").replace("ngram 2=9", "ngram 2=8").replace("-2.0 <unk> -0.2\n", "")
                .replace("-0.9 <unk> u0061\n", ""))

ARPA1 = """\\data\\
ngram 1=6

\\1-grams:
-1.0 </s>
-99 <s>
-0.6 u0061
-0.9 u0062_u0061
-1.4 u002e
-2.0 <unk>

\\end\\
"""

UNK_LOGP = -7.0


def _lm(tmp_path, text, unk_logp=None, name="w.arpa"):
    p = tmp_path / name
    p.write_text(text)
    return WordNgramLM.from_arpa(str(p), ALPHA, unk_logp=unk_logp), _parse_arpa(str(p))


def _variants(tmp_path):
    yield _lm(tmp_path, ARPA3, name="a.arpa") + (None,)
    yield _lm(tmp_path, ARPA3_NO_UNK, unk_logp=UNK_LOGP, name="b.arpa") + (UNK_LOGP,)
    yield _lm(tmp_path, ARPA1, name="c.arpa") + (None,)


def test_lookups_equal_direct_backoff(tmp_path):
    """Every state row, and random token sequences walked from <s>, against the direct backoff over the parsed n-grams: listed n-grams,
    misses with backoff chains of every length, <unk> (from the LM, or unk_logp and a fresh history), </s>."""
    for lm, grams, unk in _variants(tmp_path):
        N = max(grams)
        assert lm.order == N
        assert lm.off[0] == 0 and lm.off[1] == len(lm.tokens) and lm.off[-1] == len(lm.succ_tok)
        assert all(lm.back[s] < s for s in range(1, lm.num_states))
        for s, h in enumerate(lm.states):
            lo, hi = lm.off[s], lm.off[s + 1]
            assert s == 0 or list(lm.succ_tok[lo:hi]) == sorted(lm.succ_tok[lo:hi])
            for i, w in enumerate(lm.tokens):
                if w == "<s>":
                    continue
                got, _ = lm.lookup(s, i)
                want = wr.direct_logp(grams, h, w, unk)
                assert abs(got - want) < 1e-9, (h, w, got, want)
        produced = [w for w in lm.tokens if w not in ("<s>", "<unk>")] + ["<unk>"]
        rng = np.random.default_rng(N)
        for trial in range(400):
            seq = [produced[i] for i in rng.integers(0, len(produced), size=int(rng.integers(0, 6)))]
            s, tab, ref, hist = lm.start, 0.0, 0.0, ("<s>",)
            for w in seq + ["</s>"]:
                lp, s = lm.lookup(s, lm.tokens.index(w))
                tab += lp
                ref += wr.direct_logp(grams, hist, w, unk)
                hist = () if (w == "<unk>" and unk is not None) else hist + (w,)
            assert abs(tab - ref) < 1e-9, (seq, tab, ref)
        assert lm.states[lm.start] == (("<s>",) if N > 1 else ())


def test_trie_lexicon_lookahead_and_dropped(tmp_path):
    lm, grams = _lm(tmp_path, ARPA3)
    assert lm.dropped == DROPPED and set(lm.lexicon) == LEXICON and lm.num_words == len(LEXICON)
    assert list(lm.kind) == [0, KIND_LETTER, KIND_LETTER, KIND_LETTER, KIND_SPACE, KIND_SINGLE, KIND_SINGLE]
    assert lm.tokens[lm.tok[5]] == "u002e" and lm.tok[6] == lm.unk                 # '1' is not in the LM: <unk>
    words, below = {}, {}

    def walk(v, path):
        got = []
        if lm.trie_tok[v] >= 0:
            words[lm.tokens[lm.trie_tok[v]]] = path
            got.append(grams[1][(lm.tokens[lm.trie_tok[v]],)][0] * LN10)
        for c in range(len(ALPHA)):
            if lm.trie_next[v, c] >= 0:
                assert lm.kind[c] == KIND_LETTER
                got.extend(walk(lm.trie_next[v, c], path + (c,)))
        below[v] = max(got)
        return got

    walk(0, ())
    assert set(words) == LEXICON and len(below) == lm.num_trie_nodes
    for w, path in words.items():
        assert "_".join(ALPHA.idx_to_char[c] for c in path) == w
    for v, m in below.items():
        assert abs(lm.trie_la[v] - m) < 1e-12
    _lm(tmp_path, ARPA3, name="small.arpa")
    with pytest.raises(ValueError, match="exceed the table limit"):
        WordNgramLM.from_arpa(str(tmp_path / "small.arpa"), ALPHA, max_table_bytes=256)
    with pytest.raises(ValueError, match="unk_logp"):
        _lm(tmp_path, ARPA3_NO_UNK, name="nounk.arpa")


CASES = [(4, [1, 2, 4]), (4, [1, 5, 6]), (5, [1, 2]), (4, [3, 1, 2])]


@pytest.mark.parametrize("oov", [None, -2.5])
@pytest.mark.parametrize("alpha,beta", [(0.0, 0.3), (0.9, 0.4)])
@pytest.mark.parametrize("T,cls", CASES)
def test_restatement_equals_brute_force(tmp_path, T, cls, alpha, beta, oov):
    """K = 128 holds every prefix (at most 121 here), so the search is exact: every hypothesis of the brute force (ln P_ctc from
    F.ctc_loss in fp64 + alpha LM(tokens, </s>) + beta n_tokens, from a direct backoff over the parsed ARPA) comes out in the same
    order with the same scores, closed and open vocabulary, with and without the LM in the ranking."""
    lm, grams = _lm(tmp_path, ARPA3)
    rng = np.random.default_rng(T * 100 + sum(cls))
    V = len(ALPHA)
    logits = rng.normal(0, 1.5, size=(T, V))
    mask = np.ones(V, dtype=bool)
    mask[[0] + cls] = False
    logits[:, mask] = -np.inf
    brute = wr.brute_force(logits, cls, ALPHA, grams, alpha=alpha, beta=beta, oov=oov)
    assert brute
    hyps, _ = wr.beam_search(logits, T, 128, lm, nbest=len(brute), alpha=alpha, beta=beta, oov=oov)
    assert len(hyps) == len(brute)
    for (lab, tot, ac, lmv), (blab, btot, bac, blm) in zip(hyps, brute):
        assert lab == blab
        assert abs(tot - btot) < 1e-9 * max(1.0, abs(btot)) and abs(ac - bac) < 1e-9 * max(1.0, abs(bac))
        assert abs(lmv - blm) < 1e-9 * max(1.0, abs(blm))


@pytest.mark.parametrize("oov", [None, -2.5])
@pytest.mark.parametrize("T,cls", CASES)
def test_restatement_with_exact_ties_equals_brute_force(tmp_path, T, cls, oov):
    """The brute-force agreement holds with exact_ties=True: the hypotheses are the default's and the brute force's, and with every
    prefix held no prefix ever comes back."""
    lm, grams = _lm(tmp_path, ARPA3)
    rng = np.random.default_rng(T * 100 + sum(cls))
    logits = rng.normal(0, 1.5, size=(T, len(ALPHA)))
    mask = np.ones(len(ALPHA), dtype=bool)
    mask[[0] + cls] = False
    logits[:, mask] = -np.inf
    brute = wr.brute_force(logits, cls, ALPHA, grams, alpha=0.9, beta=0.4, oov=oov)
    stats = {}
    hyps, _ = wr.beam_search(logits, T, 128, lm, nbest=len(brute), alpha=0.9, beta=0.4, oov=oov, exact_ties=True, stats=stats)
    assert hyps == wr.beam_search(logits, T, 128, lm, nbest=len(brute), alpha=0.9, beta=0.4, oov=oov)[0]
    assert [h[0] for h in hyps] == [b[0] for b in brute]
    for h, b in zip(hyps, brute):
        assert np.allclose(h[1:], b[1:], rtol=1e-9, atol=1e-9)
    assert stats["remerges"] == 0 and stats["kth_ties"] == 0 and stats["max_live"] > 0


ALL_WORD = bc.WORD_DENSE + ["w_big_K128_V256", "w_tie_lm_K6"]


def test_every_pinned_case_is_listed():
    assert sorted(ALL_WORD) == sorted(bc.WORD_CASES)


@pytest.mark.parametrize("name", ALL_WORD)
def test_pinned_inputs_meet_floors_and_counters(name):
    """The inputs of tests/test_word_beam_fp64_gpu.py, by the restatement alone: at least half of the lines of every case are decided
    by TAU, the open-vocabulary dense cases have K*V/2 live candidates on every compared line, some closed-vocabulary lines output
    nothing, and the LM tie case (letters d and e start no lexicon word and share one column bit for bit, so both enter the OOV
    state with the same look-ahead and close score) cuts inside exact ties and ranks exact ties."""
    case, ref = bc.word_case(name), bc.word_reference(name)
    bc.check_pinned(name, case, ref)
    if name == "w_tie_lm_K6":
        assert case.exact_ties and case.alpha != 0 and case.oov is not None
        assert bc.total(case, ref, "kth_ties") > 0 and bc.total(case, ref, "final_ties") > 0
        assert case.x[:, :, 8].tobytes() == case.x[:, :, 7].tobytes()
        assert all(case.lm.trie_next[0, c] <= 0 and case.lm.kind[c] == KIND_LETTER for c in (7, 8))
    else:
        assert not case.exact_ties
    if name in ("w_K5_closed", "w_K16_closed"):
        lines = bc.decided(case, ref)
        assert 0 < sum(1 for b in lines if not ref[b].hyps) < len(lines)


def test_restatement_closed_vocabulary_drops_open_words(tmp_path):
    """Frames that can only spell 'c a' (a prefix of 'cab' that is no word): with a closed vocabulary no hypothesis survives."""
    lm, grams = _lm(tmp_path, ARPA3)
    lg = np.full((2, len(ALPHA)), -np.inf)
    lg[0, 3] = 0.0
    lg[1, 1] = 0.0
    hyps, _ = wr.beam_search(lg, 2, 8, lm, nbest=2)
    assert hyps == [] and wr.brute_force(lg, [1, 3], ALPHA, grams) == []
    hyps, _ = wr.beam_search(lg, 2, 8, lm, nbest=2, oov=-1.0)
    assert [h[0] for h in hyps] == [[3, 1]]


def test_word_beam_argument_validation_without_gpu():
    from vistaocr_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    ninf = float("-inf")
    assert lib.vocr_ctc_word_beam_workspace_bytes(294, 32, 96, 16, 1) == 294 * 32 * 16 * 8
    assert lib.vocr_ctc_word_beam_workspace_bytes(294, 32, 257, 16, 1) == 0
    assert lib.vocr_ctc_word_beam_workspace_bytes(294, 32, 96, 129, 1) == 0
    assert lib.vocr_ctc_word_beam_workspace_bytes(294, 32, 96, 8, 9) == 0
    assert lib.vocr_ctc_word_beam_workspace_bytes(0, 32, 96, 8, 1) == 0
    ws = lib.vocr_ctc_word_beam_workspace_bytes(10, 2, 96, 8, 2)

    def run(logits=one, lens=one, t=10, b=2, v=96, canon=None, beam=8, nbest=2, kind=one, tok=one, tnext=one, ttok=one, tla=one,
            nodes=5, off=one, stok=one, slogp=one, snext=one, bow=one, back=one, states=4, succ=20, tokens=10, start=1, unk=2, eos=3,
            w=0.8, wb=0.0, oov=ninf, labels=one, olens=one, scores=one, work=one, nbytes=ws):
        return lib.vocr_ctc_word_beam_search(logits, lens, t, b, v, canon, beam, nbest, kind, tok, tnext, ttok, tla, nodes, off, stok,
                                             slogp, snext, bow, back, states, succ, tokens, start, unk, eos, w, wb, oov, labels, olens,
                                             scores, work, nbytes, None)

    def refused(match, **kw):
        assert run(**kw) == -1
        assert match.encode() in lib.vocr_last_error(), lib.vocr_last_error()

    refused("null pointer", logits=None)
    refused("null pointer", lens=None)
    refused("null pointer", labels=None)
    refused("null pointer", work=None)
    refused("null table pointer", kind=None)
    refused("null table pointer", tnext=None)
    refused("null table pointer", back=None)
    refused("1 <= v <= 256", v=257)
    refused("1 <= v <= 256", t=0)
    refused("1 <= beam <= 128", beam=0)
    refused("1 <= beam <= 128", beam=129)
    refused("1 <= nbest <= beam", nbest=9)
    refused("lm_succ >= lm_tokens", succ=9)
    refused("lm_succ >= lm_tokens", nodes=0)
    refused("lm_succ >= lm_tokens", states=0)
    refused("lm_start < lm_states", start=4)
    refused("lm_start < lm_states", unk=10)
    refused("lm_start < lm_states", eos=-1)
    refused("finite", w=float("inf"))
    refused("finite", wb=float("nan"))
    refused("finite", oov=float("nan"))
    refused("finite", oov=float("inf"))
    refused("workspace too small", nbytes=ws - 1)
