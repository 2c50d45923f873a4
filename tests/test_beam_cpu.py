"""CPU: the character n-gram LM's resolved tables (vistaocr_amd/lm.py) against a direct ARPA backoff lookup, the fp64 restatement of
the beam search (tests/beam_ref.py) against brute force, its exact-tie rule and counters on the pinned inputs of the fp64 seam tests
(tests/beam_cases.py), and the argument validation of the beam-search entry points (no launch)."""
import ctypes
import math

import numpy as np
import pytest

from tests import beam_cases as bc
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


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("T,ncls,K", [(5, 2, 64), (4, 3, 128)])
def test_restatement_with_exact_ties_equals_brute_force(tmp_path, with_lm, T, ncls, K):
    """The brute-force agreement holds with exact_ties=True: hypotheses and scores are the default's, nothing is pruned so no prefix
    ever comes back (remerges = 0), and every finite candidate of the fullest frame is counted."""
    lm = _tiny_lm(tmp_path) if with_lm else None
    alpha, beta = (0.7, 0.3) if with_lm else (0.0, 0.2)
    rng = np.random.default_rng(T * 10 + ncls)
    logits = rng.normal(0, 1.5, size=(T, len(ALPHA)))
    logits[:, ncls + 1:] = -np.inf
    brute = br.brute_force(logits, list(range(1, ncls + 1)), lm=lm, alpha=alpha, beta=beta)
    stats = {}
    hyps, gap = br.beam_search(logits, T, K, nbest=len(brute), lm=lm, alpha=alpha, beta=beta, exact_ties=True, stats=stats)
    assert hyps == br.beam_search(logits, T, K, nbest=len(brute), lm=lm, alpha=alpha, beta=beta)[0]
    assert [h[0] for h in hyps] == [h[0] for h in brute]
    for h, b in zip(hyps, brute):
        assert np.allclose(h[1:], b[1:], rtol=1e-9, atol=1e-9)
    assert stats["remerges"] == 0 and stats["kth_ties"] == 0 and stats["final_ties"] == 0
    assert 0 < stats["max_live"] <= sum(ncls ** n for n in range(T)) * (ncls + 1)        # the prefixes before the last frame


def test_exact_ties_rule():
    """Two bitwise-equal columns: the default sees gap 0.0 (the line is undecided); with exact_ties the tie is decided by the slot id
    and what enters min_gap is the distance to the nearest different score, which tie_gap finds on either side."""
    assert br.tie_gap(np.array([3.0, 1.0, 1.0, 0.5, -np.inf]), 1.0) == 0.5
    assert br.tie_gap(np.array([1.25, 1.0, 1.0, 0.5]), 1.0) == 0.25
    assert br.tie_gap(np.array([1.0, 1.0]), 1.0) == np.inf
    x = np.array([[0.0, 1.0, 1.0, -1.0]] * 2)                        # classes 1 and 2 tie in every frame
    s0, s1 = {}, {}
    h0, g0 = br.beam_search(x, 2, 2, nbest=2, stats=s0)
    h1, g1 = br.beam_search(x, 2, 2, nbest=2, exact_ties=True, stats=s1)
    assert g0 == 0.0 and g1 > 0.1 and h0 == h1 and s0 == s1
    # frame 1 has 2 stays and 4 finite extensions (a repeat needs a blank first: the other 2 are -inf)
    assert s0["final_ties"] == 1 and s0["kth_ties"] == 0 and s0["max_live"] == 6
    assert [h[0] for h in h1] == [[1], [2]]                          # the smaller slot id first
    h2, g2 = br.beam_search(x, 2, 1, nbest=1, exact_ties=True, stats=s1)
    assert s1["kth_ties"] == 1 and h2[0][0] == [1] and g2 > 0.1       # K = 1: frame 0 cuts between the twins


ALL_CHAR = bc.CHAR_DENSE + bc.CHAR_VARIANTS + ["big_K128_V256"] + bc.CHAR_INTERMEDIATE + bc.CHAR_TIES + bc.CHAR_COMEBACK


def test_every_pinned_case_is_listed():
    assert sorted(ALL_CHAR) == sorted(bc.CHAR_CASES)


@pytest.mark.parametrize("name", ALL_CHAR)
def test_pinned_inputs_meet_floors_and_counters(name):
    """The inputs of tests/test_beam_fp64_gpu.py, by the restatement alone: at least half of the lines of every case are decided by
    TAU; the dense cases have K*V/2 live candidates on every compared line; the tie cases cut inside exact ties and rank exact ties;
    every come-back line merges into a prefix that returned under a new node id."""
    case, ref = bc.char_case(name), bc.char_reference(name)
    bc.check_pinned(name, case, ref)
    if name in bc.CHAR_TIES:
        assert case.exact_ties and bc.total(case, ref, "kth_ties") > 0 and bc.total(case, ref, "final_ties") > 0
        for dst, src in (bc.ENGLISH_PAIRS if name == "tie_english_K16" else bc.V12_PAIRS):
            assert case.x[:, :, dst].tobytes() == case.x[:, :, src].tobytes()
    else:
        assert not case.exact_ties
    if name in bc.CHAR_COMEBACK:
        assert all(r.stats["remerges"] > 0 and r.gap >= bc.TAU for r in ref)
    if name == "ragged_K16_lm":
        T = case.x.shape[0]
        assert {0, 1, T} <= set(case.lens) and max(case.lens) > T
        assert all(ref[b].stats["max_live"] >= case.K * case.x.shape[2] / 2 for b in bc.decided(case, ref) if case.lens[b] >= 3)
    if name in bc.CHAR_INTERMEDIATE:
        assert case.lens == list(range(1, case.x.shape[0] + 1)) and case.nbest == case.K


def test_hand_built_come_back():
    """HAND_PROBS: "a" is cut after frame 1 while "" and its child "ab" stay, comes back from "" at frame 2 under a new node id,
    and the merge of a + b into ab at frame 3 crosses the two ids.  The beams after frames 0 - 2 are the ones written down in
    HAND_KEPT, and the final beam is the brute force over the alignments those beams can still see."""
    x = bc.hand_logits()[:, 0]
    K = bc.HAND_K
    for t, kept in enumerate(bc.HAND_KEPT):
        hyps, _ = br.beam_search(x, t + 1, K, nbest=K)
        assert {tuple(h[0]) for h in hyps} == kept, t
    stats = {}
    hyps, gap = br.beam_search(x, 4, K, nbest=K, stats=stats)
    assert stats["remerges"] == 1 and gap > 1e-2
    want = sorted(bc.kept_path_scores(br.class_logprobs(x), bc.HAND_KEPT).items(), key=lambda kv: -kv[1])[:K]
    assert [tuple(h[0]) for h in hyps] == [w[0] for w in want]
    assert np.allclose([h[2] for h in hyps], [w[1] for w in want], rtol=0, atol=1e-12)
    assert (1, 2) in [w[0] for w in want]


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
