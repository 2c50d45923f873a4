"""GPU: vocr_ctc_grammar_beam_search (vistaocr_amd/csrc/ctc_beam.hip, the GRAMMAR instantiation) through ops.ctc_grammar_beam_search and
GrammarBeamDecoder: against vocr_ctc_beam_search under the automaton that accepts everything (the same bits), against brute force
where the beam holds every viable prefix, against the fp64 restatement (tests/grammar_beam_ref.py) on dense logits, with per-line
automata, bad indices and a poisoned table, on a trie beyond the sweep kernels' 8192 cells, and at the corners of the distance rule.
The inputs and the score bars are pinned in tests/grammar_beam_cases.py and their floors checked without a GPU by
tests/test_grammar_beam_cpu.py.  Run with -s: every comparison prints how many lines it compared and the largest |score - fp64| it
saw (profiles/ctc_grammar_beam_errors.txt)."""
import numpy as np
import pytest
import torch

import vistaocr_amd as va
from tests import beam_cases as bc
from tests import beam_data as bd
from tests import grammar_beam_cases as gc
from vistaocr_amd import ops
from vistaocr_amd.grammar import Grammar, pack_dense_grammars, pack_grammars

pytestmark = pytest.mark.gpu
NEG = -np.inf


def grammar_bound(T, score, D, N):
    """tests/test_grammar_gpu.py's bound on |fp32 - fp64| of a sweep score over T frames: in-degree D, N cells"""
    return 4.0 * 2.0 ** -24 * ((T + 2) * np.maximum(np.abs(score), 1.0) + T * (D + 2) + N)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _search(c, packed=None, prune=None):
    """The device outputs of a gc.Case (packed: other tables than the grammars' own)."""
    packed = pack_dense_grammars(c.grammars, "cuda") if packed is None else packed
    cd = torch.as_tensor(c.canon, dtype=torch.int32).cuda() if c.canon is not None else None
    out = ops.ctc_grammar_beam_search(_dev(c.x), c.lens, packed, c.which, cd, c.K, c.nbest, c.lm.to("cuda") if c.lm is not None else None,
                                      c.alpha, c.beta, prune)
    torch.cuda.synchronize()
    return out


def _host(out):
    return [o.cpu().numpy() for o in out]


def _bits(a, b):
    return all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))


def _forward_scores(c, out):
    """ops.ctc_align's forward score ln P_ctc(labels | x) of every rank, on the host"""
    cd = torch.as_tensor(c.canon, dtype=torch.int32).cuda() if c.canon is not None else None
    return ops.ctc_align(_dev(c.x), c.lens, out[0], out[1], cd)[0][..., 1].cpu().numpy()


def _acoustic_is_a_lower_bound(name, c, out, equal=False):
    """the search's acoustic score sums only the paths its beam kept: never above the labelling's full forward score, up to the bar"""
    sc, fwd = out[2].cpu().numpy(), _forward_scores(c, out)
    filled = np.isfinite(sc[..., 0])
    bar = gc.bars(c.group)[1] + float(grammar_bound(c.x.shape[0], np.abs(fwd[filled]).max() if filled.any() else 0.0, 1, 0))
    assert (sc[..., 1][filled] <= fwd[filled] + bar).all(), name
    if equal:
        assert np.abs(sc[..., 1][filled] - fwd[filled]).max() <= bar, name


# ------------------------------------------------------------------------------------------------------------------- Sigma*
SIGMA_LENS = [40, 0, 1, 33, 40, 17, 39, 5]


@pytest.mark.parametrize("with_lm", [False, True], ids=["nolm", "lm"])
@pytest.mark.parametrize("K", [1, 16, 128])
def test_sigma_star_is_the_existing_kernel(K, with_lm):
    """The one-state automaton that accepts everything against ops.ctc_beam_search on the same inputs (T = 40, B = 8, the English
    alphabet's 96 columns and classes, ragged lengths with 0 and 1), without and with prune_logp: the same labels, lengths and score
    bits."""
    al, canon = bc.english()
    x = _dev(bd.dense_logits(np.random.default_rng(4000 + K), 40, 8, 96))
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda()
    packed = pack_dense_grammars([Grammar.from_regex(al, ".*")], "cuda")
    assert packed["num_states"] == 1
    lm = bc.char_lm5().to("cuda") if with_lm else None
    alpha, beta = (0.8, 0.6) if with_lm else (0.0, 0.0)
    nbest = min(K, 4)
    for prune in (None, -5.0):
        want = ops.ctc_beam_search(x, SIGMA_LENS, cd, K, nbest, lm, alpha, beta, prune)
        got = ops.ctc_grammar_beam_search(x, SIGMA_LENS, packed, None, cd, K, nbest, lm, alpha, beta, prune)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (K, with_lm, prune)
        assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32)), (K, with_lm, prune,
                                                                                   float((got[2] - want[2]).abs().nan_to_num(0).max()))
        assert bool(torch.isfinite(got[2][0, :, 0]).all()) and int(got[1][1].abs().sum()) == 0


# -------------------------------------------------------------------------------------------------------------- brute force
def test_brute_force_on_the_device():
    """V = 4, T = 6, `1 (2|3)* 1`, K = 128: the beam holds every viable prefix, so the n-best is every accepted labelling in brute
    force's order; its acoustic scores are the labellings' full forward scores (ops.ctc_align), and their logsumexp is the exact
    match probability of ops.ctc_grammar_scores."""
    seeds = list(range(30))
    g = gc.tiny_grammar()
    x = np.stack([gc.tiny_logits(s) for s in seeds], axis=1)
    brute = [gc.tiny_brute(s) for s in seeds]
    nbest = max(len(h) for h in brute)
    assert nbest <= 128 and min(len(h) for h in brute) >= 8
    c = gc.Case("brute", x, [6] * len(seeds), 128, nbest, [g], None, None, None, 0.0, 0.0)
    out = _search(c)
    lab, ln, sc = _host(out)
    err, compared = np.zeros(3), 0
    for b, want in enumerate(brute):
        got = [(list(lab[b, q, :ln[b, q]]), sc[b, q]) for q in range(nbest) if np.isfinite(sc[b, q, 0])]
        assert len(got) == len(want) and all(g.accepts(y) for y, _ in got), b      # every accepted labelling, and nothing else
        assert sorted(y for y, _ in got) == sorted(h[0] for h in want), b
        totals = np.array([h[1] for h in want])
        for q, (gq, h) in enumerate(zip(got, want)):                              # order: up to the first rank brute force leaves open
            if q + 1 < len(want) and totals[q] - totals[q + 1] < gc.TAU:
                break
            assert gq[0] == h[0], (b, q)
            compared += 1
        by = {tuple(h[0]): h for h in want}
        for y, s in got:
            err = np.maximum(err, np.abs(np.asarray(s, dtype=np.float64) - np.asarray(by[tuple(y)][1:])))
    bar = gc.bars("brute")
    print("brute_K128             brute     K 128 V   4 T   6 B %2d  ranks compared %d  max |score - fp64|: total %.2e acoustic %.2e lm "
          "%.2e  bars %.1e %.1e %.1e" % (len(seeds), compared, err[0], err[1], err[2], *bar))
    assert compared >= 8 * len(seeds) * 3 // 4
    assert (err <= np.asarray(bar)).all(), (err, bar)
    _acoustic_is_a_lower_bound("brute", c, out, equal=True)
    logp = ops.ctc_grammar_scores(_dev(x), c.lens, pack_grammars([g], "cuda"), None, False)[0][:, 0].cpu().numpy().astype(np.float64)
    ac = np.where(np.isfinite(sc[..., 0]), sc[..., 1], NEG).astype(np.float64)
    m = ac.max(axis=1)
    lse = m + np.log(np.exp(ac - m[:, None]).sum(axis=1))
    tol = grammar_bound(6, logp, g.max_in_degree, g.n_states + g.n_arcs) + bar[1]    # that suite's bound on logp + this one's on the terms
    assert (np.abs(lse - logp) <= tol).all(), (np.abs(lse - logp).max(), tol.min())


# ------------------------------------------------------------------------------------------------------------- dense logits
@pytest.mark.parametrize("name", gc.DENSE)
def test_dense_logits_against_fp64(name):
    """N(0, 3), T = 24, V = 13, B = 32, `digit digit - digit digit`, K = 1 / 5 / 16 / 128, nbest = min(K, 4), without and with the LM
    and an insertion bonus: labels, lengths and order are the restatement's on every line it decides by TAU, at least 3/4 of them."""
    c, ref = gc.case(name), gc.reference(name)
    out = _search(c)
    gc.compare(name, c, ref, *_host(out))
    _acoustic_is_a_lower_bound(name, c, out)
    assert _bits(out, _search(c)), name                                         # two runs, the same bits


# ------------------------------------------------------------------------------------- per-line automata, bad indices, poison
def test_per_line_automata_bad_indices_and_a_poisoned_row():
    al = gc.field_alphabet()
    grammars = [gc.field_grammar(), Grammar.from_regex(al, r"a\d+"), Grammar.from_regex(al, r"-?\d{3}")]
    grammars.append(grammars[1])                                                # automaton 3: automaton 1's tables, poisoned below
    which = [0, 1, 2, 3, 2, 1, 0, 3, 4, -1, 1 << 20, 0]
    x = bd.dense_logits(np.random.default_rng(4200), 24, len(which), 13)
    c = gc.Case("which", x, [24] * len(which), 16, 4, grammars, which, None, None, 0.0, 0.3)
    tables = [tuple(a.copy() for a in g.dense_tables()) for g in grammars]
    tables[3][0][0, :] = -1                                                     # its start state loses every arc
    packed = pack_dense_grammars(grammars, "cuda")
    s0 = int(packed["state_off"][3])
    packed["next"][s0, :] = -1
    ref = gc.references(c, tables)
    out = _search(c, packed)
    lab, ln, sc = _host(out)
    gc.compare("which", c, ref, lab, ln, sc, floor=6)
    hit = [b for b, w in enumerate(which) if not 0 <= w < 3]
    for b in range(len(which)):
        assert np.isfinite(sc[b, 0, 0]) == (b not in hit), b                    # only the affected lines come back unfilled
    # a distance below zero cannot accept; a next state outside the automaton is no arc: poisons of the other two kinds
    packed = pack_dense_grammars(grammars[:3], "cuda")
    o0, o1, o2 = (int(v) for v in packed["state_off"][:3])
    packed["dist"][o1:o2] = -7
    packed["next"][o2:][packed["next"][o2:] >= 0] = 1 << 28
    c3 = c._replace(which=[0, 1, 2, 0, 1, 2], x=x[:, :6], lens=[24] * 6)
    sc3 = _host(_search(c3, packed))[2]
    assert np.isfinite(sc3[:, 0, 0]).tolist() == [True, False, False, True, False, False]
    assert np.array_equal(sc3[0], sc[0])                                        # a poisoned neighbour changes nothing


# ------------------------------------------------------------------------------------------------ a trie beyond 8192 cells
@pytest.mark.parametrize("name", gc.TRIE)
def test_trie_beyond_the_sweep_kernels(name):
    """About 3000 random words (more states + arcs than vocr_ctc_grammar_scores takes) with the character 5-gram at K = 16: every
    returned string is a word of the list, and the results are the restatement's under the gap rule."""
    c, ref = gc.case(name), gc.reference(name)
    g, words = gc.big_trie()
    assert g.n_states + g.n_arcs > ops.GRAMMAR_CELLS_MAX
    out = _search(c)
    lab, ln, sc = _host(out)
    gc.compare(name, c, ref, lab, ln, sc)
    al, wordset = bc.english()[0], set(words)
    dec = va.GrammarBeamDecoder(al, g, beam=16, nbest=4, lm=c.lm, lm_weight=c.alpha, insertion_bonus=c.beta)
    texts = dec.decode(_dev(c.x), c.lens)
    assert np.isfinite(sc[:, 0, 0]).all() and all(t in wordset for t in texts), texts
    _acoustic_is_a_lower_bound(name, c, out)


# ------------------------------------------------------------------------------------------------------------------ corners
def _corner(name, al, grammars, x, lens, K, nbest, which=None, beta=0.2, floor=1):
    c = gc.Case("corners", x, lens, K, nbest, grammars, which, None, None, 0.0, beta)
    ref = gc.references(c)
    out = _search(c)
    lab, ln, sc = _host(out)
    gc.compare(name, c, ref, lab, ln, sc, floor=floor)
    return c, ref, (lab, ln, sc)


def test_smallest_and_largest_alphabet_at_K128():
    """V = 2 (one symbol) and V = 256 (the full 128 KiB of candidate scores beside the static LDS) at K = 128."""
    al2 = gc.letters(2)
    x = bd.dense_logits(np.random.default_rng(4400), 9, 3, 2)
    _, ref, (lab, ln, sc) = _corner("V2_K128", al2, [Grammar.from_regex(al2, "aa?a?")], x, [9, 4, 1], 128, 4)
    assert [len(r.hyps) for r in ref] == [3, 2, 1] and np.isfinite(sc[..., 0]).sum(axis=1).tolist() == [3, 2, 1]
    al = gc.letters(256)
    x = bd.dense_logits(np.random.default_rng(4401), 6, 3, 256)
    c, ref, (lab, ln, sc) = _corner("V256_K128", al, [Grammar.from_regex(al, "[a-p]{2,4}")], x, [6, 5, 6], 128, 4, floor=2)
    assert c.K * x.shape[2] * 4 == 128 * 1024 and np.isfinite(sc[..., 0]).all() and ((ln >= 2) & (ln <= 4)).all()


def test_corners_of_the_distance_rule():
    al = gc.field_alphabet()
    rng = np.random.default_rng(4402)
    # T = 1: one frame, one symbol
    x = bd.dense_logits(rng, 1, 4, 13)
    _, _, (lab, ln, sc) = _corner("T1", al, [Grammar.from_regex(al, r"\d")], x, [1, 1, 0, 1], 16, 4)
    assert ln[[0, 1, 3], 0].tolist() == [1, 1, 1] and not np.isfinite(sc[2, 0, 0])    # no frames and a start that does not accept
    # the empty string alone: one hypothesis, the all-blank path
    x = bd.dense_logits(rng, 7, 3, 13)
    _, _, (lab, ln, sc) = _corner("empty", al, [Grammar.from_labels(al, [])], x, [7, 0, 3], 16, 4)
    assert np.isfinite(sc[..., 0]).sum(axis=1).tolist() == [1, 1, 1] and (ln == 0).all() and sc[1, 0, 1] == 0.0
    lp0 = gc.bc.br.class_logprobs(x[:, 0])[:, 0].sum()
    assert abs(sc[0, 0, 1] - lp0) <= gc.bars("corners")[1]
    # the minimum length equals the frame count: one symbol per frame, no blank, exactly one path
    chain = [1, 2, 3, 11, 4, 5]
    x = bd.dense_logits(rng, 6, 3, 13)
    _, _, (lab, ln, sc) = _corner("tight", al, [Grammar.from_labels(al, chain)], x, [6, 5, 7], 16, 4)
    assert lab[0, 0].tolist() == chain and np.isfinite(sc[:, 0, 0]).tolist() == [True, False, True] and not np.isfinite(sc[:, 1, 0]).any()
    path = sum(gc.bc.br.class_logprobs(x[:, 0])[t, k] for t, k in enumerate(chain))
    assert abs(sc[0, 0, 1] - path) <= gc.bars("corners")[1]
    # a beam that runs empty mid-line (`1 1 1` needs five frames; four pass the distance test at frame 0) beside one that does not
    x = bd.dense_logits(rng, 5, 3, 13)
    _, ref, (lab, ln, sc) = _corner("runs_empty", al, [Grammar.from_labels(al, [1, 1, 1])], x, [4, 5, 3], 16, 4)
    assert np.isfinite(sc[:, 0, 0]).tolist() == [False, True, False] and lab[1, 0, :3].tolist() == [1, 1, 1]


# -------------------------------------------------------------------------------------------------------------- the surface
def test_decoder_surface():
    al = gc.field_alphabet()
    g0, g1 = gc.field_grammar(), Grammar.from_regex(al, r"a\d+")
    x = _dev(bd.dense_logits(np.random.default_rng(4500), 24, 4, 13))
    lens, which = [24, 24, 3, 20], [0, 1, 0, 1]
    dec = va.GrammarBeamDecoder(al, [g0, g1], beam=16, nbest=4, lm=gc.field_lm(), lm_weight=0.5, insertion_bonus=0.3)
    texts = dec.decode(x, lens, which=which)
    assert g0.accepts(texts[0]) and g1.accepts(texts[1]) and texts[2] == "" and g1.accepts(texts[3])
    assert dec.decode(x, lens, uxxxx=True, which=which)[0].split(" ")[2] == "u002d"
    lists = dec.decode_nbest(x, lens, which=which)
    assert [len(l) for l in lists] == [4, 4, 0, 4]
    for b, lst in enumerate(lists):
        assert all((g0, g1)[which[b]].accepts(y) for y, _ in lst) and [s[0] for _, s in lst] == sorted((s[0] for _, s in lst), reverse=True)
    hyps, aligned = dec.decode_aligned(x, lens, which=which)
    assert hyps == texts and aligned[2] is None and all(aligned[b] is not None for b in (0, 1, 3))
    hyps, nb = dec.decode_aligned(x, lens, nbest=2, which=which)
    assert hyps == texts and [len(l) for l in nb] == [2, 2, 0, 2]
    hyps, alts = dec.decode_alternatives(x, lens, topk=2, which=which)
    assert hyps == texts and alts[2] is None and alts[0] is not None
    assert dec.decode(x, lens) == [dec.decode(x, lens, which=[0] * 4)[b] for b in range(4)]      # None: grammar 0 for every line
    one = va.GrammarBeamDecoder(al, g0)                                         # a single Grammar, the defaults
    assert all(g0.accepts(t) for t in one.decode(x, [24] * 4))
    with pytest.raises(ValueError, match="which"):
        dec.decode(x, lens, which=[0, 1, 2, 0])
    with pytest.raises(RuntimeError, match="dense tables"):
        ops.ctc_grammar_beam_search(x, lens, pack_dense_grammars([Grammar.from_regex(bc.english()[0], "a")], "cuda"))


def test_minimum_error_rate_training_under_a_grammar():
    """MinErrorRateLoss(decoder=GrammarBeamDecoder(...)): one forward and backward at T = 24, B = 4; the list is the accepted n-best."""
    al = gc.field_alphabet()
    dec = va.GrammarBeamDecoder(al, gc.field_grammar(), beam=16)
    crit = va.MinErrorRateLoss(al, decoder=dec, nbest=4, ctc_weight=0.0)
    x = _dev(bd.dense_logits(np.random.default_rng(4501), 24, 4, 13)).requires_grad_(True)
    refs = [[1, 2, 11, 3, 4], [5, 5, 11, 6, 7], [9, 8, 11, 7, 7], [2, 3, 11, 4, 10]]
    targets = torch.tensor([v for r in refs for v in r], dtype=torch.int32)
    loss = crit(x, targets, torch.tensor([24] * 4, dtype=torch.int32), torch.tensor([5] * 4, dtype=torch.int32))
    loss.backward()
    assert np.isfinite(loss.detach().item()) and loss.detach().item() > 0.0
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0.0
