"""GPU: vocr_ctc_beam_search (vistaocr_amd/csrc/ctc_beam.hip, ctc_beam_common.h) against the fp64 restatement (tests/beam_ref.py) where
the peaky inputs of tests/test_beam_gpu.py never take it: dense logits (every K*V candidate finite: the radix select cuts thousands
of live scores under a non-trivial prefix / mask), K that is no power of two, nbest = K, pruning, ragged lengths, both alphabets,
every intermediate beam of a line, exact ties at the cut and among the final ranks (bitwise-duplicated columns), prefixes that
leave the beam and come back under a new node id (find_merge's chain walk), and the largest and smallest launches (K = 128 with
V = 256: the full 128 KiB of dynamic LDS; take_all on every frame; V = 2; V = 1).

The inputs, their floors and the score bars are pinned in tests/beam_cases.py and checked without a GPU by tests/test_beam_cpu.py.
A line is compared only where every decision of the restatement won by at least TAU; labels, lengths and rank order must then be
identical.  Run with -s, every case prints how many lines it compared and the largest |score - fp64| it saw
(profiles/beam_fp64_errors.txt)."""
import numpy as np
import pytest
import torch

from tests import beam_cases as bc
from tests import beam_ref as br
from vistaocr_amd import ops

pytestmark = pytest.mark.gpu


def _run(x, lens, K, nbest, canon=None, lm=None, alpha=0.0, beta=0.0, prune=None):
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda() if canon is not None else None
    lab, ln, sc = ops.ctc_beam_search(xd, lens, cd, K, nbest, lm.to("cuda") if lm is not None else None, alpha, beta, prune)
    torch.cuda.synchronize()
    return lab.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()


def _check(name):
    case, ref = bc.char_case(name), bc.char_reference(name)
    bc.check_pinned(name, case, ref)
    out = _run(case.x, case.lens, case.K, case.nbest, canon=case.canon, lm=case.lm, alpha=case.alpha, beta=case.beta, prune=case.prune)
    bc.compare(name, case, ref, *out)
    return case, ref, out


@pytest.mark.parametrize("name", bc.CHAR_DENSE)
def test_dense_logits_against_fp64(name):
    """N(0, 3) logits over the English alphabet, K in {1, 5, 16, 64, 100, 128}, without an LM and with the character 5-gram: at least
    K*V/2 candidates are finite on every compared line."""
    case, _, _ = _check(name)
    assert case.dense


@pytest.mark.parametrize("name", bc.CHAR_VARIANTS)
def test_dense_variants_against_fp64(name):
    """nbest = K on a full beam, prune_logp = -3 and -6, the Arabic alphabet (V = 166), ragged lengths in one batch, B = 1, B = 65."""
    case, ref, (lab, ln, sc) = _check(name)
    if name == "ragged_K16_lm":
        T = case.x.shape[0]
        for b, L in enumerate(case.lens):
            assert (ln[b] <= min(L, T)).all()
        b = case.lens.index(0)                                           # no frames: the empty labelling with P = 1, and nothing else
        assert ln[b, 0] == 0 and sc[b, 0, 1] == 0.0 and abs(sc[b, 0, 2] - case.lm.eos[case.lm.start]) < 1e-5
        assert not np.isfinite(sc[b, 1:, 0]).any() and (ln[b, 1:] == 0).all()
        over, full = case.lens.index(T + 9), case.lens.index(T)          # a length above T is T (the two lines share no logits,
        assert len(ref[over].hyps) == len(ref[full].hyps) == case.nbest  # so only the shape of the answer is compared)
    if name == "K16_nbest16_lm":
        assert np.isfinite(sc[..., 0]).all()                             # a full beam: every one of the K ranks is listed


def test_largest_launch_against_fp64():
    """K = 128, V = 256: 128 KiB of dynamic LDS next to the static 20 KiB, 32640 live candidates per frame."""
    case, ref, _ = _check("big_K128_V256")
    assert case.K * case.x.shape[2] * 4 == 128 * 1024 and case.dense


@pytest.mark.parametrize("name", bc.CHAR_INTERMEDIATE)
def test_every_intermediate_beam(name):
    """One launch whose lines are the same dense logits with lens = 1..T and nbest = K: rank for rank, line b is the complete beam
    after frame b.  The lines are compared in order, so a divergence names its first frame."""
    case, ref, _ = _check(name)
    assert len(bc.decided(case, ref)) == case.x.shape[0]                 # every frame's beam is decided (checked on the CPU too)


@pytest.mark.parametrize("name", bc.CHAR_TIES)
def test_ties_at_the_cut_and_in_the_final_ranks(name):
    """Bitwise-duplicated columns of different classes: the K-th score is shared (top_k's id passes and the i <= id_cut cut) and
    neighbouring final ranks are equal (rank_final's rank at the last frame); the order is the restatement's (score desc, id asc)."""
    case, ref, _ = _check(name)
    assert case.exact_ties and bc.total(case, ref, "kth_ties") > 0 and bc.total(case, ref, "final_ties") > 0


@pytest.mark.parametrize("name", bc.CHAR_COMEBACK)
def test_prefix_that_comes_back(name):
    """Every line has a merge into a parent prefix that left the beam and returned under a new node id while the child stayed."""
    case, ref, _ = _check(name)
    assert all(r.stats["remerges"] > 0 for r in ref) and len(bc.decided(case, ref)) == len(ref)


def test_hand_built_come_back():
    """bc.HAND_PROBS: "a" is cut after frame 1 while its child "ab" stays, returns from "" at frame 2, and a + b merges into ab at
    frame 3 across two node ids.  The beam is the brute force over the alignments the written-down beams can still see."""
    x = bc.hand_logits()
    K = bc.HAND_K
    for t, kept in enumerate(bc.HAND_KEPT):
        lab, ln, sc = _run(x, [t + 1], K, K)
        assert {tuple(lab[0, q, :ln[0, q]]) for q in range(K) if np.isfinite(sc[0, q, 0])} == kept, t
    want = sorted(bc.kept_path_scores(br.class_logprobs(x[:, 0]), bc.HAND_KEPT).items(), key=lambda kv: -kv[1])[:K]
    lab, ln, sc = _run(x, [4], K, K)
    assert [tuple(lab[0, q, :ln[0, q]]) for q in range(K)] == [w[0] for w in want]
    assert np.allclose(sc[0, :, 1], [w[1] for w in want], rtol=0, atol=1e-5)
    p_ab = np.exp(sc[0, [w[0] for w in want].index((1, 2)), 1])
    assert p_ab < np.exp(br.ctc_logprob(br.class_logprobs(x[:, 0]), [1, 2])) - 1e-3      # the cut did lose mass of "ab"


def _exact(x, K, classes_used, beta=0.2):
    """The search holds every prefix: its output is the brute force, in order, with its scores."""
    brute = br.brute_force(x, classes_used, beta=beta)
    totals = np.array([h[1] for h in brute])
    assert len(brute) < 2 or np.min(totals[:-1] - totals[1:]) > 1e-4                     # the fixed seed has no near ties
    nbest = min(len(brute), K)
    lab, ln, sc = _run(x[:, None, :], [x.shape[0]], K, nbest, beta=beta)
    got = [(list(lab[0, q, :ln[0, q]]), sc[0, q]) for q in range(nbest) if np.isfinite(sc[0, q, 0])]
    assert [g[0] for g in got] == [h[0] for h in brute[:nbest]]
    for (_, gsc), (_, btot, bac, _) in zip(got, brute):
        assert abs(gsc[1] - bac) <= 1e-5 * abs(bac) + 1e-6 and abs(gsc[0] - btot) <= 1e-5 * abs(btot) + 1e-5 and gsc[2] == 0.0
    return brute


def test_take_all_on_every_frame():
    """K = 128, V = 3, T = 3: at most 1 + 2 + 4 prefixes before the last frame, so fewer finite candidates than K in every frame
    (top_k's take_all path throughout) and the output is the brute force's 9 labellings."""
    x = np.random.default_rng(5).normal(0, 1.5, size=(3, 3))
    ref_stats = {}
    br.beam_search(x, 3, 128, stats=ref_stats)
    assert ref_stats["max_live"] < 128
    assert len(_exact(x, 128, [1, 2])) == 9


def test_smallest_alphabets():
    """V = 2: one symbol; K = 4 holds all of "", a, a a, a a a.  V = 1: only the blank, so only the empty labelling, with ln 1 = 0
    exactly, and every further rank empty."""
    x = np.random.default_rng(6).normal(0, 1.5, size=(5, 2))
    assert len(_exact(x, 4, [1])) == 4
    ref, gap = br.beam_search(x, 5, 2, nbest=2, beta=0.2)
    assert gap > 1e-2
    lab, ln, sc = _run(x[:, None, :], [5], 2, 2, beta=0.2)
    assert [list(lab[0, q, :ln[0, q]]) for q in range(2)] == [h[0] for h in ref]
    assert np.allclose(sc[0, :, :2], [h[1:3] for h in ref], rtol=0, atol=1e-5)
    x1 = np.random.default_rng(7).normal(0, 3, size=(6, 3, 1))
    lab, ln, sc = _run(x1, [6, 0, 3], 3, 2, beta=0.7)
    assert (ln == 0).all() and (lab == 0).all()
    assert (sc[:, 0] == 0.0).all()                                                       # total, acoustic, lm: all exactly 0
    assert np.isneginf(sc[:, 1, :2]).all() and (sc[:, 1, 2] == 0.0).all()
