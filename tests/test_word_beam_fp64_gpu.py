"""GPU: vocr_ctc_word_beam_search (vistaocr_amd/csrc/ctc_word_beam.hip, ctc_beam_common.h) against the fp64 restatement
(tests/word_beam_ref.py) where the sentence logits of tests/test_word_beam_gpu.py never take it: dense logits with a closed and an
open vocabulary (K in {5, 16, 64, 128}, the 400-word 3-gram), K = 128 with V = 256, exact ties between two OOV beams with the LM on,
and, with no reference at all, bit-for-bit agreement with the character search on its dense, tie and come-back inputs, which puts the
shared top_k / find_merge through this kernel's larger per-beam state.

The inputs, their floors and the score bars are pinned in tests/beam_cases.py and checked without a GPU by
tests/test_word_beam_cpu.py.  Run with -s, every case prints how many lines it compared and the largest |score - fp64| it saw
(profiles/beam_fp64_errors.txt)."""
import numpy as np
import pytest
import torch

from tests import beam_cases as bc
from vistaocr_amd import ops

pytestmark = pytest.mark.gpu


def _run(x, lens, K, nbest, lm, canon=None, alpha=0.8, beta=0.0, oov=None):
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    cd = torch.as_tensor(canon, dtype=torch.int32).cuda() if canon is not None else None
    lab, ln, sc = ops.ctc_word_beam_search(xd, lens, cd, lm.to("cuda"), K, nbest, alpha, beta, oov)
    torch.cuda.synchronize()
    return lab.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()


def _check(name):
    case, ref = bc.word_case(name), bc.word_reference(name)
    bc.check_pinned(name, case, ref)
    out = _run(case.x, case.lens, case.K, case.nbest, case.lm, canon=case.canon, alpha=case.alpha, beta=case.beta, oov=case.oov)
    bc.compare(name, case, ref, *out)
    return case, ref, out


@pytest.mark.parametrize("name", bc.WORD_DENSE)
def test_dense_logits_against_fp64(name):
    """N(0, 3) logits over the English alphabet, the 400-word 3-gram at lm_weight 0.8, word_bonus 1.  With a closed vocabulary some
    lines legitimately output nothing: they are compared too, an empty rank list is empty on both sides."""
    case, ref, (lab, ln, sc) = _check(name)
    for b in bc.decided(case, ref):
        assert int(np.isfinite(sc[b, :, 0]).sum()) == len(ref[b].hyps)
        if not ref[b].hyps:
            assert (ln[b] == 0).all() and (lab[b] == 0).all()


def test_largest_launch_against_fp64():
    """K = 128, V = 256 with an open vocabulary (the tiny lexicon in a 256-column alphabet): 128 KiB of dynamic LDS next to this
    kernel's 27 KiB static."""
    case, ref, _ = _check("w_big_K128_V256")
    assert case.K * case.x.shape[2] * 4 == 128 * 1024 and case.dense


def test_ties_with_the_lm_on():
    """The letters d and e start no lexicon word and share one column bit for bit: the two beams enter the OOV state with the same
    look-ahead and close score, so the cut and the final ranks fall inside exact ties that the slot id decides."""
    case, ref, _ = _check("w_tie_lm_K6")
    assert case.exact_ties and bc.total(case, ref, "kth_ties") > 0 and bc.total(case, ref, "final_ties") > 0


EQUIVALENT = ["K5", "K16", "K64", "K100", "K128", "arabic_K16", "ragged_K16_lm", "B65_K16", "big_K128_V256", "inter_K5", "tie_K4",
              "tie_K7", "tie_K16", "tie_K64", "tie_english_K16"] + bc.CHAR_COMEBACK


@pytest.mark.parametrize("name", EQUIVALENT)
def test_equivalence_with_character_search(name):
    """tests/test_word_beam_gpu.py's equivalence on the dense, tie and come-back inputs of the character search: with lm_weight =
    word_bonus = oov_penalty = 0 every candidate of the character search exists here with the same score, so labels, lengths and
    acoustic scores are the character search's bit for bit, whatever either of them computes."""
    case = bc.char_case(name)
    V = case.x.shape[2]
    lm = bc.word_lm400() if V == 96 else bc.tiny_word_lm("v256") if V == 256 else bc.tiny_word_lm(V)
    xd = torch.from_numpy(case.x).cuda()
    cd = torch.as_tensor(case.canon, dtype=torch.int32).cuda() if case.canon is not None else None
    a = [t.cpu().numpy() for t in ops.ctc_beam_search(xd, case.lens, cd, case.K, case.nbest)]
    w = [t.cpu().numpy() for t in ops.ctc_word_beam_search(xd, case.lens, cd, lm.to("cuda"), case.K, case.nbest, 0.0, 0.0, 0.0)]
    assert np.isfinite(a[2][..., 1]).any()
    assert a[0].tobytes() == w[0].tobytes() and a[1].tobytes() == w[1].tobytes()
    assert a[2][..., 1].tobytes() == w[2][..., 1].tobytes()
