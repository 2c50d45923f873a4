"""The cases tests/test_nbest_cpu.py (bars, mutants) and tests/test_nbest_gpu.py (the kernels) share: small batches of lines, each with
an n-best list made of a base labelling and random one-edit neighbours of it, plus the hypotheses a search can hand over that have no
score.  Data only; nothing here comes from the code under test.

The sizes are the smallest at which vocr_ctc_nbest_grad can still go wrong: the lattice kernel keeps a labelling of up to 31 labels
(S = 63) in registers and prefetches PF = 8 frames, beyond that it stages TB = 8 frames in LDS; the gradient kernel works on tiles of
TT = 16 frames and splits the hypotheses into QG = 4 groups (n = 1, 3: groups left empty; n = 128: 32 per group)."""
import numpy as np
import torch

from tests import ctc_ref as cr
from tests.beam_data import dense_logits

NEG = float("-inf")
PEAKY, DENSE = ("peaky", 8.0, 1.0), ("beam_dense", 3.0)
CANON9 = [0, 1, 1, 3, 4, 4, 4, 7, 8]          # classes of 2 ({1, 2}) and 3 ({4, 5, 6}) members; V >= 9

# name, T, B, V, n, longest labelling per line, kinds, lens ("full" or a list), regime, canon (None / "c9"), weights, specials
CASES = [
    ("seam31", 80, 3, 40, 3, [31, 12, 0], "random", [80, 70, 33], PEAKY, None, "mixed", ()),
    ("seam32", 80, 3, 40, 3, [32, 31, 5], "random", [80, 65, 64], PEAKY, None, "sum0", ()),
    ("seam33", 80, 4, 40, 3, [33, 32, 31, 33], "random", [80, 65, 66, 64], PEAKY, None, "pos", ()),
    ("seam33_dense", 80, 2, 40, 3, [33, 20], "random", [80, 66], DENSE, None, "mixed", ()),
    ("long_peaky", 294, 2, 96, 3, [100, 97], "random", [294, 250], PEAKY, None, "mixed", ("dup",)),
    ("long_dense", 294, 2, 96, 2, [100, 40], "random", [294, 111], DENSE, None, "sum0", ()),
    ("T1", 1, 4, 7, 3, [1, 0, 1, 1], "random", [1, 1, 1, 0], DENSE, None, "mixed", ("bad",)),
    # lens 0, 1, around PF = 8 and around TT = 16 in one batch
    ("T15", 15, 4, 12, 3, [4, 3, 2, 1], "random", [15, 8, 9, 10], PEAKY, None, "mixed", ()),
    ("T16", 16, 5, 12, 3, [4, 3, 2, 1, 2], "random", [16, 7, 1, 0, 15], PEAKY, None, "pos", ("nofit",)),
    ("T17", 17, 4, 12, 3, [5, 3, 2, 1], "random", [17, 16, 9, 1], DENSE, None, "sum0", ("unfilled",)),
    ("T33", 33, 3, 12, 3, [6, 6, 3], "random", [33, 32, 31], PEAKY, None, "mixed", ()),
    ("V2", 24, 3, 2, 3, [5, 1, 0], "equal", [24, 17, 9], DENSE, None, "mixed", ()),
    ("V5", 20, 2, 5, 3, [4, 6], ["abab", "random"], "full", DENSE, None, "sum0", ("dup",)),
    ("V96_n1", 40, 3, 96, 1, [10, 7, 0], "random", [40, 33, 8], PEAKY, None, "neg1", ()),
    ("V166", 30, 2, 166, 3, [8, 5], "random", "full", PEAKY, None, "mixed", ()),
    ("V256", 20, 2, 256, 3, [6, 4], "random", [20, 13], DENSE, None, "pos", ("bad",)),
    ("n128", 20, 2, 20, 128, [5, 4], "random", [20, 18], DENSE, None, "mixed", ("dup", "unfilled", "nofit", "bad")),
    ("patterns", 70, 4, 30, 3, [20, 31, 33, 34], ["equal", "abab", "equal", "abab"], [70, 70, 70, 69], PEAKY, None, "mixed", ()),
    ("tight", 50, 4, 20, 3, [5, 31, 33, 12], "random", "tight", DENSE, None, "neg1", ()),
    ("classes", 40, 3, 12, 4, [8, 6, 3], "random", [40, 31, 17], PEAKY, "c9", "mixed", ("dup", "bad_class")),
    ("classes_dense", 18, 2, 9, 3, [4, 3], "random", "full", DENSE, "c9", "sum0", ("neginf_member",)),
    ("classes_seam", 80, 2, 12, 3, [33, 31], "random", [80, 70], PEAKY, "c9", "pos", ("neginf_member",)),
    ("dead_frame", 20, 3, 10, 3, [4, 3, 2], "random", "full", DENSE, None, "mixed", ("dead_frame",)),
    ("zero_weights", 20, 2, 10, 3, [4, 3], "random", [20, 11], DENSE, None, "zero", ("dup",)),
    ("specials", 30, 3, 15, 6, [6, 5, 4], "random", [30, 12, 5], PEAKY, None, "mixed", ("dup", "unfilled", "nofit", "bad")),
]
MUTANT_CASES = ("classes", "classes_dense", "specials", "V5", "T16")


def _edit(rng, lab, allowed):
    """one random substitution, deletion or insertion"""
    lab = list(lab)
    kind = int(rng.integers(3)) if lab else 2
    c = int(allowed[rng.integers(len(allowed))])
    if kind == 0:
        lab[int(rng.integers(len(lab)))] = c
    elif kind == 1:
        del lab[int(rng.integers(len(lab)))]
    else:
        lab.insert(int(rng.integers(len(lab) + 1)), c)
    return lab


def build_case(name, seed=0):
    """dict(x fp32 [T,B,V], lens, hyps[b][q] (label list or None), canon (list or None), w float64 [B,n], M = the label width to pass)"""
    spec = [c for c in CASES if c[0] == name][0]
    _, T, B, V, n, ls, kinds, lens, regime, canon, wkind, specials = spec
    rng = np.random.default_rng([seed, [c[0] for c in CASES].index(name)])
    kinds = [kinds] * B if isinstance(kinds, str) else kinds
    canon = CANON9 + list(range(9, V)) if canon == "c9" else None
    allowed = [v for v in range(1, V) if canon is None or canon[v] != 0]
    base = []
    for b in range(B):
        lab = cr.make_labels(rng, V, ls[b], kinds[b])
        if canon is not None:                                 # any member index stands for its class: keep what make_labels drew
            lab = [v if canon[v] != 0 else allowed[0] for v in lab]
        base.append(lab)
    if lens == "full":
        lens = [T] * B
    elif lens == "tight":                                     # one feasible path for the base labelling
        lens = [cr.need(l) for l in base]
    lens = [int(v) for v in lens]
    assert max(lens) <= T
    if regime[0] == "beam_dense":
        x = torch.from_numpy(dense_logits(rng, T, B, V, regime[1]))
    else:
        fit = [l if cr.need(l) <= lens[b] else [] for b, l in enumerate(base)]
        x = cr.build_logits(rng, T, B, V, fit, lens, regime)
    hyps = []
    for b in range(B):
        row = [base[b]]
        while len(row) < n:
            h = _edit(rng, base[b], allowed)
            row.append(h if len(h) <= ls[b] or len(h) <= max(ls) else base[b])
        hyps.append(row)
    M = max(max(len(h) for h in row) for row in hyps)
    for sp in specials:
        b = 0
        if sp == "dup":
            hyps[0][n - 1] = list(hyps[0][0])
        elif sp == "unfilled" and n > 1:
            hyps[b][1] = None
        elif sp == "nofit":                                   # one repeated label: k of them take 2k - 1 frames, more than the line has
            b = min((v, i) for i, v in enumerate(lens) if v > 0)[1]
            k = lens[b] // 2 + 2
            assert k <= T and 2 * k - 1 > lens[b]
            hyps[b][min(2, n - 1)] = [allowed[0]] * k
            M = max(M, k)
        elif sp == "bad":                                     # a label outside (0, V)
            hyps[min(1, B - 1)][0] = [V] + list(base[min(1, B - 1)][1:]) if base[min(1, B - 1)] else [0]
            if n > 2:
                hyps[0][2] = [0]
        elif sp == "bad_class":                               # no column here is in the blank's class except 0 itself
            hyps[min(1, B - 1)][n - 1] = [0, allowed[0]]
        elif sp == "neginf_member":                           # one member of the 3-class at -inf everywhere, one of the 2-class on a line
            x[:, :, 5] = NEG
            x[:, 0, 2] = NEG
        elif sp == "dead_frame":
            x[3, 0, :] = NEG                                  # a whole frame inside line 0: every hypothesis of it scores -inf
            x[lens[1] - 1, 1, 1:] = NEG                       # the last frame of line 1 allows the blank only
    if wkind == "zero":
        w = np.zeros((B, n))
    elif wkind == "neg1":
        w = -np.ones((B, n))
    else:
        w = rng.normal(0, 1, (B, n))
        if wkind == "sum0":
            w = w - w.mean(1, keepdims=True)
        elif wkind == "pos":
            w = np.abs(w) + 0.1
    w = w.astype(np.float32).astype(np.float64)
    return dict(name=name, x=x, lens=lens, hyps=hyps, canon=canon, w=w, M=max(M, 1), T=T, B=B, V=V, n=n)
