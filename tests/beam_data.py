"""Synthetic inputs of the beam-search tests: peaky logits (one dominant class per frame, mostly blank, at most one competitor per
frame, every other class impossible), dense logits (every column finite, as an untrained model gives), dense logits with bitwise
duplicated columns (exact score ties) and a character 5-gram ARPA file written from random text.  Test helper only."""
import math
from collections import Counter

import numpy as np


def peaky_logits(rng, T, B, V, classes=None, p_char=0.35, p_alt=0.5, cost=(2.0, 40.0)):
    """[T, B, V] float32.  Each frame: a dominant class (a character with probability p_char, blank otherwise, runs of 1-3 frames),
    and with probability p_alt one competitor whose logit is `cost` below it; all other logits -inf.  Sparse competitors keep the
    candidates near every beam cut well apart, so an fp32 search and an fp64 restatement take the same decisions."""
    classes = np.arange(1, V) if classes is None else np.asarray(classes)
    allc = np.concatenate([[0], classes])
    x = np.full((T, B, V), -np.inf, dtype=np.float32)
    for b in range(B):
        t = 0
        while t < T:
            c = int(rng.choice(classes)) if rng.random() < p_char else 0
            for _ in range(int(rng.integers(1, 4))):
                if t >= T:
                    break
                x[t, b, c] = rng.normal(0.0, 1.0)
                if rng.random() < p_alt:
                    a = int(rng.choice(allc[allc != c]))
                    x[t, b, a] = x[t, b, c] - rng.uniform(*cost)
                t += 1
    return x


def dense_logits(rng, T, B, V, sigma=3.0):
    """[T, B, V] float32, every entry N(0, sigma): all K*V candidates of a frame are finite, so the selection cuts a large live set.
    sigma = 3 keeps most lines decided (the restatement's smallest gap above the tests' TAU); sigma = 1 is too flat for that."""
    return rng.normal(0.0, sigma, size=(T, B, V)).astype(np.float32)


def tie_logits(rng, T, B, V, sigma, pairs):
    """dense_logits with column dst a bitwise copy of column src for every (dst, src) of `pairs` (columns of different classes):
    prefixes that differ only by swapping src and dst score exactly alike, in fp32 as in fp64, so cuts and final ranks fall inside
    exact ties and the slot id decides them."""
    x = dense_logits(rng, T, B, V, sigma)
    for dst, src in pairs:
        x[:, :, dst] = x[:, :, src]
    return x


def write_char_arpa(path, units, order=5, lines=400, seed=0, min_count=2):
    """A character n-gram ARPA file over `units` (uxxxx strings) estimated from random Markov text: relative frequencies with a
    fixed discount, random backoff weights, n-grams seen fewer than `min_count` times dropped (their prefixes stay listed)."""
    rng = np.random.default_rng(seed)
    U = len(units)
    trans = rng.dirichlet(np.full(U, 0.3), size=U)
    counts = [Counter() for _ in range(order + 1)]
    for _ in range(lines):
        n = int(rng.integers(5, 40))
        seq = ["<s>"]
        cur = int(rng.integers(U))
        for _ in range(n):
            seq.append(units[cur])
            cur = int(rng.choice(U, p=trans[cur]))
        seq.append("</s>")
        for k in range(1, order + 1):
            for i in range(len(seq) - k + 1):
                counts[k][tuple(seq[i:i + k])] += 1
    grams = {1: {}}
    total = sum(c for g, c in counts[1].items() if g != ("<s>",))
    for g, c in counts[1].items():
        grams[1][g] = -99.0 if g == ("<s>",) else math.log10(0.9 * c / total)
    grams[1][("<unk>",)] = math.log10(0.01)
    for k in range(2, order + 1):
        grams[k] = {}
        for g, c in counts[k].items():
            if c >= min_count and g[:-1] in grams[k - 1]:
                grams[k][g] = math.log10(0.8 * c / counts[k - 1][g[:-1]])
    with open(path, "w") as fh:
        fh.write("\\data\\\n")
        for k in range(1, order + 1):
            fh.write("ngram %d=%d\n" % (k, len(grams[k])))
        for k in range(1, order + 1):
            fh.write("\n\\%d-grams:\n" % k)
            for g in sorted(grams[k]):
                bo = "" if k == order or g[-1] == "</s>" else " %.4f" % -rng.uniform(0.0, 0.6)
                fh.write("%.4f %s%s\n" % (grams[k][g], " ".join(g), bo))
        fh.write("\n\\end\\\n")
    return path
