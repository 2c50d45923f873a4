"""Synthetic inputs of the word beam-search tests, all from a seeded generator: a Zipf-weighted lexicon of random letter-words over the
English alphabet, a word 3-gram ARPA in the reference's token format (form_tokenized_words: letters joined by "_", punctuation and
digits tokens of their own) estimated from random sentences, and "sentence-peaky" logits: a CTC rendering of such sentences with
blank runs and sparse competitors, some of which win a frame and turn a word into an out-of-vocabulary typo.  Test helper only."""
import math
from collections import Counter

import numpy as np

from vistaocr_amd.textutils import form_tokenized_words

LETTERS = ["u%04x" % c for c in range(0x61, 0x7b)]
PUNCT = ["u002e", "u002c", "u003b", "u0021"]
DIGITS = ["u%04x" % c for c in range(0x30, 0x3a)]
SPACE = "u0020"


def make_lexicon(rng, n_words, min_len=2, max_len=8):
    """n_words distinct random letter-words (tuples of uxxxx units) and their Zipf weights (rank r: 1 / r^1.1, normalised)."""
    words, seen = [], set()
    while len(words) < n_words:
        n = int(rng.integers(min_len, max_len + 1))
        w = tuple(LETTERS[i] for i in rng.integers(0, len(LETTERS), size=n))
        if w not in seen:
            seen.add(w)
            words.append(w)
    p = 1.0 / np.arange(1, n_words + 1) ** 1.1
    return words, p / p.sum()


def make_sentences(rng, words, weights, n, min_words=3, max_words=9, n_succ=4):
    """n random sentences as uxxxx character lists.  Words follow a bigram chain (each word has n_succ favourite successors, taken
    half of the time, the Zipf unigram otherwise); a word is followed by punctuation with probability 0.15, and a number (1-3 digits)
    stands in for a word with probability 0.08."""
    W = len(words)
    succ = rng.integers(0, W, size=(W, n_succ))
    cdf = np.cumsum(weights)

    def zipf():
        return min(int(np.searchsorted(cdf, rng.random() * cdf[-1], side="right")), W - 1)

    out = []
    for _ in range(n):
        chars = []
        cur = zipf()
        for i in range(int(rng.integers(min_words, max_words + 1))):
            if i:
                chars.append(SPACE)
            if rng.random() < 0.08:
                chars.extend(DIGITS[d] for d in rng.integers(0, 10, size=int(rng.integers(1, 4))))
            else:
                chars.extend(words[cur])
            if rng.random() < 0.15:
                chars.append(PUNCT[int(rng.integers(len(PUNCT)))])
            cur = int(succ[cur, rng.integers(n_succ)]) if rng.random() < 0.5 else zipf()
        out.append(chars)
    return out


def write_word_arpa(path, words, weights, sentences, order=3, seed=0, min_count=2, unk=True, extra=()):
    """A word n-gram ARPA file in the reference's token format, estimated from `sentences` (uxxxx character lists, tokenised by
    form_tokenized_words): every lexicon word a 1-gram (count + its Zipf weight as a prior), punctuation and digits as seen, relative
    frequencies with a fixed discount for orders > 1 (n-grams seen fewer than `min_count` times dropped, their prefixes listed), random
    backoff weights.  `extra`: (token, log10 p) 1-grams added as they are (tokens the search can never produce)."""
    rng = np.random.default_rng(seed)
    counts = [Counter() for _ in range(order + 1)]
    for chars in sentences:
        seq = ["<s>"] + form_tokenized_words(chars) + ["</s>"]
        for k in range(1, order + 1):
            for i in range(len(seq) - k + 1):
                counts[k][tuple(seq[i:i + k])] += 1
    prior = {"_".join(w): p for w, p in zip(words, weights)}
    uni = Counter({g[0]: c for g, c in counts[1].items() if g != ("<s>",)})
    total = sum(uni.values())
    mass = {t: uni.get(t, 0) / total + prior.get(t, 0.0) for t in set(uni) | set(prior)}
    z = sum(mass.values())
    grams = {1: {(t,): math.log10(0.9 * m / z) for t, m in mass.items()}}
    grams[1][("<s>",)] = -99.0
    if unk:
        grams[1][("<unk>",)] = math.log10(0.005)
    for t, lp in extra:
        grams[1][(t,)] = lp
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


def sentence_logits(rng, sentences, alphabet, T, p_alt=0.4, p_typo=0.06, cost=(2.0, 40.0)):
    """[T, B, V] float32 CTC renderings of the sentences (one per line, cut at T frames, blank after the end) and the line lengths.
    Each character takes 1-2 frames and is followed by 1-3 blank frames, dominant raw logits near 4 (above the greedy decode's
    threshold); with probability p_alt a frame has one competitor `cost` below its dominant class, all other logits -inf.  With probability p_typo a letter's frames are won by another letter (0.3-1.5 above the true
    one): the greedy decode then writes a word that is usually not in the lexicon."""
    V = len(alphabet)
    idx = {alphabet.idx_to_char[c]: c for c in range(V - 1, 0, -1)}
    letters = np.array([idx[u] for u in LETTERS])
    allc = np.arange(V)
    B = len(sentences)
    x = np.full((T, B, V), -np.inf, dtype=np.float32)
    lens = []
    for b, chars in enumerate(sentences):
        t = 0
        for u in chars:
            c = idx[u]
            typo = u in LETTERS and rng.random() < p_typo
            alt = int(rng.choice(letters[letters != c])) if typo else -1
            for _ in range(int(rng.integers(1, 3))):
                if t >= T:
                    break
                x[t, b, c] = rng.normal(4.0, 1.0)
                if typo:
                    x[t, b, alt] = x[t, b, c] + rng.uniform(0.3, 1.5)
                elif rng.random() < p_alt:
                    a = int(rng.choice(allc[allc != c]))
                    x[t, b, a] = x[t, b, c] - rng.uniform(*cost)
                t += 1
            for _ in range(int(rng.integers(1, 4))):
                if t >= T:
                    break
                x[t, b, 0] = rng.normal(4.0, 1.0)
                if rng.random() < p_alt:
                    a = int(rng.choice(allc[1:]))
                    x[t, b, a] = x[t, b, 0] - rng.uniform(*cost)
                t += 1
        while t < T:
            x[t, b, 0] = 4.0
            t += 1
        lens.append(T)
    return x, lens
