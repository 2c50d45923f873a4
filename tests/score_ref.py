"""Reference for vocr_edit_stats (tests only): the cell-by-cell Levenshtein DP with the trace rule of the reference's
src/edit_dist_trace.py, over characters and over form_tokenized_words tokens, and a numpy anti-diagonal form of the same for pairs
that are too long for a Python double loop.

A is the hypothesis, B the reference.  At a cell the diagonal (COPY when the elements are equal, else SUB) is taken if its cost is <=
both others, otherwise INS (from i-1) if its cost is <= DEL's, otherwise DEL (from j-1).  The walk starts at (|A|, |B|) and, unlike the
script's, is complete: at j = 0 the remaining i are INS, at i = 0 the remaining j are DEL."""
import numpy as np

from vistaocr_amd.textutils import form_tokenized_words

COPY, SUB, INS, DEL = 1, 2, 3, 4
FIELDS = ("char_dist", "char_sub", "char_ins", "char_del", "hyp_chars", "ref_chars",
          "word_dist", "word_sub", "word_ins", "word_del", "hyp_words", "ref_words")


def plain_table(A, B):
    """(D, op) of the double loop: D [la+1, lb+1] distances, op [la+1, lb+1] the operation taken at each inner cell."""
    la, lb = len(A), len(B)
    D = np.zeros((la + 1, lb + 1), dtype=np.int64)
    op = np.zeros((la + 1, lb + 1), dtype=np.int8)
    D[:, 0] = np.arange(la + 1)
    D[0, :] = np.arange(lb + 1)
    for i in range(1, la + 1):
        for j in range(1, lb + 1):
            ins, dele = D[i - 1, j] + 1, D[i, j - 1] + 1
            same = A[i - 1] == B[j - 1]
            sub = D[i - 1, j - 1] + (0 if same else 1)
            D[i, j] = min(ins, dele, sub)
            if sub <= ins and sub <= dele:
                op[i, j] = COPY if same else SUB
            elif ins <= dele:
                op[i, j] = INS
            else:
                op[i, j] = DEL
    return D, op


def antidiagonal_table(A, B):
    """The same tables, one anti-diagonal i + j = d at a time (elements are mapped to integers first)."""
    ids = {}
    a = np.array([ids.setdefault(x, len(ids)) for x in A], dtype=np.int64)
    b = np.array([ids.setdefault(x, len(ids)) for x in B], dtype=np.int64)
    la, lb = len(a), len(b)
    D = np.zeros((la + 1, lb + 1), dtype=np.int64)
    D[:, 0] = np.arange(la + 1)
    D[0, :] = np.arange(lb + 1)
    op = np.zeros((la + 1, lb + 1), dtype=np.int8)
    if la == 0 or lb == 0:
        return D, op
    ne = (a[:, None] != b[None, :]).astype(np.int64)
    for d in range(2, la + lb + 1):
        i = np.arange(max(1, d - lb), min(la, d - 1) + 1)
        j = d - i
        D[i, j] = np.minimum(np.minimum(D[i - 1, j - 1] + ne[i - 1, j - 1], D[i - 1, j] + 1), D[i, j - 1] + 1)
    sub, ins, dele = D[:-1, :-1] + ne, D[:-1, 1:] + 1, D[1:, :-1] + 1
    op[1:, 1:] = np.where((sub <= ins) & (sub <= dele), np.where(ne == 1, SUB, COPY), np.where(ins <= dele, INS, DEL))
    return D, op


def walk(op, la, lb):
    """The operations from the front and the (i, j) each one was taken at (1-based; 0 where the side has no element)."""
    i, j, out = la, lb, []
    while i > 0 or j > 0:
        o = INS if j == 0 else DEL if i == 0 else int(op[i, j])
        out.append((o, 0 if o == DEL else i, 0 if o == INS else j))
        if o == INS:
            i -= 1
        elif o == DEL:
            j -= 1
        else:
            i -= 1
            j -= 1
    return out[::-1]


def trace(A, B, table=plain_table):
    """(distance, [sub, ins, del], ops from the front with their cells)."""
    D, op = table(A, B)
    steps = walk(op, len(A), len(B))
    counts = [sum(1 for o, _, _ in steps if o == k) for k in (SUB, INS, DEL)]
    assert sum(counts) == D[len(A), len(B)]
    return int(D[len(A), len(B)]), counts, steps


def pair_stats(hyp, ref, alphabet, table=plain_table):
    """hyp / ref: label lists (valid ones).  Returns (the twelve statistics in FIELDS' order, uint8 character ops from the front,
    int64 [V,V] confusion of this pair: [reference class][hypothesis class], INS in row 0, DEL in column 0)."""
    canon = alphabet.canonical_indices()
    hc, rc = [alphabet.idx_to_char[int(k)] for k in hyp], [alphabet.idx_to_char[int(k)] for k in ref]
    cd, cc, steps = trace(hc, rc, table)
    conf = np.zeros((len(alphabet), len(alphabet)), dtype=np.int64)
    for o, i, j in steps:
        conf[canon[int(ref[j - 1])] if j else 0, canon[int(hyp[i - 1])] if i else 0] += 1
    hw, rw = form_tokenized_words(hc), form_tokenized_words(rc)
    wd, wc, _ = trace(hw, rw, table)
    return ([cd] + cc + [len(hc), len(rc), wd] + wc + [len(hw), len(rw)], np.array([o for o, _, _ in steps], dtype=np.uint8), conf)


def rates(stats):
    """(cer, wer) as ErrorScorer defines them."""
    return stats[0] / max(stats[5], 1), stats[6] / max(stats[11], 1)
