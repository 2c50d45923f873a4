"""CPU: the fp64 restatement of the CTC edit scores (tests/edit_ref.py: every edit from the hypothesis's forward and backward lattices)
against the independent definition - tests.align_ref.align(x, length, edited labelling, canon).ctc for EVERY substitution, deletion
and insertion of every case, to 1e-9 absolute with -inf matched exactly - and vocr_ctc_edit_scores' argument validation through the
C-ABI without a device."""
import numpy as np
import pytest

from tests import edit_ref as er
from vistaocr_amd import _lib

# (T, V, length, labels, canon, what): length = the line's lens entry.
CASES = [
    (5, 4, 5, [], None, "L = 0"),
    (4, 4, 4, [2], None, "L = 1"),
    (6, 4, 6, [1, 2], None, "L = 2; substituting 2 -> 1 or 1 -> 2 creates a repeat"),
    (6, 4, 6, [1, 1], None, "aa: any substitution and either deletion removes the repeat"),
    (7, 4, 7, [1, 2, 1], None, "aba: deleting b creates a repeat"),
    (8, 5, 8, [3, 1, 1, 4], None, "a repeat inside"),
    (2, 4, 2, [1, 1], None, "T too short for aa (needs 3 frames), long enough after either deletion"),
    (3, 4, 3, [1, 2, 1, 2], None, "T too short; a deletion leaves three labels on three frames"),
    (4, 4, 4, [2, 2, 2], None, "T too short for aaa (needs 5 frames): a deletion and a substitution of the middle label fit"),
    (8, 4, 5, [1, 2, 3], None, "lens < T"),
    (8, 4, 1, [3], None, "lens = 1"),
    (6, 4, 0, [2], None, "lens = 0: the deletion leaves the empty labelling on no frames"),
    (6, 4, 0, [], None, "lens = 0, L = 0"),
    (6, 5, 6, [1, 3, 2], [0, 1, 2, 2, 4], "a class of two members, labelled once by each member"),
    (6, 5, 6, [4, 2], [0, 1, 2, 2, 4], "inserting a member of the neighbour's class"),
    (6, 5, 6, [1, 3], [0, 1, 0, 3, 3], "a member in the blank's class: its column is no edit"),
    (6, 5, 6, [1, 2], [0, 1, 0, 3, 3], "an invalid label: in the blank's class"),
    (6, 4, 6, [1, 4], None, "an invalid label: outside the alphabet"),
    (6, 4, 6, [0, 2], None, "an invalid label: the blank"),
    (7, 4, 7, [1, 2], None, "a frame of -inf"),
    (7, 4, 7, [2, 3, 2], None, "-inf columns"),
    (3, 8, 3, [5, 6, 7], None, "every frame forced"),
]


def case_logits(i):
    T, V, length, labels, canon, what = CASES[i]
    rng = np.random.default_rng(300 + i)
    x = rng.normal(0, 1.5, size=(T, V))
    if what == "a frame of -inf":
        x[3, :] = -np.inf
    if what == "-inf columns":
        x[:, 1] = -np.inf
        x[2, 3] = -np.inf
        x[5, 0] = -np.inf
    return x


def assert_same(got, want, tol, label=""):
    """Every entry of ctc / sub / dele / ins: -inf exactly where the other is, otherwise within tol (a number or an array per entry)."""
    worst = 0.0
    for name in ("ctc", "sub", "dele", "ins"):
        g, w = np.asarray(getattr(got, name), dtype=np.float64), np.asarray(getattr(want, name), dtype=np.float64)
        assert g.shape == w.shape, (label, name, g.shape, w.shape)
        assert not np.isnan(g).any() and not np.any(g == np.inf), (label, name)
        assert np.array_equal(np.isneginf(g), np.isneginf(w)), (label, name, np.argwhere(np.isneginf(g) != np.isneginf(w))[:5].tolist())
        fin = np.isfinite(w)
        if fin.any():
            d = np.abs(np.where(fin, g, 0.0) - np.where(fin, w, 0.0))
            t = tol(w) if callable(tol) else tol
            bad = d > t
            assert not bad.any(), (label, name, np.argwhere(bad)[:5].tolist(), float(d.max()))
            worst = max(worst, float(d.max()))
    return worst


@pytest.mark.parametrize("i", range(len(CASES)))
def test_lattice_recursions_equal_the_forward_score_of_every_edited_labelling(i):
    T, V, length, labels, canon, what = CASES[i]
    x = case_logits(i)
    got = er.edit_scores(x, length, labels, canon)
    want = er.direct_scores(x, length, labels, canon)
    worst = assert_same(got, want, 1e-9, what)
    L = len(labels)
    n_edits = L * V + L + (L + 1) * V
    print("case %d (%s): %d edits, %d finite, largest difference %.3g" % (i, what, n_edits, int(np.isfinite(want.sub).sum() + np.isfinite(
        want.dele).sum() + np.isfinite(want.ins).sum()), worst))
    if "invalid" in what:
        assert want.ctc == -np.inf and not np.isfinite(want.sub).any() and not np.isfinite(want.dele).any() and not np.isfinite(want.ins).any()
    if what.startswith("T too short for a"):
        assert want.ctc == -np.inf
    if what.startswith("T too short for aa "):
        assert np.isfinite(want.dele).all()
    if what.startswith("lens = 0:"):
        assert want.dele[0] == 0.0 and not np.isfinite(want.sub).any() and not np.isfinite(want.ins).any()


def test_random_lines():
    """T = 3 .. 8, random labellings with repeats, some that do not fit: every edit against the direct definition."""
    rng = np.random.default_rng(17)
    edits = 0
    for k in range(60):
        T, V = int(rng.integers(3, 9)), int(rng.integers(3, 6))
        L = int(rng.integers(0, 5))
        labels = [int(v) for v in rng.integers(1, V, size=L)]
        canon = None
        if k % 4 == 3:
            canon = list(range(V))
            canon[V - 1] = V - 2
        x = rng.normal(0, 2.0, size=(T, V))
        length = int(rng.integers(1, T + 1))
        assert_same(er.edit_scores(x, length, labels, canon), er.direct_scores(x, length, labels, canon), 1e-9, (k, labels, length))
        edits += L * V + L + (L + 1) * V
    assert edits > 800


def test_own_class_column_is_the_unedited_score_and_classes_share_values():
    canon = [0, 1, 2, 2, 4]
    x = np.random.default_rng(3).normal(0, 1.5, size=(7, 5))
    labels = [1, 3, 4]
    s = er.edit_scores(x, 7, labels, canon)
    for p, v in enumerate(labels):
        assert abs(s.sub[p, v] - s.ctc) < 1e-12
    assert np.array_equal(s.sub[:, 2], s.sub[:, 3]) and np.array_equal(s.ins[:, 2], s.ins[:, 3])
    assert np.all(s.sub[:, 0] == -np.inf) and np.all(s.ins[:, 0] == -np.inf)
    ch, gp = er.posteriors(s, labels, canon, 5)
    assert np.allclose(ch.sum(axis=1), 1.0) and np.allclose(gp.sum(axis=1), 1.0)
    assert np.all(ch[:, 3] == 0.0) and np.all(gp[:, 3] == 0.0)            # column 3 is no canonical class: counted once, under 2


def test_c_abi_validation_without_a_device():
    lib = _lib.load()
    assert lib.vocr_ctc_edit_workspace_bytes(294, 32, 96, 1, 67) > 0
    assert lib.vocr_ctc_edit_workspace_bytes(294, 32, 96, 4, 294) > 0            # the beam searches' layout: label_stride = T
    assert lib.vocr_ctc_edit_workspace_bytes(294, 32, 257, 1, 31) == 0
    assert lib.vocr_ctc_edit_workspace_bytes(294, 32, 1, 1, 31) == 0
    assert lib.vocr_ctc_edit_workspace_bytes(294, 32, 96, 129, 31) == 0
    assert lib.vocr_ctc_edit_workspace_bytes(294, 32, 96, 1, 295) == 0           # a labelling longer than the line
    assert lib.vocr_ctc_edit_workspace_bytes(0, 32, 96, 1, 0) == 0
    assert lib.vocr_ctc_edit_workspace_bytes(294, 32, 96, 128, 294) == 0         # 5.7 GB of lattices
    assert lib.vocr_ctc_edit_workspace_bytes(4000, 1, 96, 1, 1823) > 0
    assert lib.vocr_ctc_edit_workspace_bytes(4000, 1, 96, 1, 1824) == 0          # one row of the sweep no longer fits the LDS
    small, big = lib.vocr_ctc_edit_workspace_bytes(294, 32, 96, 1, 20), lib.vocr_ctc_edit_workspace_bytes(294, 32, 96, 1, 60)
    assert big - small == 32 * 2 * 80 * 294 * 4                                  # two lattices of 2 M + 1 positions per labelling
    rc = lib.vocr_ctc_edit_scores(None, None, 294, 32, 96, None, None, None, 1, 31, 31, None, None, None, None, None, 0, None)
    assert rc == -1 and b"vocr_ctc_edit_scores" in lib.vocr_last_error()
