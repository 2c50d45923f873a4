"""CPU: vocr_gemm_plan - the planner vocr_gemm and vocr_gemm_pair launch from - on every row of the GEMM suite's case table
(tests/gemm_ref.py), at the 256 CUs the library assumes without a device (and an MI355X has).  A planner change that silently empties
one of the suite's categories fails here, on any machine."""
import pytest

from tests import gemm_ref as gr


@pytest.fixture(scope="module")
def lib():
    from vistaocr_amd import _lib, build
    build.build()
    return _lib.load()


def _all_plans(lib):
    for case in gr.CASES:
        for epi in case.epis:
            for layout in case.layouts:
                yield case, epi, layout, gr.plans_of(case, epi, layout, lib)


def test_every_row_takes_the_path_it_is_named_for(lib):
    for case, epi, layout, plans in _all_plans(lib):
        assert gr.path_name(plans) == case.expected_path(epi, layout), (case, epi, gr.LAYOUT_NAMES[layout], plans)


def test_the_table_reaches_every_kernel_load_form_and_cut_form(lib):
    seen, pieces, row_tiles, launches, split_epi, pair = set(), set(), set(), set(), set(), set()
    for case, epi, layout, plans in _all_plans(lib):
        for _, p in plans:
            seen.add(gr.path_of(p) + ("" if p["kernel"] == "panel" else " " + gr.LAYOUT_NAMES[layout]))
            if p["kernel"] == "panel":
                seen.add(gr.path_of(p) + " " + gr.LAYOUT_NAMES[layout])
                row_tiles.add(p["max_row_tiles"])
            elif p["pieces_per_tile"] > 1:
                pieces.add(p["pieces_per_tile"])
        if len(plans) == 1 and plans[0][1]["kernel"] == "panel" and plans[0][1]["ksplit"] > 1:
            split_epi.add(epi)
        if case.pair is not None:
            pair.add((case.pair, path_kind(plans)))
    # tile kernel: three tile shapes x two load forms x the cut forms each shape has, in all four layouts
    for layout in gr.LAYOUT_NAMES.values():
        for load in ("vec", "scalar"):
            for path in ("tile64x64/%s/whole", "tile64x64/%s/cut", "tile128x128/%s/cut", "tile128x64/%s/whole", "tile128x64/%s/ragged",
                         "tile128x128/%s/ragged"):
                assert (path % load) + " " + layout in seen, (path % load, layout, sorted(seen))
        for path in ("panel/whole", "panel/split"):
            assert path + " " + layout in seen, (path, layout)
    # the reduce's 4-wide loop with a remainder (pieces = 1 + 4 j + r, r != 0), and without one
    assert any(p > 4 and (p - 1) % 4 for p in pieces) and any((p - 1) % 4 == 0 or p < 5 for p in pieces), pieces
    # row groups of every length: 1 only exists under a K split (the last 8-tile group of 260 rows), where the plan answers the longest
    assert {2, 3, 4, 5, 6, 7, 8, 9, 17, 19} <= row_tiles, row_tiles
    # every epilogue through the panel kernel's slab reduce
    assert split_epi == set(gr.ALL_EPI), split_epi
    # the pair: both modes as one launch (whole and split) and as two calls
    assert pair >= {(0, "panel/whole"), (0, "panel/split"), (1, "panel/whole"), (1, "panel/split"), (0, "2x"), (1, "2x")}, pair


def path_kind(plans):
    return "2x" if len(plans) == 2 else gr.path_of(plans[0][1])


def test_workspace_size_answers_cover_every_plan(lib):
    """vocr_gemm_workspace_bytes / vocr_gemm_pair_workspace_bytes only see m, n, k: whatever layout and (padded) leading dimensions a
    call comes with, a workspace of that size must hold what its plan uses, and a plan made with unlimited workspace must not ask for
    more (or the size answer would quietly cost K cuts)."""
    from vistaocr_amd import ops
    for case in gr.CASES:
        for epi in case.epis:
            has_bias, relu, acc = gr.EPILOGUES[epi]
            for layout in case.layouts:
                ta, tb = layout
                lda, ldb, ldc = case.lds(ta, tb)
                if case.pair is None:
                    size = lib.vocr_gemm_workspace_bytes(case.m, case.n, case.k, int(bool(has_bias or relu)))
                else:
                    size = lib.vocr_gemm_pair_workspace_bytes(case.m, case.n, case.k, case.pair)
                kw = dict(aligned=case.aligned(epi), epilogue=bool(has_bias or relu), accumulate=bool(acc), nprob=2 if case.pair == 0 else 1,
                          nseg=2 if case.pair == 1 else 1, tiles_only=case.tiles_only)
                given = ops.gemm_plan(ta, tb, case.m, case.n, case.k, lda, ldb, ldc, workspace_bytes=size, **kw)
                unlimited = ops.gemm_plan(ta, tb, case.m, case.n, case.k, lda, ldb, ldc, workspace_bytes=1 << 40, **kw)
                assert given["workspace_bytes"] <= size, (case, epi, layout, given, size)
                assert unlimited["workspace_bytes"] <= size and unlimited == given, (case, epi, layout, unlimited, given, size)


def test_plan_query_validates_its_arguments(lib):
    import ctypes
    out = (ctypes.c_int * 12)()
    assert lib.vocr_gemm_plan(0, 0, 0, 4, 4, 4, 4, 4, 3, 0, 0, 0, 1, 1, 0, out) == -1 and b"vocr_gemm_plan" in lib.vocr_last_error()
    assert lib.vocr_gemm_plan(0, 0, 4, 4, 4, 3, 4, 4, 3, 0, 0, 0, 1, 1, 0, out) == -1 and b"leading dimension" in lib.vocr_last_error()
    assert lib.vocr_gemm_plan(0, 0, 4, 4, 4, 4, 4, 4, 3, 0, 0, 0, 2, 2, 0, out) == -1
    assert lib.vocr_gemm_plan(0, 0, 4, 4, 4, 4, 4, 4, 3, 0, 1, 0, 2, 1, 0, out) == -1          # the pair does not accumulate
    assert lib.vocr_gemm_plan(0, 0, 4, 4, 4, 4, 4, 4, 3, 0, 0, 0, 1, 1, 0, None) == -1
    assert lib.vocr_gemm_plan(0, 0, 4, 4, 4, 4, 4, 4, 3, 0, 0, 0, 1, 1, 0, out) == 0 and list(out)[:5] == [0, 1, 1, 1, 32]
