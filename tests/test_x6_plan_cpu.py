"""CPU: vocr_gemm_x6_plan - the planner vocr_gemm_x6 / vocr_gemm_h3 and their two-view forms launch from - on every row of the split-operand
GEMM suite's case table (tests/x6_ref.py), at the 256 CUs the library assumes without a device (and an MI355X has).  A planner change that
silently empties one of the suite's categories fails here, on any machine."""
import ctypes

import pytest

from tests import x6_ref as xr


@pytest.fixture(scope="module")
def ops():
    from vistaocr_amd import build, ops
    build.build()
    return ops


def test_every_row_takes_the_path_it_is_named_for(ops):
    for case in xr.CASES:
        plan = case.ask(ops)
        assert plan["cus"] == 256
        assert xr.path_problem(case, plan) is None, xr.path_problem(case, plan)


def test_the_table_reaches_every_category_and_launch_form(ops):
    assert {c.what for c in xr.CASES} == set(xr.CATEGORIES)
    paths, grids, stages, mtiles_mod4 = set(), set(), set(), set()
    for case in xr.CASES:
        p = case.ask(ops)
        paths.add(xr.path_of(p))
        grids.add(p["whole_tiles"])
        grids.add(p["cut_tiles"] * p["ksplit"])
        if p["cut_tiles"] == 0:
            stages.add((p["tile"], p["stages_per_split"]))
        mtiles_mod4.add(((case.m + 255) // 256) % 4)
    assert paths >= {"narrow/whole", "narrow/cut", "narrow/rounds+cut", "wide/whole", "wide/cut", "wide/rounds+cut", "narrow/whole wide-refused"}, paths
    # fewer k16 stages than ring slots, on both tiles: 1 .. 6 (fp16x3 has six slots on the narrow tile, bf16x6 four) and one more
    assert {(4, s) for s in range(1, 8)} | {(8, s) for s in range(1, 7)} <= stages, stages
    # grids below 8 workgroups, grids that are no multiple of 8, last panels of 1, 2 and 3 row tiles
    assert {1, 3, 4, 6, 9, 15} <= grids and mtiles_mod4 >= {0, 1, 2, 3}, (grids, mtiles_mod4)


def test_plan_answers_are_consistent_and_fit_the_workspace(ops):
    from vistaocr_amd import _lib
    lib = _lib.load()
    for case in xr.CASES:
        p = case.ask(ops)
        nkk = case.k16 // 16
        assert p["whole_tiles"] + p["cut_tiles"] == p["tiles"] and p["tile"] in (4, 8)
        assert (p["ksplit"] - 1) * p["stages_per_split"] < nkk <= p["ksplit"] * p["stages_per_split"]        # no empty split
        assert (p["cut_tiles"] == 0) == (p["ksplit"] == 1) and (p["cut_tiles"] == 0 or case.ws)
        assert p["workspace_bytes"] == p["cut_tiles"] * p["ksplit"] * 256 * 32 * p["tile"] * 4
        assert p["workspace_bytes"] <= lib.vocr_gemm_x6_workspace_bytes(case.m, case.n, case.k16)
        assert p["cut_tiles"] * p["ksplit"] <= p["cus"]                                                      # the cut remainder is at most one round


def test_plan_query_validates_its_arguments(ops):
    from vistaocr_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 9)()
    assert lib.vocr_gemm_x6_plan(0, 128, 64, 128, 0, -1, 1, out) == -1 and b"vocr_gemm_x6_plan" in lib.vocr_last_error()
    assert lib.vocr_gemm_x6_plan(256, 128, 40, 128, 0, -1, 1, out) == -1                     # k % 16
    assert lib.vocr_gemm_x6_plan(256, 128, 64, 128, 8, -1, 1, out) == -1 and b"tile boundaries" in lib.vocr_last_error()
    assert lib.vocr_gemm_x6_plan(256, 128, 64, 128, 0, 8, 1, out) == -1
    assert lib.vocr_gemm_x6_plan(256, 128, 64, 128, 0, -1, 1, None) == -1
    assert lib.vocr_gemm_x6_plan(256, 128, 64, 128, 0, -1, 1, out) == 0 and list(out) == [4, 1, 1, 0, 1, 4, 1, 256, 0]
