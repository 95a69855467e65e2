"""The host half of the GEMM dispatch (csrc/gemm_nt.hip) decides what it decided before (no GPU: the queries dereference and launch nothing).

tests/golden/gemm_dispatch_table.json was recorded by tests/golden/make_golden_gemm_dispatch.py from a known-good library (its header names the
commit); this replays every recorded call against the built library: which tile `ovla_gemm_resolved_tile` answers (or which error, word for
word), what `ovla_gemm_plan` plans, which schedule `ovla_gemm_fixed_schedule` fixes and the workspace it needs.  An edit of the tile-config
table that changes a decision fails here; a deliberate change re-records the table from the commit that made it (see the generator)."""
import importlib.util
import json
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_golden_gemm_dispatch", GOLDEN / "make_golden_gemm_dispatch.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def table():
    return json.loads((GOLDEN / "gemm_dispatch_table.json").read_text())


@pytest.fixture(scope="module")
def libs(gen):
    import __graft_entry__ as g

    g._pkg()
    return gen.load_lib()


def test_fixture_covers_the_grid_the_generator_defines(gen, table):
    assert len(table["header"]["commit"]) == 40 and len(table["header"]["build_hash"]) == 32
    assert table["M"] == gen.MS and [tuple(c) for c in table["classes"]] == gen.CLASSES and table["tiles"] == gen.TILES
    assert [tuple(c) for c in table["combos"]] == gen.combos() and table["plan_workspaces"] == gen.PLAN_WS
    assert set(gen.TILES) >= {0, 7, 103, 110, 1018} | set(gen.BASE_TILES) | set(gen.PLUS100)
    assert set(gen.TILES) == {0} | set(gen.BASE_TILES) | set(gen.PLUS100) | set(gen.REMOVED_TILES) | set(gen.UNKNOWN_TILES) and len(gen.TILES) == len(set(gen.TILES))
    assert len(table["resolved"]) == len(gen.CLASSES) and all(len(r) == len(gen.combos()) for r in table["resolved"])
    assert all(len(row) == len(gen.TILES) for row in table["rows"])
    assert (GOLDEN / "gemm_dispatch_table.json").stat().st_size < max(f.stat().st_size for f in GOLDEN.glob("*.npz"))


def test_resolved_tile_and_error_texts_are_the_recorded_ones(gen, table, libs):
    _lib, lib = libs
    errors = table["errors"]

    def want(code):
        return code if code >= 0 else errors[-code - 1]

    bad, calls = [], 0
    for cls, per_cls in zip(gen.CLASSES, table["resolved"]):
        for combo, entry in zip(gen.combos(), per_cls):
            if isinstance(entry, dict):   # rejected by the argument checks whatever M and tile: one representative call pins the text
                todo = [(gen.MS[0], 0, entry["rep"])]
            else:
                todo = [(M, tile, v[i] if isinstance(v, list) else v) for tile, v in zip(gen.TILES, table["rows"][entry]) for i, M in enumerate(gen.MS)]
            for M, tile, code in todo:
                got = gen.resolved(_lib, lib, M, cls, tile, combo)
                calls += 1
                if got != want(code) and len(bad) < 20:
                    bad.append((M, cls, tile, combo, got, want(code)))
    assert not bad, f"{len(bad)}+ of {calls} calls differ (M, class, tile, (epilogue, split_k, workspace), got, recorded): {bad}"


def test_plan_is_the_recorded_one(gen, table, libs):
    _lib, lib = libs
    for cls, per_cls in zip(gen.CLASSES, table["plan"]):
        for M, per_m in zip(gen.MS, per_cls):
            for ws, rec in zip(gen.PLAN_WS, per_m):
                got = gen.plan(lib, M, cls, ws)
                assert got[:4] == rec[:4], (M, cls, ws, got, rec)
                assert abs(got[4] - rec[4]) <= 1e-12 * abs(rec[4]), (M, cls, ws, got, rec)


def test_fixed_schedule_and_its_workspace_are_the_recorded_ones(gen, table, libs):
    _lib, lib = libs
    for cls, per_cls in zip(gen.CLASSES, table["fixed"]):
        assert len(per_cls) == 32
        for flags, rec in enumerate(per_cls):
            assert gen.fixed(_lib, lib, cls, flags) == rec, (cls, flags)
