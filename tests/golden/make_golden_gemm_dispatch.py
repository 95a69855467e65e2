"""Records the host-side decisions of the GEMM dispatch (csrc/gemm_nt.hip) as gemm_dispatch_table.json, replayed by
tests/test_gemm_dispatch_table.py against the library under test.  No GPU is needed: the three queries dereference and launch nothing.

  resolved   ovla_gemm_resolved_tile over M x problem class x tile id x epilogue x split_k x workspace -> tile, or (rc, ovla_last_error())
  plan       ovla_gemm_plan over M x problem class x workspace {0, 96 MiB}                           -> tile, full, rem, splits, est_seconds
  fixed      ovla_gemm_fixed_schedule over problem class x epi_flags 0..31 -> (tile, splits) or (rc, error), and
             ovla_gemm_fixed_workspace_bytes of the result over M

The table is the record of a KNOWN-GOOD library (the header names the commit and the library's source hash), never of the code under test:
without --regenerate this script only verifies that the library it is given is the one the fixture was recorded from, and refuses otherwise.

    python tests/golden/make_golden_gemm_dispatch.py [--lib PATH]                                  # verify the fixture's provenance
    python tests/golden/make_golden_gemm_dispatch.py --regenerate --commit HASH [--lib PATH]      # record (from a build of commit HASH)
"""
import argparse
import ctypes
import importlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
OUT = Path(__file__).resolve().parent / "gemm_dispatch_table.json"

MS = [8, 64, 65, 256, 257, 512, 522, 608, 1024, 1216, 2500, 4176, 4864, 9728]
# (N, K, K2, k2_group_n): tests/test_batch_schedule.py::CLASSES, the LoRA classes of tests/test_host_logic.py::test_gemm_schedule_decisions,
# K-extensions of 16 / 64 / 96 / 128 columns, and one K that is not a multiple of 64
CLASSES = [(12288, 4096, 0, 0), (4096, 4096, 0, 0), (22016, 4096, 0, 0), (4096, 11008, 0, 0), (32064, 4096, 0, 0), (4352, 1024, 0, 0),
           (1152, 4608, 0, 0), (4096, 28672, 0, 0), (32, 4096, 0, 0), (12288, 4096, 32, 4096), (768, 256, 0, 0),
           (22016, 4096, 32, 11008), (4096, 11008, 32, 0), (4096, 4096, 32, 0), (3072, 1024, 32, 0), (1024, 1024, 32, 0),
           (4096, 4096, 16, 0), (4096, 4096, 64, 0), (4096, 4096, 96, 0), (4096, 4096, 128, 0), (4096, 4104, 0, 0)]
BASE_TILES = [1, 2, 5, 6, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 21, 22]
PLUS100 = [101, 102, 105, 116, 117, 118, 122]
# ids that were configurations when the table was recorded and have been removed since (3: the 256x128 8-wave tile).  The query answers before
# the unknown-id check, so their recorded columns still hold; they keep their place in the fixture's column order, among the base ids
REMOVED_TILES = [3]
UNKNOWN_TILES = [7, 103, 110, 1018]      # never configurations: kept to pin the unknown-id behaviour
TILES = [0] + sorted(BASE_TILES + REMOVED_TILES) + PLUS100 + UNKNOWN_TILES
EPILOGUES = ["plain", "bias", "residual", "residual_misaligned", "c_pre", "colscale", "film", "rope", "rope_misaligned", "rowsq", "rowscale",
             "swiglu", "swiglu_c_pre", "dact1", "dact2", "a_group_32", "a_group_128"]
SPLIT_KS = [1, 4]
WORKSPACES = [True, False]
PLAN_WS = [0, 96 << 20]
WS_BYTES = 96 << 20

# placeholder device pointers (never dereferenced): 16-byte aligned unless a case asks otherwise
P_A, P_B, P_C, P_A2, P_B2, P_CPRE, P_BIAS, P_RES, P_SCALE, P_GAMMA, P_BETA, P_COS, P_SIN, P_DACT, P_SQ, P_PART, P_R, P_WS = (
    0x10000 * (i + 1) for i in range(18))
ACT_SWIGLU = 5


def load_lib(path=None):
    """The library with the prototypes of include/ovla.h.  `path`: a build to load as it is (no staleness check: the parent's build is
    loaded beside newer sources); None: the tree's own library through _lib.lib()."""
    if str(ROOT) not in sys.path:
        sys.path.insert(0, str(ROOT))
    _lib = importlib.import_module("openvla-oft_amd._lib")
    if path is None:
        return _lib, _lib.lib()
    import torch  # noqa: F401  (the HIP runtime torch ships must be the first one mapped, as in _lib.lib())

    handle = ctypes.CDLL(str(path), mode=2)
    for name, (ret, argtypes) in _lib.FUNCTIONS.items():
        fn = getattr(handle, name)
        fn.restype = _lib._CTYPE[ret] if ret in _lib._CTYPE else ctypes.c_int
        fn.argtypes = [ctypes.POINTER(_lib.STRUCTS[t]) if kind == "struct" else _lib._CTYPE[t] for kind, t in argtypes]
    return _lib, handle


def gemm_args(_lib, M, cls, tile, epi, split_k, workspace):
    N, K, K2, group = cls
    a = _lib.STRUCTS["ovla_gemm_args"]()
    a.A, a.lda, a.B, a.ldb, a.C, a.ldc = P_A, K, P_B, K, P_C, N
    a.M, a.N, a.K, a.K2, a.k2_group_n, a.tile, a.split_k, a.alpha = M, N, K, K2, group, tile, split_k, 1.0
    if K2 > 0:
        a.A2, a.lda2, a.B2, a.ldb2 = P_A2, K2 * (N // group if group else 1), P_B2, K2
    if workspace:
        a.workspace, a.workspace_bytes = P_WS, max(WS_BYTES, split_k * M * N * 4 if split_k > 1 else 0)
    if epi == "bias":
        a.bias = P_BIAS
    elif epi == "residual":
        a.residual, a.ldr = P_RES, N
    elif epi == "residual_misaligned":
        a.residual, a.ldr = P_RES, N + 4
    elif epi == "c_pre":
        a.C_pre = P_CPRE
    elif epi == "colscale":
        a.colscale = P_SCALE
    elif epi == "film":
        a.film_gamma, a.film_beta, a.film_rows = P_GAMMA, P_BETA, 8
    elif epi in ("rope", "rope_misaligned"):
        off = 8 if epi == "rope_misaligned" else 0
        a.rope_cos, a.rope_sin, a.rope_S, a.rope_cols = P_COS + off, P_SIN + off, 76, max(128, (N * 2 // 3) // 128 * 128)
    elif epi == "rowsq":
        a.rowsq_out = P_SQ
    elif epi == "rowscale":
        a.rowscale_part, a.rowscale_slots, a.rowscale_eps, a.rowscale_r = P_PART, {4096: 64, 11008: 172}.get(K, 8), 1e-6, P_R
    elif epi in ("swiglu", "swiglu_c_pre"):
        a.act = ACT_SWIGLU
        if epi == "swiglu_c_pre":
            a.C_pre = P_CPRE
    elif epi == "dact1":
        a.dact_src, a.ld_dact, a.dact_mode, a.dact_act = P_DACT, N, 1, 1
    elif epi == "dact2":
        a.dact_src, a.ld_dact, a.dact_mode, a.ldc = P_DACT, 2 * N, 2, 2 * N
    elif epi in ("a_group_32", "a_group_128"):
        a.a_group_n = 32 if epi == "a_group_32" else 128
        a.lda = (N // a.a_group_n) * K
    else:
        assert epi == "plain", epi
    return a


def combos():
    return [(e, s, w) for e in EPILOGUES for s in SPLIT_KS for w in WORKSPACES]


def resolved(_lib, lib, M, cls, tile, combo):
    """-> the resolved tile id, or [rc, error text]."""
    a = gemm_args(_lib, M, cls, tile, *combo)
    t = ctypes.c_int32(-7)
    rc = lib.ovla_gemm_resolved_tile(ctypes.byref(a), ctypes.addressof(t))
    return t.value if rc == 0 else [rc, lib.ovla_last_error().decode()]


def plan(lib, M, cls, ws):
    t, f, r, s = (ctypes.c_int32() for _ in range(4))
    e = ctypes.c_double()
    rc = lib.ovla_gemm_plan(M, cls[0], cls[1], cls[2], cls[3], ws, *(ctypes.addressof(x) for x in (t, f, r, s, e)))
    assert rc == 0
    return [t.value, f.value, r.value, s.value, e.value]


def fixed(_lib, lib, cls, flags):
    """-> [tile, splits, [workspace bytes per M]], or [rc, error text]."""
    s = _lib.STRUCTS["ovla_gemm_schedule"]()
    rc = lib.ovla_gemm_fixed_schedule(cls[0], cls[1], cls[2], cls[3], flags, ctypes.byref(s))
    if rc != 0:
        return [rc, lib.ovla_last_error().decode()]
    return [s.tile, s.splits, [lib.ovla_gemm_fixed_workspace_bytes(M, cls[0], ctypes.byref(s)) for M in MS]]


def record(_lib, lib):
    """The table.  `resolved`: one entry per (class, combo), an index into `rows`; a row holds one value per tile id, a single value where
    every M agrees and a list over MS otherwise; a value is a tile id (>= 0) or -(1 + index into `errors`).  A (class, combo) that the
    argument checks reject with the same text for every M and tile is kept as ONE representative call (M = MS[0], tile = 0): {"rep": value}."""
    errors, rows, row_ix = [], [], {}

    def code(v):
        if isinstance(v, int):
            assert v >= 0
            return v
        if v not in errors:
            errors.append(v)
        return -(1 + errors.index(v))

    index = []
    for cls in CLASSES:
        per_cls = []
        for combo in combos():
            row = []
            for tile in TILES:
                vals = [code(resolved(_lib, lib, M, cls, tile, combo)) for M in MS]
                row.append(vals[0] if len(set(vals)) == 1 else vals)
            if all(isinstance(v, int) and v < 0 and v == row[0] for v in row):
                per_cls.append({"rep": row[0]})
                continue
            key = json.dumps(row)
            if key not in row_ix:
                row_ix[key] = len(rows)
                rows.append(row)
            per_cls.append(row_ix[key])
        index.append(per_cls)
    return {
        "M": MS, "classes": [list(c) for c in CLASSES], "tiles": TILES, "combos": [list(c) for c in combos()], "plan_workspaces": PLAN_WS,
        "errors": errors, "rows": rows, "resolved": index,
        "plan": [[[plan(lib, M, cls, ws) for ws in PLAN_WS] for M in MS] for cls in CLASSES],
        "fixed": [[fixed(_lib, lib, cls, flags) for flags in range(32)] for cls in CLASSES],
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=None, help="library to query (default: the tree's own build)")
    ap.add_argument("--regenerate", action="store_true", help="record a new table from this library")
    ap.add_argument("--commit", default=None, help="with --regenerate: the commit the library was built from")
    args = ap.parse_args()
    _lib, lib = load_lib(args.lib)
    built = lib.ovla_build_hash().decode()
    if not args.regenerate:
        if not OUT.exists():
            sys.exit(f"{OUT.name} does not exist; record it with --regenerate --commit HASH from a build of a known-good commit")
        head = json.loads(OUT.read_text())["header"]
        if head["build_hash"] != built:
            sys.exit(f"refusing: {OUT.name} was recorded from commit {head['commit']} (library source hash {head['build_hash']}), this library was built "
                     f"from sources with hash {built}.  The table is the record of a known-good parent, not of the code under test; pass --regenerate "
                     f"--commit HASH only to record a deliberate change of the dispatch from a build of that commit.")
        print(f"{OUT.name}: recorded from commit {head['commit']}, which is this library ({built})")
        return
    if not args.commit:
        sys.exit("--regenerate needs --commit HASH (the commit the library was built from)")
    table = {"header": {"commit": args.commit, "build_hash": built, "generator": "tests/golden/make_golden_gemm_dispatch.py"}}
    table.update(record(_lib, lib))
    OUT.write_text(json.dumps(table, separators=(",", ":")) + "\n")
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes): {len(table['rows'])} distinct rows, {len(table['errors'])} error texts")


if __name__ == "__main__":
    main()
