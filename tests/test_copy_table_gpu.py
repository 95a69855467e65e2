"""ovla_copy_table (csrc/copy_table.hip): the grouped, strided device-to-device copy behind the policy pool's slot swap, byte-exact against numpy.
One table mixes every kind of entry the kernel distinguishes: the 16-byte vector path and the 2-byte element path, rows that share a tile, a row
that spans many tiles, the 64-byte segments at a 256-byte stride of the B_slots layout, and an entry without rows."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

load = importlib.import_module
MIB = 1 << 20

# (source offset, destination offset, src_ld_bytes, dst_ld_bytes, rows, row_bytes) inside the two arenas; the arenas' bases are 256-byte aligned
LAYOUT = [
    (34, 6, 2, 2, 1, 2),                                    # 1 row of 2 bytes
    (64, 102, 28, 28, 1, 28),                               # 1 row of 28 bytes
    (1024, 1024, 64, 256, 300, 64),                         # lora_B's shape: 64-byte segments at a 256-byte destination stride
    (32768, 81920, 2048 + 64, 4096, 7, 2048),               # 7 rows of 2 KiB, both sides strided
    (65536, 131072, MIB + 6, MIB + 6, 1, MIB + 6),          # 1 row that spans 65 tiles, on the element path (row_bytes % 16 == 6)
    (2 * MIB + 18, 2 * MIB + 34, 128, 160, 5, 96),          # both sides 2 bytes off 16-byte alignment
    (2 * MIB + 4096, 2 * MIB + 4096, 64, 64, 0, 64),        # rows == 0: skipped
]
ARENA = 2 * MIB + 8192
B_ENTRY = 2


def _entries(src, dst, layout):
    return [(src.data_ptr() + so, dst.data_ptr() + do, sld, dld, rows, rb) for so, do, sld, dld, rows, rb in layout]


def _expected(src_np, dst_np, layout):
    want, inside = dst_np.copy(), np.zeros(dst_np.shape, dtype=bool)
    for so, do, sld, dld, rows, rb in layout:
        for r in range(rows):
            want[do + r * dld: do + r * dld + rb] = src_np[so + r * sld: so + r * sld + rb]
            inside[do + r * dld: do + r * dld + rb] = True
    return want, inside


def test_plan_counts_tiles_and_refuses_on_the_host(pkg):
    """ovla_copy_table_plan needs no device: the tile prefix sums of LAYOUT (16 KiB tiles) and the refusals, on made-up even addresses."""
    _lib = load("openvla-oft_amd._lib")
    lib, T = _lib.lib(), _lib.STRUCTS["ovla_copy_entry"]

    def plan(layout, n=None):
        arr = (T * max(len(layout), 1))()
        for i, (so, do, sld, dld, rows, rb) in enumerate(layout):
            arr[i].src, arr[i].dst, arr[i].src_ld_bytes, arr[i].dst_ld_bytes, arr[i].rows, arr[i].row_bytes = 0x10000000 + so, 0x20000000 + do, sld, dld, rows, rb
        starts = (ctypes.c_int32 * (len(layout) + 1))()
        rc = lib.ovla_copy_table_plan(arr, len(layout) if n is None else n, ctypes.cast(starts, ctypes.c_void_p))
        return rc, list(starts), lib.ovla_last_error().decode()

    rc, starts, _ = plan(LAYOUT)
    assert rc == 0 and starts == [0, 1, 2, 4, 5, 70, 71, 71]
    assert plan([(0, 0, 16384, 16384, 3, 16384)])[1] == [0, 3] and plan([(0, 0, 16386, 16386, 3, 16386)])[1] == [0, 6]
    for layout, n, word in (([(0, 0, 64, 64, 2, 27)], None, "row_bytes"), ([(0, 0, 64, 64, 2, 0)], None, "row_bytes"), ([(0, 1, 64, 64, 2, 28)], None, "multiples of 2"),
                            ([(0, 0, 63, 64, 1, 28)], None, "multiples of 2"), ([(0, 0, 64, 16, 2, 32)], None, "below row_bytes"), ([(0, 0, 64, 64, -1, 32)], None, "rows"),
                            (LAYOUT, 0, "n = 0"), (LAYOUT, -2, "n = -2")):
        rc, _, msg = plan(layout, n)
        assert rc != 0 and word in msg, (layout, n, msg)
    assert lib.ovla_copy_table_plan(ctypes.POINTER(T)(), 1, None) != 0 and "null" in lib.ovla_last_error().decode()


@pytest.fixture(scope="module")
def arenas(dev):
    g = torch.Generator().manual_seed(11)
    src = torch.randint(0, 256, (ARENA,), dtype=torch.uint8, generator=g).to(dev)
    pattern = ((torch.arange(ARENA, dtype=torch.int64) * 37 + 11) % 251).to(torch.uint8)
    assert src.data_ptr() % 256 == 0
    return src, pattern


@pytest.mark.gpu
def test_mixed_table_is_byte_exact(arenas, dev):
    ops = load("openvla-oft_amd.ops")
    src, pattern = arenas
    dst = pattern.to(dev)
    assert dst.data_ptr() % 256 == 0
    tab = ops.copy_table(_entries(src, dst, LAYOUT))
    assert tab["n"] == len(LAYOUT) and tab["nbytes"] == sum(e[4] * e[5] for e in LAYOUT)
    # tiles of 16 KiB: 1 + 1 + ceil(300 / 256) + ceil(7 / 8) + 65 + 1 + 0
    assert tab["total"] == 1 + 1 + 2 + 1 + 65 + 1
    got = dst.cpu().numpy()
    want, inside = _expected(src.cpu().numpy(), pattern.numpy(), LAYOUT)
    assert inside.sum() == tab["nbytes"], "the test's rectangles do not overlap"
    assert np.array_equal(got[inside], want[inside]), "a byte inside a destination rectangle differs from its source"
    assert np.array_equal(got[~inside], pattern.numpy()[~inside]), "a byte outside the destination rectangles was written"
    assert (got[inside] != pattern.numpy()[inside]).mean() > 0.9, "precondition: the copy is visible against the pre-filled pattern"
    # the same table again (cached by value) into the same place: idempotent
    assert ops.copy_table(_entries(src, dst, LAYOUT)) is tab
    assert np.array_equal(dst.cpu().numpy(), want)


@pytest.mark.gpu
def test_single_entry_table_matches(arenas, dev):
    ops = load("openvla-oft_amd.ops")
    src, pattern = arenas
    dst_all, dst_one = pattern.to(dev), pattern.to(dev)
    ops.copy_table(_entries(src, dst_all, LAYOUT))
    for k in (B_ENTRY, 4, 5):
        dst_one.copy_(pattern)
        tab = ops.copy_table(_entries(src, dst_one, [LAYOUT[k]]))
        assert tab["n"] == 1
        want, inside = _expected(src.cpu().numpy(), pattern.numpy(), [LAYOUT[k]])
        got = dst_one.cpu().numpy()
        assert np.array_equal(got, want)
        assert np.array_equal(got[inside], dst_all.cpu().numpy()[inside]), f"entry {k} alone differs from entry {k} in the mixed table"


@pytest.mark.gpu
def test_tensor_entries(dev):
    """ops.copy_entry on the pool's own shapes: a contiguous row group into A_slots, lora_B into a column block of B_slots, a flat buffer."""
    ops, engine = load("openvla-oft_amd.ops"), load("openvla-oft_amd.engine")
    g = torch.Generator().manual_seed(5)
    G, n, r, in_f, out_f, s = 3, 4, 32, 72, 200, 2
    A = torch.randn(G * r, in_f, generator=g).to(torch.bfloat16).to(dev)
    Bm = torch.randn(out_f, r, generator=g).to(torch.bfloat16).to(dev)
    flat = torch.randn(1001, generator=g).to(dev)
    A_slots, B_slots = torch.full((G * n * r, in_f), 7.0, dtype=torch.bfloat16, device=dev), torch.full((out_f, n * r), 7.0, dtype=torch.bfloat16, device=dev)
    flat_dst = torch.zeros_like(flat)
    entries = [ops.copy_entry(A[k * r:(k + 1) * r], A_slots[engine.slot_a_rows(k, s, n, r)]) for k in range(G)]
    entries += [ops.copy_entry(Bm, B_slots[:, s * r:(s + 1) * r]), ops.copy_entry(flat, flat_dst)]
    assert entries[G][2:] == (64, 256, out_f, 64)
    ops.copy_table(entries)
    A_want, B_want = torch.full_like(A_slots, 7.0), torch.full_like(B_slots, 7.0)
    engine.fill_slot(A_want, B_want, s, A, Bm, G)
    assert torch.equal(A_slots, A_want) and torch.equal(B_slots, B_want) and torch.equal(flat_dst, flat)


@pytest.mark.gpu
def test_refusals(arenas, dev):
    ops, _lib = load("openvla-oft_amd.ops"), load("openvla-oft_amd._lib")
    src, pattern = arenas
    dst = pattern.to(dev)
    lib = _lib.lib()
    good = ops.copy_table_build(_entries(src, dst, LAYOUT[:1]), dev)
    ptr = ctypes.cast(ctypes.c_void_p(good["table"].data_ptr()), ctypes.POINTER(_lib.STRUCTS["ovla_copy_entry"]))
    null = ctypes.POINTER(_lib.STRUCTS["ovla_copy_entry"])()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ovla_copy_table(null, good["tile_start"].data_ptr(), 1, good["total"], stream) != 0
    assert b"null" in lib.ovla_last_error()
    for n in (0, -3):
        assert lib.ovla_copy_table(ptr, good["tile_start"].data_ptr(), n, good["total"], stream) != 0
        assert b"entries" in lib.ovla_last_error()
    with pytest.raises(_lib.OvlaError, match="n = 0"):
        ops.copy_table([])
    with pytest.raises(_lib.OvlaError, match="row_bytes"):
        ops.copy_table(_entries(src, dst, [(0, 0, 64, 64, 2, 27)]))
    with pytest.raises(_lib.OvlaError, match="multiples of 2"):
        ops.copy_table(_entries(src, dst, [(1, 0, 64, 64, 2, 28)]))
    with pytest.raises(_lib.OvlaError, match="below row_bytes"):
        ops.copy_table(_entries(src, dst, [(0, 0, 64, 16, 2, 32)]))
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), pattern), "a refused table writes nothing"
