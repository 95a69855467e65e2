"""Per-tensor statistics on the CPU: the numpy restatement (tests/tensor_stats_reference.py) against ovla_grad_sumsq's restatement and against
closed forms on exact data, and ovla_tensor_stats_plan -- host only, so it runs here -- on its prefix sums and on every refusal of the contract
(include/ovla.h "Per-tensor statistics")."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import grad_clip_reference as G
from tests import tensor_stats_reference as R

C = R.CHUNK


@pytest.fixture(scope="module")
def values():
    g = np.random.default_rng(23)
    n = 5 * C + 77
    v = (g.standard_normal(n) * 10.0 ** g.uniform(-3, 3, n)).astype(np.float32)
    w = (g.standard_normal(n) * 0.05).astype(np.float32)
    return v, w


@pytest.mark.parametrize("scale", (1.0, 1.0 / 3.0), ids=["scale1", "scale_third"])
@pytest.mark.parametrize("round_bf16", (True, False), ids=["bf16", "f32"])
def test_one_entry_table_is_grad_sumsq_bit_for_bit(values, round_bf16, scale):
    v, w = values
    for n in (0, 1, 7, 257, C - 1, C, C + 1, 3 * C + 5, v.size):
        got = R.tensor_stats(v, w, [(0, n)], grad_scale=scale, grad_round_bf16=round_bf16)[0]
        want = G.grad_sumsq(v[:n], scale, round_bf16)
        assert got["grad_sumsq"].tobytes() == want.tobytes(), (n, got["grad_sumsq"], want)
        assert got["param_sumsq"].tobytes() == G.grad_sumsq(w[:n], 1.0, False).tobytes(), "the parameter goes through the same sum, unscaled"
        assert got["n_nonfinite"] == 0 and got["n_bad_steps"] == 0
        seen = G.seen_gradient(v[:n], scale, round_bf16)
        assert got["grad_absmax"] == (np.abs(seen).max() if n else 0.0)


def test_exact_data_sums_to_plain_sums_and_to_the_whole_buffer():
    """Small integers: every square and every partial sum is exact in double, so any order gives the same bits."""
    g = np.random.default_rng(5)
    lengths = (0, 1, 7, C - 1, C, C + 1, 3 * C + 5)
    segs, off = [], 0
    for n in lengths:                                               # chunk-aligned starts: the whole buffer's chunks are the segments' chunks
        segs.append((off, n))
        off += (n + C - 1) // C * C
    grad = np.zeros(off, np.float32)
    param = np.zeros(off, np.float32)
    for o, n in segs:
        grad[o:o + n] = g.integers(-64, 65, n)
        param[o:o + n] = g.integers(-8, 9, n)
    out = R.tensor_stats(grad, param, segs)
    for (o, n), rec in zip(segs, out):
        assert rec["grad_sumsq"] == np.sum(grad[o:o + n].astype(np.float64) ** 2)
        assert rec["param_sumsq"] == np.sum(param[o:o + n].astype(np.float64) ** 2)
        assert rec["grad_absmax"] == (np.abs(grad[o:o + n]).max() if n else 0.0) and rec["n_nonfinite"] == 0
    assert out["grad_sumsq"].sum() == G.grad_sumsq(grad) == np.sum(grad.astype(np.float64) ** 2)
    assert out["param_sumsq"].sum() == G.grad_sumsq(param)
    # the scale and the rounding are those of the gradient alone: 1/2 is exact, bf16 keeps 8 bits of these integers
    half = R.tensor_stats(grad, param, segs, grad_scale=0.5, grad_round_bf16=True)
    assert np.array_equal(half["grad_sumsq"] * 4.0, out["grad_sumsq"]) and np.array_equal(half["param_sumsq"], out["param_sumsq"])


def test_non_finite_elements_are_counted_not_maximised_and_latched():
    grad = np.arange(1, 41, dtype=np.float32)
    param = np.ones(40, np.float32)
    grad[[3, 17, 30]] = (np.nan, np.inf, -np.inf)
    segs = [(0, 8), (8, 8), (16, 8), (24, 0), (24, 16)]
    out = R.tensor_stats(grad, param, segs, n_bad_steps=[0, 5, 0, 7, 1])
    assert out["n_nonfinite"].tolist() == [1, 0, 1, 0, 1] and out["n_bad_steps"].tolist() == [1, 5, 1, 7, 2]
    assert out["grad_absmax"].tolist() == [8.0, 16.0, 24.0, 0.0, 40.0]
    assert np.isnan(out["grad_sumsq"][0]) and out["grad_sumsq"][2] == np.inf and out["grad_sumsq"][4] == np.inf and out["grad_sumsq"][3] == 0.0
    assert out["grad_sumsq"][1] == np.sum(np.arange(9, 17.0) ** 2)
    # a finite product that overflows fp32 is non-finite as AdamW sees it
    big = R.segment_stats(np.array([3e38, 1.0], np.float32), np.ones(2, np.float32), grad_scale=2.0)
    assert big["n_nonfinite"] == 1 and big["grad_absmax"] == 2.0
    assert not R.same_records(out, out) and R.same_records(out, R.tensor_stats(grad, param, segs)) == [(1, "n_bad_steps"), (3, "n_bad_steps"), (4, "n_bad_steps")]


# ----------------------------------------------------------------------------------------------------------------------------------------
# ovla_tensor_stats_plan: host only
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops_built(ops):
    import __graft_entry__ as g

    g.build()
    return ops


def spaced(lengths, gap=64):
    segs, off = [], 0
    for n in lengths:
        segs.append((off, n))
        off += (n + gap + 7) // 8 * 8
    return segs, off


def test_plan_prefix_sums(ops_built):
    lengths = (0, 1, 7, C - 1, C, C + 1, 3 * C + 5)
    segs, total = spaced(lengths)
    plan = ops_built.tensor_stats_plan(segs, total)
    assert plan["chunk_start"].dtype == np.int32 and plan["chunk_start"].tolist() == [0, 0, 1, 2, 3, 4, 6, 10] == R.plan(segs).tolist()
    assert (plan["n_segs"], plan["total_chunks"]) == (7, 10) and "segs" not in plan, "host only: no device copy without a device"
    assert R.table_error(segs, total) is None
    # exactly at the end of the buffer, and one all-empty table
    assert ops_built.tensor_stats_plan([(0, C), (C, 8)], C + 8)["chunk_start"].tolist() == [0, 1, 2]
    assert ops_built.tensor_stats_plan([(0, 0), (0, 0)], 0)["chunk_start"].tolist() == [0, 0, 0]


REFUSED = {"no segments": ([], 100),
           "negative n": ([(0, -1)], 100),
           "negative offset": ([(-8, 4)], 100),
           "offset % 8": ([(0, 3), (4, 3)], 100),
           "descending": ([(64, 8), (0, 8)], 100),
           "overlapping": ([(0, 9), (8, 8)], 100),
           "past the buffer": ([(0, 8), (96, 5)], 100),
           "negative buffer": ([(0, 0)], -1)}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_plan_refusals(ops_built, what):
    _lib = importlib.import_module("openvla-oft_amd._lib")
    segs, buffer_n = REFUSED[what]
    assert R.table_error(segs, buffer_n) is not None
    with pytest.raises(_lib.OvlaError, match="ovla_tensor_stats_plan"):
        ops_built.tensor_stats_plan(segs, buffer_n)


def test_plan_refuses_null_pointers_and_writes_nothing_on_a_refusal(ops_built):
    _lib = importlib.import_module("openvla-oft_amd._lib")
    handle, Seg = _lib.lib(), _lib.STRUCTS["ovla_tensor_seg"]
    table = (Seg * 2)(Seg(0, 8), Seg(8, 8))
    chunk_start = np.full(3, -7, np.int32)
    assert handle.ovla_tensor_stats_plan(table, 2, 16, chunk_start.ctypes.data) == 0 and chunk_start.tolist() == [0, 1, 2]
    assert handle.ovla_tensor_stats_plan(None, 2, 16, chunk_start.ctypes.data) == -1
    assert handle.ovla_tensor_stats_plan(table, 2, 16, None) == -1 and b"ovla_tensor_stats_plan" in handle.ovla_last_error()
    chunk_start[:] = -7
    assert handle.ovla_tensor_stats_plan(table, 2, 15, chunk_start.ctypes.data) == -1 and chunk_start.tolist() == [-7, -7, -7]
    assert ctypes.sizeof(Seg) == 16 and ctypes.sizeof(_lib.STRUCTS["ovla_tensor_stat"]) == R.PARTIAL_BYTES == ops_built.TENSOR_STATS_PARTIAL_BYTES
    assert np.dtype(ops_built.TENSOR_STAT_DTYPE) == R.STAT_DTYPE
