"""ovla_tensor_stats on the GPU, on raw buffers: every field of every segment bit for bit against the numpy restatement
(tests/tensor_stats_reference.py), no read outside a segment, no write outside partials and out, one segment's data reaching only its own
entry, the non-finite counts and the latch, ovla_grad_sumsq's bits from a one-entry table, and the launch-side refusals.  Every comparison
is exact."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests import grad_clip_reference as G
from tests import tensor_stats_reference as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
load = importlib.import_module
C = R.CHUNK
GUARD, GAP = 64, 64
# nothing, the scalar tail alone, a partial group, one group, a group and a tail, one wave / one workgroup of groups short and over, the last
# chunk short by one, exactly full, over by one, several chunks, and 258 partials: more than the second launch has lanes
LENGTHS = (0, 1, 3, 4, 5, 255, 257, C - 1, C, C + 1, 3 * C + 5, 257 * C + 5)
SCALES = (1.0, 1.0 / 3.0)


def layout(lengths):
    segs, off = [], 0
    for n in lengths:
        segs.append((off, n))
        off = (off + n + 7) // 8 * 8 + GAP
    return segs, off


SEGS, TOTAL = layout(LENGTHS)


@pytest.fixture(scope="module")
def host():
    """Flat host buffers, shared read-only: gradients of mixed sign over six decades (as the grad-clip tests draw theirs) and parameters as
    fp32 and as bf16 bits, NaN in every gap between the segments."""
    g = np.random.default_rng(17)
    grad = np.full(TOTAL, np.nan, np.float32)
    p32 = np.full(TOTAL, np.nan, np.float32)
    p16 = np.full(TOTAL, 0x7FC0, np.uint16)
    for off, n in SEGS:
        grad[off:off + n] = (g.standard_normal(n) * 10.0 ** g.uniform(-3, 3, n)).astype(np.float32)
        p32[off:off + n] = (g.standard_normal(n) * 10.0 ** g.uniform(-2, 1, n)).astype(np.float32)
        p16[off:off + n] = (G.bf16_round(p32[off:off + n]).view(np.uint32) >> 16).astype(np.uint16)
    for a in (grad, p32, p16):
        a.setflags(write=False)
    return dict(grad=grad, f32=p32, bf16=p16)


_twin = {}


def twin(host, param, round_bf16, scale):
    """The restatement's records for the shared buffers, computed once per variant."""
    key = (param, round_bf16, scale)
    if key not in _twin:
        widened = host["f32"] if param == "f32" else G.widen_bf16(host["bf16"])
        _twin[key] = R.tensor_stats(host["grad"], widened, SEGS, grad_scale=scale, grad_round_bf16=round_bf16)
    return _twin[key]


def guarded(values, dev, fill):
    """Host array -> (device buffer with GUARD elements of `fill` on both sides, the view of the middle, the host image of the whole)."""
    whole = np.full(values.shape[0] + 2 * GUARD, fill, values.dtype)
    whole[GUARD:GUARD + values.shape[0]] = values
    t = torch.from_numpy(whole.view(np.int16) if values.dtype == np.uint16 else whole).to(dev)
    if values.dtype == np.uint16:
        t = t.view(BF)
    return t, t[GUARD:GUARD + values.shape[0]], whole


def raw(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


def stale_out(n_segs, dev, latch0=100):
    """An `out` of garbage (NaN sums, NaN maximum, a count of -1) whose latches are 100 + t, with two guard records behind it."""
    rec = np.zeros(n_segs + 2, R.STAT_DTYPE)
    rec["grad_sumsq"], rec["param_sumsq"], rec["grad_absmax"], rec["n_nonfinite"] = np.nan, np.nan, np.nan, -1
    rec["n_bad_steps"] = latch0 + np.arange(n_segs + 2)
    return torch.from_numpy(rec.view(np.int64).reshape(-1, 4).copy()).to(dev), rec


def stale_partials(total_chunks, dev):
    rec = np.zeros(total_chunks + 2, R.STAT_DTYPE)
    rec["grad_sumsq"], rec["param_sumsq"], rec["grad_absmax"], rec["n_nonfinite"], rec["n_bad_steps"] = np.nan, np.inf, np.inf, 1 << 40, -3
    return torch.from_numpy(rec.view(np.int64).reshape(-1, 4).copy()).to(dev), rec


@pytest.fixture(scope="module")
def plan(ops, dev):
    p = ops.tensor_stats_plan(SEGS, TOTAL, device=dev)
    assert p["chunk_start"].tolist() == R.plan(SEGS).tolist() and p["total_chunks"] == 6 + 1 + 1 + 2 + 4 + 258   # six segments below a chunk, C - 1, C, C + 1, 3 C + 5, 257 C + 5
    return p


@pytest.mark.parametrize("scale", SCALES, ids=["scale1", "scale_third"])
@pytest.mark.parametrize("round_bf16", (True, False), ids=["round_bf16", "keep_f32"])
@pytest.mark.parametrize("param", ("bf16", "f32"))
def test_every_field_equals_the_restatement_and_nothing_else_is_touched(ops, dev, host, plan, param, round_bf16, scale):
    n_segs, total = plan["n_segs"], plan["total_chunks"]
    gbuf, gview, gwhole = guarded(host["grad"], dev, np.float32(np.nan))         # NaN guards and NaN gaps: one read outside a segment poisons a sum
    pbuf, pview, pwhole = guarded(host[param], dev, np.uint16(0x7FC0) if param == "bf16" else np.float32(np.nan))
    out, out0 = stale_out(n_segs, dev)
    partials, part0 = stale_partials(total, dev)
    ops.tensor_stats(plan, gview, pview, out[:n_segs], partials[:total], grad_round_bf16=round_bf16, grad_scale=scale)
    got = ops.read_tensor_stats(out)
    want = twin(host, param, round_bf16, scale).copy()
    assert np.isfinite(want["grad_sumsq"]).all() and np.isfinite(want["param_sumsq"]).all() and (want["n_nonfinite"] == 0).all()
    want["n_bad_steps"] = out0["n_bad_steps"][:n_segs]                           # no non-finite element: every latch is kept
    assert R.same_records(got[:n_segs], want) == [], f"{param} round {round_bf16} scale {scale}"
    assert (got[0]["grad_sumsq"], got[0]["param_sumsq"], got[0]["grad_absmax"], got[0]["n_nonfinite"]) == (0.0, 0.0, 0.0, 0), "n == 0: all zero"
    assert got[n_segs:].tobytes() == out0[n_segs:].tobytes(), "out was written past its n_segs records"
    assert raw(partials[total:]) == part0[total:].tobytes(), "partials was written past its total_chunks records"
    back = ops.read_tensor_stats(partials, total)
    assert (back["n_bad_steps"] == 0).all() and np.isfinite(back["grad_sumsq"]).all(), "every partial record is rewritten whole"
    assert raw(gbuf) == gwhole.tobytes() and raw(pbuf) == pwhole.tobytes(), "grad or param was written"


def test_one_segments_data_reaches_only_its_own_entry(ops, dev, host, plan):
    n_segs, total = plan["n_segs"], plan["total_chunks"]
    grad, param = torch.from_numpy(host["grad"]).to(dev), torch.from_numpy(host["f32"]).to(dev)
    partials = torch.empty((total, 4), dtype=torch.int64, device=dev)

    def run():
        out = torch.zeros((n_segs, 4), dtype=torch.int64, device=dev)
        ops.tensor_stats(plan, grad, param, out, partials, grad_round_bf16=True, grad_scale=1.0 / 3.0)
        return [raw(out[t]) for t in range(n_segs)]

    before = run()
    assert run() == before, "the same inputs give the same bytes (stale partials do not matter)"
    for t in (2, 7, 10, 11):                                                      # a tail-only segment, a short chunk, several chunks, 258 partials
        off, n = SEGS[t]
        grad[off:off + n] *= 1.5
        param[off:off + n] += 0.25
        after = run()
        assert [i for i in range(n_segs) if after[i] != before[i]] == [t], f"rewriting segment {t}"
        before = after


def test_non_finite_elements_counts_maximum_and_the_latch(ops, dev, host, plan):
    n_segs, total = plan["n_segs"], plan["total_chunks"]
    g = host["grad"].copy()
    planted = {1: [(0, np.nan)], 4: [(4, np.inf)], 8: [(0, -np.inf), (C - 1, np.nan)], 10: [(C + 3, np.nan), (3 * C + 4, np.inf), (17, -np.inf)],
               11: [(256 * C + 9, np.nan)]}
    for t, items in planted.items():
        for o, v in items:
            g[SEGS[t][0] + o] = v
    want = R.tensor_stats(g, host["f32"], SEGS, grad_round_bf16=False)
    assert want["n_nonfinite"].tolist() == [len(planted.get(t, ())) for t in range(n_segs)]
    grad, param = torch.from_numpy(g).to(dev), torch.from_numpy(host["f32"]).to(dev)
    out, partials = ops.tensor_stats_buffers(n_segs, total, dev)
    out[0, 2] = 9 << 32                                                           # the n == 0 segment's latch: kept
    latch = np.zeros(n_segs, np.int32)
    latch[0] = 9
    for call in (1, 2):
        ops.tensor_stats(plan, grad, param, out, partials, grad_round_bf16=False)
        got = ops.read_tensor_stats(out)
        want["n_bad_steps"] = latch + call * (want["n_nonfinite"] > 0)
        assert R.same_records(got, want) == [], f"call {call}"
    assert got["n_bad_steps"].tolist() == [9, 2, 0, 0, 2, 0, 0, 0, 2, 0, 2, 2]
    assert np.isnan(got["grad_sumsq"][1]) and got["grad_sumsq"][4] == np.inf and got["grad_absmax"][1] == 0.0, "a segment of one NaN has no finite element"
    for t in planted:
        keep = np.isfinite(g[SEGS[t][0]:SEGS[t][0] + SEGS[t][1]])
        assert got["grad_absmax"][t] == (np.abs(g[SEGS[t][0]:SEGS[t][0] + SEGS[t][1]][keep]).max() if keep.any() else 0.0)
    # a clean third call: the counts return to zero, the latches stay
    ops.tensor_stats(plan, torch.from_numpy(host["grad"]).to(dev), param, out, partials, grad_round_bf16=False)
    clean = ops.read_tensor_stats(out)
    assert (clean["n_nonfinite"] == 0).all() and clean["n_bad_steps"].tolist() == got["n_bad_steps"].tolist()


@pytest.mark.parametrize("round_bf16", (True, False), ids=["bf16", "f32"])
def test_a_one_entry_table_gives_grad_sumsq_s_slot(ops, dev, round_bf16):
    g = np.random.default_rng(29)
    n_max = 515 * C + 3
    values = (g.standard_normal(n_max) * 10.0 ** g.uniform(-3, 3, n_max)).astype(np.float32)
    grad = torch.from_numpy(values).to(dev)
    slots = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = torch.empty(ops.grad_sumsq_workspace_elems(n_max), dtype=torch.float64, device=dev)
    for n in (C + 1, n_max):
        p = ops.tensor_stats_plan([(0, n)], n_max, device=dev)
        out, partials = ops.tensor_stats_buffers(1, p["total_chunks"], dev)
        ops.tensor_stats(p, grad, grad, out, partials, grad_round_bf16=round_bf16, grad_scale=1.0 / 3.0)
        ops.grad_sumsq(grad, slots, 0, ws, is_bf16=round_bf16, grad_scale=1.0 / 3.0, n=n)
        got = ops.read_tensor_stats(out)[0]
        assert got["grad_sumsq"].tobytes() == slots.cpu().numpy()[0].tobytes(), f"n {n}"
        assert got["param_sumsq"].tobytes() == R.sumsq_of(values[:n]).tobytes()


def test_launch_side_refusals_write_nothing(ops, dev, host, plan):
    _lib = load("openvla-oft_amd._lib")
    handle = _lib.lib()
    n_segs, total = plan["n_segs"], plan["total_chunks"]
    grad, param = torch.from_numpy(host["grad"]).to(dev), torch.from_numpy(host["f32"]).to(dev)
    out, out0 = stale_out(n_segs, dev)
    partials, part0 = stale_partials(total, dev)

    def args():
        return ops.tensor_stats_args(plan, grad, param, out, partials, grad_round_bf16=False)

    cases = []
    for field in ("grad", "param", "segs", "chunk_start", "partials", "out"):
        cases.append((f"null {field}", {field: None}))
    cases += [("n_segs = 0", dict(n_segs=0)), ("n_segs < 0", dict(n_segs=-1)), ("total_chunks < 0", dict(total_chunks=-1)),
              ("grad off by 4 bytes", dict(grad=grad.data_ptr() + 4)), ("param off by 8 bytes", dict(param=param.data_ptr() + 8)),
              ("out off by 4 bytes", dict(out=out.data_ptr() + 4)), ("partials off by 4 bytes", dict(partials=partials.data_ptr() + 4)),
              ("partials one byte short", dict(partials_bytes=32 * total - 1)),
              ("one chunk fewer than the plan", dict(total_chunks=total - 1)), ("one chunk more than the plan", dict(total_chunks=total + 1)),
              ("another table's segment count", dict(n_segs=n_segs - 1))]
    assert handle.ovla_tensor_stats(None, ctypes.c_void_p(ops._stream())) == -1
    for what, change in cases:
        a = args()
        for k, v in change.items():
            setattr(a, k, v)
        assert handle.ovla_tensor_stats(ctypes.byref(a), ctypes.c_void_p(ops._stream())) == -1, what
        assert b"ovla_tensor_stats" in handle.ovla_last_error(), what
    torch.cuda.synchronize()
    assert raw(out) == out0.tobytes() and raw(partials) == part0.tobytes(), "a refused call launches nothing"
    assert handle.ovla_tensor_stats(ctypes.byref(args()), ctypes.c_void_p(ops._stream())) == 0, "the unchanged arguments are accepted"
    assert (ops.read_tensor_stats(out, n_segs)["n_nonfinite"] == 0).all()
