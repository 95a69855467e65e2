"""The per-tensor statistics contract (include/ovla.h "Per-tensor statistics") restated in numpy on top of tests/grad_clip_reference.py.
Independent of the package: the tests compare the kernels and the engine against this file bit for bit.  For segment t = (offset_t, n_t):

    r_i = fp32(g_i * grad_scale), rounded to bf16 (RNE) when grad_round_bf16: grad_clip_reference.seen_gradient, ovla_grad_sumsq's r_i
    grad_sumsq   the sum of double(r_i)^2 in ovla_grad_sumsq's fixed order with the chunks counted from the segment's own start: exactly
                 grad_clip_reference's chunk_partials / final_sum on the segment's elements alone
    param_sumsq  the same sum of double(param_i)^2 (a bf16 parameter widened exactly), same ownership and order
    grad_absmax  max |r_i| over the finite r_i, 0 when there is none (fp32)
    n_nonfinite  the number of r_i that are NaN or +-Inf
    n_bad_steps  the previous value + 1 when n_nonfinite > 0, otherwise the previous value
    plan         chunk_start[t] = the chunks, ceil(n / CHUNK) each, of the segments before t; chunk_start[n_segs] = total_chunks

A segment with n == 0 gives all zeros and keeps n_bad_steps.  Nothing outside a segment is looked at.
"""
import numpy as np

from tests import grad_clip_reference as G

CHUNK = G.CHUNK
PARTIAL_BYTES = 32                  # OVLA_TENSOR_STATS_PARTIAL_BYTES
STAT_DTYPE = np.dtype([("grad_sumsq", "<f8"), ("param_sumsq", "<f8"), ("grad_absmax", "<f4"), ("n_bad_steps", "<i4"), ("n_nonfinite", "<i8")])
assert STAT_DTYPE.itemsize == PARTIAL_BYTES


def plan(segments):
    """chunk_start int32 [n_segs + 1] of a legal table [(offset, n), ...]."""
    counts = [(int(n) + CHUNK - 1) // CHUNK for _, n in segments]
    return np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int32)


def table_error(segments, buffer_n):
    """None for a legal table, else the reason ovla_tensor_stats_plan refuses it."""
    if len(segments) < 1:
        return "n_segs < 1"
    if buffer_n < 0:
        return "buffer_n < 0"
    end = 0
    for off, n in segments:
        if off < 0 or n < 0:
            return "negative"
        if off % 8:
            return "offset % 8"
        if off < end:
            return "not ascending or overlapping"
        if off + n > buffer_n:
            return "past the buffer"
        end = off + n
    return None


def sumsq_of(values):
    """The fixed-order double sum of squares of fp32 values taken as they are (double(x)^2 is exact)."""
    d = np.asarray(values, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return G.final_sum(G.chunk_partials(d * d))


def segment_stats(grad, param, *, grad_scale=1.0, grad_round_bf16=False, n_bad_steps=0):
    """One segment: `grad` fp32 [n], `param` fp32 [n] (a bf16 parameter already widened, G.widen_bf16) -> one STAT_DTYPE record."""
    r = G.seen_gradient(grad, grad_scale, grad_round_bf16)
    finite = np.isfinite(r)
    out = np.zeros((), STAT_DTYPE)
    out["grad_sumsq"] = sumsq_of(r)
    out["param_sumsq"] = sumsq_of(param)
    out["grad_absmax"] = np.abs(r[finite]).max() if finite.any() else np.float32(0.0)
    out["n_nonfinite"] = int((~finite).sum())
    out["n_bad_steps"] = n_bad_steps + int(out["n_nonfinite"] > 0)
    return out


def tensor_stats(grad, param, segments, *, grad_scale=1.0, grad_round_bf16=False, n_bad_steps=None):
    """ovla_tensor_stats over a table: flat `grad` fp32 and `param` fp32 (widened) buffers -> STAT_DTYPE [n_segs].  `n_bad_steps`: the latches
    before the call (default zeros)."""
    before = np.zeros(len(segments), np.int32) if n_bad_steps is None else np.asarray(n_bad_steps, np.int32)
    out = np.zeros(len(segments), STAT_DTYPE)
    for t, (off, n) in enumerate(segments):
        out[t] = segment_stats(grad[off:off + n], param[off:off + n], grad_scale=grad_scale, grad_round_bf16=grad_round_bf16, n_bad_steps=int(before[t]))
    return out


def same_records(got, want):
    """Bit equality of two STAT_DTYPE arrays field by field, a NaN sum matching any NaN; returns the list of (index, field) that differ."""
    bad = []
    for f in STAT_DTYPE.names:
        a, b = np.asarray(got[f]).reshape(-1), np.asarray(want[f]).reshape(-1)
        for i in range(a.shape[0]):
            if a.dtype.kind == "f" and np.isnan(a[i]) and np.isnan(b[i]):
                continue
            if a[i].tobytes() != b[i].tobytes():
                bad.append((i, f))
    return bad
