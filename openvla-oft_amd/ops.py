"""Tensor-level wrappers over the C-ABI (include/ovla.h).  PyTorch is used here only as the owner of device memory
and of the HIP stream; every arithmetic op below is a hand-written gfx950 kernel in libovla_hip.so.  Nothing in this
module falls back to torch math: a missing library or a failed launch raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import threading

import numpy as np
import torch

from . import _lib
from ._lib import STRUCTS

ACT_NONE, ACT_GELU, ACT_RELU, ACT_SILU, ACT_GELU_TANH, ACT_SWIGLU = 0, 1, 2, 3, 4, 5
BF16 = torch.bfloat16

# bench.py sets this to a list to time individual launches with HIP events on the launch stream:
# entries are (kernel_family, start_event, end_event, algorithmic_flops)
PROFILE = None


_WS_BYTES = 96 << 20   # persistent fp32 scratch per device for split-K / hybrid-schedule partial sums (stream-ordered reuse)
_ws_cache = {}
_ws_retired = []       # outgrown workspaces stay allocated: a captured hipGraph (engine.ChunkGraph) has their raw pointers in its kernel arguments


def _workspace(device, nbytes):
    """One scratch buffer per (device, stream): launches on one stream reuse it in stream order; the two vision towers run
    on different streams and must not share partial-sum slabs.  A buffer that has been handed out is never freed: when a call needs more
    than the current one holds, a larger one takes its place for LATER launches and the old one is retired, not released -- graph replays
    recorded earlier keep writing into memory they still own."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        if ws is not None:
            _ws_retired.append(ws)
        ws = torch.empty(max(nbytes, _WS_BYTES) // 4, dtype=torch.float32, device=device)
        _ws_cache[key] = ws
    return ws


# Arrival counters of the in-launch hybrid reduce (ovla_gemm_args.hybrid_counters): one zeroed array per (device, stream), which the kernels
# keep all-zero.  OPT-IN (OVLA_HYBRID_INLAUNCH=1): bit-identical to the separate gemm_hybrid_reduce launch but measured SLOWER on every hybrid
# shape (tools/hybrid_ab.py, profiles/r03_hybrid_inlaunch_ab.txt: 4864 x 4096 x 4096 214 vs 160 us, 608 x 4096 x 4096 67.5 vs 38.5 us) -- the
# agent-scope release each K-part workgroup needs before it signals writes back its XCD's whole L2 (the other tiles' output lines included),
# which costs far more than the 15 us launch it removes.
import os as _os

_HYB_INLAUNCH = _os.environ.get("OVLA_HYBRID_INLAUNCH", "0") == "1"
_HYB_N = 4096
_hyb_cache = {}


def _hybrid_counters(device):
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    c = _hyb_cache.get(key)
    if c is None:
        c = _hyb_cache[key] = torch.zeros(_HYB_N, dtype=torch.int32, device=device)
    return c


def _prof_begin():
    if PROFILE is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _prof_end(e0, family, flops):
    if e0 is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        PROFILE.append((family, e0, e1, flops))


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t) -> int:
    return 0 if t is None else t.data_ptr()


def _chk(t: torch.Tensor, dtype=BF16, name="tensor"):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a device tensor (the HIP path has no CPU fallback)")


def check_device(index: int = 0) -> None:
    _lib.check(_lib.lib().ovla_check_device(index), "ovla_check_device")


# ----------------------------------------------------------------------------------------------------------------------
def gemm(a, b, *, out=None, bias=None, act=ACT_NONE, residual=None, colscale=None, c_pre=None, a2=None, b2=None,
         k2_group_n=0, film=None, split_k=1, tile=0, alpha=1.0, a_group_n=0, dact=None, rope=None, rowsq_out=None, rowscale=None, schedule=None):
    """out[M,N] = epilogue(a[M,K] @ b[N,K]^T (+ a2[M,G*K2] @ b2[N,K2]^T)); all bf16 2-D, last dim contiguous.
    schedule=(tile, splits): run under exactly this fixed schedule (ovla_gemm_bf16_fixed) instead of the planner's or the cost model's choice."""
    _chk(a, name="a"); _chk(b, name="b")
    M, K = a.shape
    N = b.shape[0]
    if a_group_n:   # block-diagonal: a is [M, G*K], b is [G*a_group_n, K]
        K = b.shape[1]
        assert a.shape[1] == (N // a_group_n) * K, f"gemm(block-diagonal): {a.shape} vs {b.shape}"
    assert b.shape[1] == K, f"gemm: K mismatch {a.shape} x {b.shape}"
    assert a.stride(1) == 1 and b.stride(1) == 1
    out_cols = 2 * N if (dact is not None and dact[0] == "swiglu") else (N // 2 if act == ACT_SWIGLU else N)   # ACT_SWIGLU: b = [gate; up], out = silu(gate) * up
    if out is None:
        out = torch.empty((M, out_cols), dtype=BF16, device=a.device)
    assert out.shape == (M, out_cols) and out.stride(1) == 1
    g = STRUCTS["ovla_gemm_args"]()
    g.A, g.lda, g.B, g.ldb = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0)
    g.C, g.ldc = out.data_ptr(), out.stride(0)
    if a2 is not None:
        assert b2 is not None and a2.stride(1) == 1 and b2.stride(1) == 1 and b2.shape[0] == N and a2.shape[0] == M
        g.A2, g.lda2, g.B2, g.ldb2, g.K2 = a2.data_ptr(), a2.stride(0), b2.data_ptr(), b2.stride(0), b2.shape[1]
        g.k2_group_n = k2_group_n
    if c_pre is not None:
        assert c_pre.shape == (M, N) and c_pre.stride(0) == (N if act == ACT_SWIGLU else out.stride(0))   # ACT_SWIGLU: c_pre = the contiguous [M, 2F] projection output
        g.C_pre = c_pre.data_ptr()
    if bias is not None:
        assert bias.numel() == N
        g.bias = bias.data_ptr()
    if colscale is not None:
        assert colscale.numel() == N
        g.colscale = colscale.data_ptr()
    if residual is not None:
        assert residual.shape == (M, N) and residual.stride(1) == 1
        g.residual, g.ldr = residual.data_ptr(), residual.stride(0)
    if film is not None:
        gamma, beta, rows = film
        assert gamma.shape[-1] == N and gamma.is_contiguous() and beta.is_contiguous()
        g.film_gamma, g.film_beta, g.film_rows = gamma.data_ptr(), beta.data_ptr(), rows
    if dact is not None:   # backward epilogue: ("act", z, act_id) or ("swiglu", gu)
        src = dact[1]
        assert src.stride(1) == 1 and src.shape == (M, out_cols) and src.dtype == BF16
        g.dact_src, g.ld_dact = src.data_ptr(), src.stride(0)
        g.dact_mode, g.dact_act = (2, ACT_SILU) if dact[0] == "swiglu" else (1, dact[2])
    if rope is not None:   # (cos, sin, S, cols): RoPE on output columns [0, cols) (q | k heads of a fused q|k|v projection), head_dim 128
        cos, sin, rS, rcols = rope
        assert cos.shape[1] == 64 and cos.shape[0] >= rS and cos.is_contiguous() and sin.is_contiguous()
        g.rope_cos, g.rope_sin, g.rope_S, g.rope_cols = cos.data_ptr(), sin.data_ptr(), rS, rcols
    if rowsq_out is not None:   # RMSNorm fold, producer side: fp32 [M, N / 64] sums of squares of the output's 64-column groups
        assert rowsq_out.dtype == torch.float32 and rowsq_out.shape == (M, N // 64) and rowsq_out.is_contiguous()
        g.rowsq_out = rowsq_out.data_ptr()
    if rowscale is not None:    # consumer side: (parts fp32 [M, K / 64], eps, rstd scratch fp32 [M]): C = epilogue(rstd[m] * alpha * acc)
        parts, eps, rbuf = rowscale
        assert parts.dtype == torch.float32 and parts.shape == (M, K // 64) and parts.is_contiguous() and rbuf.dtype == torch.float32 and rbuf.numel() >= M
        g.rowscale_part, g.rowscale_slots, g.rowscale_eps, g.rowscale_r = parts.data_ptr(), K // 64, eps, rbuf.data_ptr()
    if schedule is not None:   # the caller's fixed schedule: the library refuses what it cannot run (block-diagonal mode, backward epilogues, tile / split_k)
        sched = STRUCTS["ovla_gemm_schedule"]()
        sched.tile, sched.splits = schedule
        g.M, g.N, g.K, g.act, g.split_k, g.tile, g.alpha, g.a_group_n = M, N, K, act, split_k, tile, alpha, a_group_n
        ws = _workspace(a.device, max(gemm_fixed_workspace_bytes(M, N, sched), _WS_BYTES))
        g.workspace, g.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        e0 = _prof_begin()
        _lib.check(_lib.lib().ovla_gemm_bf16_fixed(ctypes.byref(g), ctypes.byref(sched), _stream()), "ovla_gemm_bf16_fixed")
        _prof_end(e0, f"gemm_fixed_t{sched.tile}s{sched.splits}", 2.0 * M * N * (K + g.K2))
        return out
    if getattr(_mode, "invariant", False) and dact is None and not a_group_n:   # batch-invariant mode: the caller's tile / split_k give way to the fixed schedule
        g.M, g.N, g.K, g.act, g.split_k, g.tile, g.alpha = M, N, K, act, 0, 0, alpha
        general = (act not in (ACT_NONE, ACT_SWIGLU) or c_pre is not None or colscale is not None or film is not None
                   or (bias is not None and bias.data_ptr() % 16) or (residual is not None and (residual.data_ptr() % 16 or residual.stride(0) % 8)))
        epi = ((EPI_ROPE if rope is not None else 0) | (EPI_ROWSCALE if rowscale is not None else 0) | (EPI_ROWSQ if rowsq_out is not None else 0)
               | (EPI_SWIGLU if act == ACT_SWIGLU else 0) | (EPI_GENERAL if general else 0))
        sched = _fixed_schedule_struct(N, K, g.K2, g.k2_group_n, epi)
        ws = _workspace(a.device, max(gemm_fixed_workspace_bytes(M, N, sched), _WS_BYTES))
        g.workspace, g.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        e0 = _prof_begin()
        _lib.check(_lib.lib().ovla_gemm_bf16_fixed(ctypes.byref(g), ctypes.byref(sched), _stream()), "ovla_gemm_bf16_fixed")
        _prof_end(e0, f"gemm_fixed_t{sched.tile}s{sched.splits}", 2.0 * M * N * (K + g.K2))
        return out
    g.M, g.N, g.K, g.act, g.split_k, g.tile, g.alpha, g.a_group_n = M, N, K, act, split_k, tile, alpha, a_group_n
    ws = _workspace(a.device, max(4 * split_k * M * N if split_k > 1 else 0, _WS_BYTES))
    g.workspace, g.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    if _HYB_INLAUNCH:
        g.hybrid_counters, g.n_hybrid_counters = _hybrid_counters(a.device).data_ptr(), _HYB_N
    e0 = _prof_begin()
    _lib.call("ovla_gemm_bf16", g, _stream())
    if e0 is not None:
        _prof_end(e0, _gemm_family(g), 2.0 * M * N * (K + (b2.shape[1] if b2 is not None else 0)))
    return out


def _gemm_family(g):
    """Profiling only: which kernel instance `ovla_gemm_bf16` runs for these arguments ("gemm_nt_t17" = gemm_nt_kernel<256,256,2,4>, "gemm_nt_t18" = the
    4-wave gemm_nt_w4_kernel, ...), from the library's own decision code (ovla_gemm_resolved_tile) -- so bench.py can report the dominant instance by itself."""
    import ctypes

    t = ctypes.c_int32()
    _lib.check(_lib.lib().ovla_gemm_resolved_tile(ctypes.byref(g), ctypes.byref(t)), "ovla_gemm_resolved_tile")
    tile = t.value % 100 if t.value >= 100 else t.value
    return f"gemm_nt_t18k{g.K2 // 32}" if tile == 18 else f"gemm_nt_t{tile}"   # the 4-wave kernel is one instantiation per K-extension width


def gemm_tn(x, y, *, out=None, alpha=1.0, accumulate=True, out_dtype=torch.float32):
    """out[P,Q] (+)= alpha * x[M,P]^T @ y[M,Q].  accumulate=True: fp32 accumulation into `out`, in a fixed order (bit-reproducible)."""
    _chk(x, name="x"); _chk(y, name="y")
    M, P = x.shape
    Q = y.shape[1]
    assert y.shape[0] == M and x.stride(1) == 1 and y.stride(1) == 1
    if out is None:
        out = torch.zeros((P, Q), dtype=out_dtype, device=x.device) if accumulate else torch.empty((P, Q), dtype=out_dtype, device=x.device)
    assert out.shape == (P, Q) and out.stride(1) == 1
    g = STRUCTS["ovla_gemm_tn_args"]()
    g.X, g.ldx, g.Y, g.ldy, g.C, g.ldc = x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), out.data_ptr(), out.stride(0)
    g.M, g.P, g.Q, g.alpha = M, P, Q, alpha
    if accumulate:
        assert out.dtype == torch.float32
        g.out_mode = 0
    else:
        g.out_mode = 1 if out.dtype == torch.float32 else 2
    ws = _tn_workspace(g, 1, x.device)
    e0 = _prof_begin()
    _lib.call("ovla_gemm_tn_bf16", g, _stream())
    _prof_end(e0, "gemm_tn", 2.0 * M * P * Q)
    return out


_TN_WS_FLOATS = {}


def _tn_workspace(g, group_size, device):
    """The fp32 split-partial workspace one TN problem needs (None when it is not split); sets g.W.  Allocated on the current stream, so the
    caching allocator hands it to nothing else before the launch that uses it has run."""
    import ctypes

    key = (g.M, g.P, g.Q, g.out_mode, group_size)   # everything the split plan depends on
    n = _TN_WS_FLOATS.get(key)
    if n is None:
        n = _lib.lib().ovla_gemm_tn_workspace_floats(ctypes.byref(g), group_size)
        if n < 0:
            raise _lib.OvlaError(f"ovla_gemm_tn_workspace_floats: invalid problem ({_lib.lib().ovla_last_error().decode()})")
        _TN_WS_FLOATS[key] = n
    if n == 0:
        return None
    ws = torch.empty(n, dtype=torch.float32, device=device)
    g.W = ws.data_ptr()
    return ws


TN_MAX_GROUP = 4   # OVLA_TN_MAX_GROUP (ovla.h)


def gemm_tn_grouped(problems):
    """problems: list of (x, y, out_fp32) with out accumulated (+=).  One launch for up to 4 TN GEMMs."""
    import ctypes

    n = len(problems)
    arr = (STRUCTS["ovla_gemm_tn_args"] * n)()
    ws = []   # kept alive until the launch is enqueued
    flops = 0.0
    for i, (x, y, out) in enumerate(problems):
        _chk(x, name="x"); _chk(y, name="y")
        M, P = x.shape
        Q = y.shape[1]
        assert y.shape[0] == M and x.stride(1) == 1 and y.stride(1) == 1 and out.shape == (P, Q) and out.dtype == torch.float32
        g = arr[i]
        g.X, g.ldx, g.Y, g.ldy, g.C, g.ldc = x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), out.data_ptr(), out.stride(0)
        g.M, g.P, g.Q, g.alpha, g.out_mode = M, P, Q, 1.0, 0
        ws.append(_tn_workspace(g, n, x.device))
        flops += 2.0 * M * P * Q
    e0 = _prof_begin()
    _lib.check(_lib.lib().ovla_gemm_tn_grouped(arr, n, _stream()), "ovla_gemm_tn_grouped")
    _prof_end(e0, "gemm_tn", flops)


def row_sumsq(x, out=None):
    """out[m, j] = sum of squares of x[m, 64 j : 64 j + 64] (fp32 [rows, dim / 64]): the first decoder layer's RMSNorm-fold input."""
    _chk(x, name="x")
    rows, dim = x.shape
    assert x.stride(1) == 1 and dim % 64 == 0
    if out is None:
        out = torch.empty((rows, dim // 64), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().ovla_row_sumsq(x.data_ptr(), x.stride(0), out.data_ptr(), rows, dim, _stream()), "ovla_row_sumsq")
    return out


def gemm_plan(M, N, K, K2=0, k2_group_n=0, workspace_bytes=_WS_BYTES):
    """The schedule `tile = 0` would pick (ovla_gemm_plan, host only): (tile id, full tiles, remainder tiles, remainder splits, estimated seconds)."""
    import ctypes

    t, f, r, sp, est = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
    _lib.check(_lib.lib().ovla_gemm_plan(M, N, K, K2, k2_group_n, ctypes.c_int64(workspace_bytes), ctypes.byref(t), ctypes.byref(f), ctypes.byref(r),
                                         ctypes.byref(sp), ctypes.byref(est)), "ovla_gemm_plan")
    return t.value, f.value, r.value, sp.value, est.value


# ----------------------------------------------------------------------------------------------------------------------
# Batch-invariant mode (ovla.h: ovla_gemm_bf16_fixed).  Inside `with batch_invariant():` every forward GEMM runs under the fixed schedule of its
# (N, K, K2, k2_group_n, epilogue) class instead of the planner's M-dependent one, so an output row's bits do not depend on how many rows share
# the launch: the batched inference API (predict_action_batch) gives each observation the same actions whatever else is in the batch.
# OVLA_BATCH_INVARIANT=0 leaves the batched API on the planner's schedules (A/B measurement only: results then depend on the batch).
EPI_ROPE, EPI_ROWSCALE, EPI_SWIGLU, EPI_GENERAL, EPI_ROWSQ = 1, 2, 4, 8, 16
BATCH_INVARIANT_DEFAULT = _os.environ.get("OVLA_BATCH_INVARIANT", "1") != "0"
_mode = threading.local()   # per thread, like the library's own schedule pointer: another thread's GEMMs keep the planner
_fixed_cache = {}


@contextlib.contextmanager
def batch_invariant(on: bool = True):
    prev = getattr(_mode, "invariant", False)
    _mode.invariant = bool(on)
    try:
        yield
    finally:
        _mode.invariant = prev


def batch_invariant_enabled() -> bool:
    return getattr(_mode, "invariant", False)


def _fixed_schedule_struct(N, K, K2=0, k2_group_n=0, epi=0):
    key = (N, K, K2, k2_group_n, epi)
    s = _fixed_cache.get(key)
    if s is None:
        s = STRUCTS["ovla_gemm_schedule"]()
        _lib.check(_lib.lib().ovla_gemm_fixed_schedule(N, K, K2, k2_group_n, epi, ctypes.byref(s)), "ovla_gemm_fixed_schedule")
        _fixed_cache[key] = s
    return s


def gemm_fixed_schedule(N, K, K2=0, k2_group_n=0, epi=0):
    """The fixed schedule (tile id, splits) of a problem class (ovla_gemm_fixed_schedule, host only; independent of M by construction)."""
    s = _fixed_schedule_struct(N, K, K2, k2_group_n, epi)
    return s.tile, s.splits


def gemm_fixed_workspace_bytes(M, N, sched):
    if isinstance(sched, tuple):
        s = STRUCTS["ovla_gemm_schedule"]()
        s.tile, s.splits = sched
        sched = s
    return int(_lib.lib().ovla_gemm_fixed_workspace_bytes(M, N, ctypes.byref(sched)))


def transpose_table(pairs, device):
    """Builds the device descriptor table for transpose_batched from [(src, dst)] (2-D bf16 tensors that never move)."""
    import ctypes

    T = STRUCTS["ovla_transpose_args"]
    arr = (T * len(pairs))()
    starts = [0]
    for i, (src, dst) in enumerate(pairs):
        rows, cols = src.shape
        assert dst.shape == (cols, rows) and src.stride(1) == 1 and dst.stride(1) == 1
        arr[i].src, arr[i].dst, arr[i].rows, arr[i].cols, arr[i].lds, arr[i].ldd = src.data_ptr(), dst.data_ptr(), rows, cols, src.stride(0), dst.stride(0)
        starts.append(starts[-1] + ((rows + 63) // 64) * ((cols + 63) // 64))
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    tile_start = torch.tensor(starts, dtype=torch.int32).to(device)
    return dict(table=raw, tile_start=tile_start, n=len(pairs), total=starts[-1], keep=pairs)


def transpose_batched(tab):
    import ctypes

    ptr = ctypes.cast(ctypes.c_void_p(tab["table"].data_ptr()), ctypes.POINTER(STRUCTS["ovla_transpose_args"]))
    _lib.check(_lib.lib().ovla_transpose_batched(ptr, tab["tile_start"].data_ptr(), tab["n"], tab["total"], _stream()), "ovla_transpose_batched")


def copy_entry(src, dst):
    """One ovla_copy_table entry (src, dst, src_ld_bytes, dst_ld_bytes, rows, row_bytes) for two tensors of the same dtype and shape, 1-D (one
    row) or 2-D with unit inner stride (a strided view of a wider tensor is what the table is for)."""
    assert src.dtype == dst.dtype and src.shape == dst.shape and src.dim() in (1, 2) and src.stride(-1) == 1 and dst.stride(-1) == 1
    es = src.element_size()
    if src.dim() == 1:
        return (src.data_ptr(), dst.data_ptr(), src.numel() * es, dst.numel() * es, 1, src.numel() * es)
    rows, cols = src.shape
    if src.stride(0) == cols and dst.stride(0) == cols:   # both contiguous: one long row
        return (src.data_ptr(), dst.data_ptr(), rows * cols * es, rows * cols * es, 1, rows * cols * es)
    return (src.data_ptr(), dst.data_ptr(), src.stride(0) * es, dst.stride(0) * es, rows, cols * es)


def copy_table_build(entries, device, keep=None):
    """The device table of ovla_copy_table from [(src, dst, src_ld_bytes, dst_ld_bytes, rows, row_bytes)] (addresses and byte counts; the
    tensors behind them never move: `keep` holds references).  ovla_copy_table_plan validates the entries and counts the tiles."""
    T = STRUCTS["ovla_copy_entry"]
    n = len(entries)
    arr = (T * max(n, 1))()
    for i, (src, dst, sld, dld, rows, row_bytes) in enumerate(entries):
        arr[i].src, arr[i].dst, arr[i].src_ld_bytes, arr[i].dst_ld_bytes, arr[i].rows, arr[i].row_bytes = src, dst, sld, dld, rows, row_bytes
    starts = (ctypes.c_int32 * (n + 1))()
    _lib.check(_lib.lib().ovla_copy_table_plan(arr, n, ctypes.cast(starts, ctypes.c_void_p)), "ovla_copy_table_plan")
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    tile_start = torch.tensor(list(starts), dtype=torch.int32).to(device)
    nbytes = sum(e[4] * e[5] for e in entries)
    return dict(table=raw, tile_start=tile_start, n=n, total=int(starts[n]), nbytes=nbytes, keep=keep)


_copy_tables = {}


def copy_table(entries, device=None):
    """ovla_copy_table on the current stream: every entry's rows x row_bytes rectangle, device to device, in ONE launch.  `entries`: a table
    from copy_table_build, or the entry tuples themselves -- their table is then built on first use and cached by value."""
    if isinstance(entries, dict):
        tab = entries
    else:
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        key = (device, tuple(tuple(int(v) for v in e) for e in entries))
        tab = _copy_tables.get(key)
        if tab is None:
            if len(_copy_tables) >= 64:   # by-value tables are for tools and tests; the engine keeps its own per (policy, slot)
                _copy_tables.pop(next(iter(_copy_tables)))
            tab = _copy_tables[key] = copy_table_build(key[1], device)
    ptr = ctypes.cast(ctypes.c_void_p(tab["table"].data_ptr()), ctypes.POINTER(STRUCTS["ovla_copy_entry"]))
    _lib.check(_lib.lib().ovla_copy_table(ptr, tab["tile_start"].data_ptr(), tab["n"], tab["total"], _stream()), "ovla_copy_table")
    return tab


def colsum(x, out):
    """out[n] += sum_m x[m,n]  (fp32 accumulate)."""
    _chk(x); _chk(out, torch.float32)
    g = STRUCTS["ovla_colsum_args"]()
    g.X, g.ldx, g.out, g.M, g.N = x.data_ptr(), x.stride(0), out.data_ptr(), x.shape[0], x.shape[1]
    _lib.call("ovla_colsum_bf16", g, _stream())
    return out


# ----------------------------------------------------------------------------------------------------------------------
def attn_fwd(q, k, v, B, S, H, hd, *, kv_len=None, causal=False, scale=None, out=None):
    """q/k/v: 2-D views [B*S, >=H*hd] (row stride arbitrary, heads contiguous).  Returns (out [B*S, H*hd], lse [B,H,S])."""
    for t in (q, k, v):
        _chk(t)
        assert t.stride(1) == 1 and t.shape[0] == B * S
    if out is None:
        out = torch.empty((B * S, H * hd), dtype=BF16, device=q.device)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    g = STRUCTS["ovla_attn_fwd_args"]()
    g.Q, g.K, g.V, g.q_stride, g.k_stride, g.v_stride = q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), v.stride(0)
    g.O, g.o_stride, g.lse, g.kv_len = out.data_ptr(), out.stride(0), lse.data_ptr(), _p(kv_len)
    g.B, g.H, g.S, g.head_dim, g.causal = B, H, S, hd, int(causal)
    g.scale = float(scale if scale is not None else hd ** -0.5)
    e0 = _prof_begin()
    _lib.call("ovla_attn_fwd", g, _stream())
    _prof_end(e0, "attn_fwd", 4.0 * B * H * S * S * hd * (0.5 if causal else 1.0))
    return out, lse


def attn_bwd(q, k, v, o, do, lse, B, S, H, hd, *, kv_len=None, causal=False, scale=None, dq=None, dk=None, dv=None, rope=None):
    """`rope=(cos, sin)` (ovla_rope_table): dq / dk come out with the inverse RoPE rotation applied (gradients w.r.t. the pre-RoPE q / k)."""
    for t in (q, k, v, o, do):
        _chk(t)
        assert t.stride(1) == 1
    dev = q.device
    if dq is None:
        dq = torch.empty((B * S, H * hd), dtype=BF16, device=dev)
    if dk is None:
        dk = torch.empty((B * S, H * hd), dtype=BF16, device=dev)
    if dv is None:
        dv = torch.empty((B * S, H * hd), dtype=BF16, device=dev)
    delta = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    g = STRUCTS["ovla_attn_bwd_args"]()
    g.Q, g.K, g.V, g.q_stride, g.k_stride, g.v_stride = q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), v.stride(0)
    g.O, g.dO, g.o_stride, g.do_stride = o.data_ptr(), do.data_ptr(), o.stride(0), do.stride(0)
    g.lse, g.delta = lse.data_ptr(), delta.data_ptr()
    g.dQ, g.dK, g.dV, g.dq_stride, g.dk_stride, g.dv_stride = dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dq.stride(0), dk.stride(0), dv.stride(0)
    g.kv_len = _p(kv_len)
    g.B, g.H, g.S, g.head_dim, g.causal = B, H, S, hd, int(causal)
    g.scale = float(scale if scale is not None else hd ** -0.5)
    if rope is not None:
        assert rope[0].shape[0] >= S and rope[0].shape[1] == hd // 2 and rope[0].is_contiguous() and rope[1].is_contiguous()
        g.rope_cos, g.rope_sin = rope[0].data_ptr(), rope[1].data_ptr()
    e0 = _prof_begin()
    _lib.call("ovla_attn_bwd", g, _stream())
    _prof_end(e0, "attn_bwd", 10.0 * B * H * S * S * hd * (0.5 if causal else 1.0))
    return dq, dk, dv


def attn_probs(q, k, lse, B, S, H, hd, *, rows=None, kv_len=None, causal=False, scale=None, per_head=False, mean=True, out=None):
    """The attention probabilities of the query rows `rows` (int32 device tensor of flattened rows b*S+s; None: all B*S rows), recomputed
    from the q / k views and the `lse` of an `attn_fwd` call with the same kv_len, causal and scale.  Returns (P fp32 [R, H, S] or None,
    P_mean fp32 [R, S] or None); `out=(P, P_mean)` supplies the buffers (either may be None).  Masked keys are exactly 0; a row index
    outside [0, B*S) gives a zero row."""
    for t in (q, k):
        _chk(t)
        assert t.stride(1) == 1 and t.shape[0] == B * S
    _chk(lse, torch.float32, "lse")
    assert lse.is_contiguous() and lse.numel() == B * H * S
    if rows is not None:
        _chk(rows, torch.int32, "rows")
        assert rows.dim() == 1 and rows.is_contiguous()
    R = B * S if rows is None else rows.numel()
    P, Pm = out if out is not None else (None, None)
    if out is None:
        if not (per_head or mean):
            raise ValueError("attn_probs: at least one of per_head and mean must be set")
        if per_head:
            P = torch.empty((R, H, S), dtype=torch.float32, device=q.device)
        if mean:
            Pm = torch.empty((R, S), dtype=torch.float32, device=q.device)
    for t, shape, name in ((P, (R, H, S), "P"), (Pm, (R, S), "P_mean")):
        if t is not None:
            _chk(t, torch.float32, name)
            assert tuple(t.shape) == shape and t.is_contiguous(), f"{name}: expected contiguous {shape}, got {tuple(t.shape)}"
    g = STRUCTS["ovla_attn_probs_args"]()
    g.Q, g.K, g.q_stride, g.k_stride = q.data_ptr(), k.data_ptr(), q.stride(0), k.stride(0)
    g.lse, g.kv_len, g.rows, g.P, g.P_mean = lse.data_ptr(), _p(kv_len), _p(rows), _p(P), _p(Pm)
    g.B, g.H, g.S, g.R, g.head_dim, g.causal = B, H, S, R, hd, int(causal)
    g.scale = float(scale if scale is not None else hd ** -0.5)
    e0 = _prof_begin()
    _lib.call("ovla_attn_probs", g, _stream())
    _prof_end(e0, "attn_probs", 2.0 * R * H * S * hd)
    return P, Pm


# ----------------------------------------------------------------------------------------------------------------------
def norm_fwd(x, weight, bias=None, *, eps, rms, out=None, save_stats=True):
    _chk(x); _chk(weight)
    rows, dim = x.shape
    assert x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if (save_stats and not rms) else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    g = STRUCTS["ovla_norm_fwd_args"]()
    g.x, g.y, g.weight, g.bias, g.mean, g.rstd = x.data_ptr(), out.data_ptr(), weight.data_ptr(), _p(bias), _p(mean), _p(rstd)
    g.rows, g.dim, g.eps, g.is_rms = rows, dim, eps, int(rms)
    _lib.call("ovla_norm_fwd", g, _stream())
    return out, mean, rstd


def norm_bwd(x, dy, weight, mean, rstd, *, rms, dx=None, dx_accum=False, dweight=None, dbias=None):
    _chk(x); _chk(dy)
    rows, dim = x.shape
    assert x.is_contiguous() and dy.is_contiguous()
    if dx is None:
        assert not dx_accum
        dx = torch.empty_like(x)
    g = STRUCTS["ovla_norm_bwd_args"]()
    g.x, g.dy, g.weight, g.mean, g.rstd, g.dx = x.data_ptr(), dy.data_ptr(), weight.data_ptr(), _p(mean), rstd.data_ptr(), dx.data_ptr()
    g.dweight, g.dbias, g.rows, g.dim, g.is_rms, g.dx_accum = _p(dweight), _p(dbias), rows, dim, int(rms), int(dx_accum)
    _lib.call("ovla_norm_bwd", g, _stream())
    return dx


def rope_table(S, hd, theta, device):
    cos = torch.empty((S, hd // 2), dtype=BF16, device=device)
    sin = torch.empty((S, hd // 2), dtype=BF16, device=device)
    _lib.check(_lib.lib().ovla_rope_table(cos.data_ptr(), sin.data_ptr(), S, hd, theta, _stream()), "ovla_rope_table")
    return cos, sin


def rope_(qk, S, n_heads, hd, cos, sin, inverse=False):
    """In place on the first n_heads*hd columns of qk [rows, ld]."""
    _chk(qk)
    g = STRUCTS["ovla_rope_args"]()
    g.qk, g.ld, g.rows, g.S, g.n_heads, g.head_dim = qk.data_ptr(), qk.stride(0), qk.shape[0], S, n_heads, hd
    g.cos_table, g.sin_table, g.inverse = cos.data_ptr(), sin.data_ptr(), int(inverse)
    _lib.call("ovla_rope", g, _stream())
    return qk


def swiglu_fwd(gu, out=None):
    _chk(gu)
    rows, F2 = gu.shape
    h = torch.empty((rows, F2 // 2), dtype=BF16, device=gu.device) if out is None else out
    assert h.shape == (rows, F2 // 2) and h.dtype == BF16 and h.is_contiguous()
    g = STRUCTS["ovla_swiglu_fwd_args"]()
    g.gu, g.h, g.rows, g.F = gu.data_ptr(), h.data_ptr(), rows, F2 // 2
    _lib.call("ovla_swiglu_fwd", g, _stream())
    return h


def swiglu_bwd(gu, dh, out=None):
    _chk(gu); _chk(dh)
    rows, F2 = gu.shape
    dgu = torch.empty_like(gu) if out is None else out
    assert dgu.shape == gu.shape and dgu.dtype == BF16 and dgu.is_contiguous()
    g = STRUCTS["ovla_swiglu_bwd_args"]()
    g.gu, g.dh, g.dgu, g.rows, g.F = gu.data_ptr(), dh.data_ptr(), dgu.data_ptr(), rows, F2 // 2
    _lib.call("ovla_swiglu_bwd", g, _stream())
    return dgu


def act_bwd(z, dh, act, out=None):
    _chk(z); _chk(dh)
    assert z.is_contiguous() and dh.is_contiguous()
    dz = torch.empty_like(z) if out is None else out
    assert dz.shape == z.shape and dz.dtype == BF16 and dz.is_contiguous()
    g = STRUCTS["ovla_act_bwd_args"]()
    g.z, g.dh, g.dz, g.n, g.act = z.data_ptr(), dh.data_ptr(), dz.data_ptr(), z.numel(), act
    _lib.call("ovla_act_bwd", g, _stream())
    return dz


def add(a, b=None, out=None):
    _chk(a)
    if out is None:
        out = torch.empty_like(a)
    g = STRUCTS["ovla_add_args"]()
    g.a, g.b, g.out, g.n = a.data_ptr(), _p(b), out.data_ptr(), a.numel()
    _lib.call("ovla_add_bf16", g, _stream())
    return out


def colscale(x, scale, out=None):
    _chk(x)
    if out is None:
        out = torch.empty_like(x)
    g = STRUCTS["ovla_colscale_args"]()
    g.x, g.scale, g.out, g.rows, g.dim = x.data_ptr(), scale.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1]
    _lib.call("ovla_colscale_bf16", g, _stream())
    return out


# ----------------------------------------------------------------------------------------------------------------------
def im2col(pixels, c0, patch, k_padded, n_img=1, img_cstride=6):
    _chk(pixels)
    B, C, H, W = pixels.shape
    assert pixels.is_contiguous()
    out = torch.empty((B * n_img * (H // patch) * (W // patch), k_padded), dtype=BF16, device=pixels.device)
    g = STRUCTS["ovla_im2col_args"]()
    g.pixels, g.out, g.ldo, g.B, g.C_total, g.c0, g.H, g.W, g.patch = pixels.data_ptr(), out.data_ptr(), k_padded, B, C, c0, H, W, patch
    g.n_img, g.img_cstride = n_img, img_cstride
    _lib.call("ovla_im2col", g, _stream())
    return out


def vit_embed(patches, pos, prefix, B, n_patches, dim, out=None):
    n_prefix = 0 if prefix is None else prefix.shape[0]
    tokens = torch.empty((B * (n_patches + n_prefix), dim), dtype=BF16, device=patches.device) if out is None else out
    assert tokens.shape == (B * (n_patches + n_prefix), dim) and tokens.dtype == BF16 and tokens.is_contiguous()
    g = STRUCTS["ovla_vit_embed_args"]()
    g.patches, g.pos, g.prefix, g.tokens = patches.data_ptr(), pos.data_ptr(), _p(prefix), tokens.data_ptr()
    g.B, g.n_patches, g.n_prefix, g.dim = B, n_patches, n_prefix, dim
    _lib.call("ovla_vit_embed", g, _stream())
    return tokens


def copy_rows(src, dst, B, rows, dim, *, src_batch_stride, src_row0, src_ld, dst_batch_stride, dst_row0, dst_ld, dst_col0=0,
              accumulate=False):
    g = STRUCTS["ovla_copy_rows_args"]()
    g.src, g.dst, g.B, g.rows, g.dim = src.data_ptr(), dst.data_ptr(), B, rows, dim
    g.src_batch_stride, g.src_row0, g.src_ld = src_batch_stride, src_row0, src_ld
    g.dst_batch_stride, g.dst_row0, g.dst_ld, g.dst_col0, g.accumulate = dst_batch_stride, dst_row0, dst_ld, dst_col0, int(accumulate)
    _lib.call("ovla_copy_rows", g, _stream())
    return dst


def film_bwd(dy, x_pre, gamma, dgamma, dbeta, B, rows_per_batch):
    """In place: dy <- dy * (1 + gamma[b]); accumulates dgamma / dbeta (fp32 [B, dim])."""
    g = STRUCTS["ovla_film_bwd_args"]()
    g.dy, g.x_pre, g.gamma, g.dgamma, g.dbeta = dy.data_ptr(), x_pre.data_ptr(), gamma.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr()
    g.B, g.rows_per_batch, g.dim = B, rows_per_batch, dy.shape[1]
    _lib.call("ovla_film_bwd", g, _stream())
    return dy


def masked_mean(x, row_mask, B, L, dim):
    out = torch.empty((B, dim), dtype=BF16, device=x.device)
    g = STRUCTS["ovla_masked_mean_args"]()
    g.x, g.row_mask, g.out, g.B, g.L, g.dim = x.data_ptr(), row_mask.data_ptr(), out.data_ptr(), B, L, dim
    _lib.call("ovla_masked_mean", g, _stream())
    return out


def language_average(ids, labels, table, out, *, action_token_begin=31743):
    """out[:B] = mean of table[ids] over the non-action text positions (ovla.h: ovla_language_average); ids / labels int64 [B, L] on the device."""
    B, L = ids.shape
    assert ids.dtype == torch.int64 and labels.dtype == torch.int64 and ids.is_contiguous() and labels.is_contiguous() and ids.is_cuda and labels.is_cuda
    assert out.shape[0] >= B and out.shape[1] == table.shape[1] and out.is_contiguous()
    g = STRUCTS["ovla_language_average_args"]()
    g.ids, g.labels, g.embed_table, g.out = ids.data_ptr(), labels.data_ptr(), table.data_ptr(), out.data_ptr()
    g.B, g.L, g.D, g.vocab, g.action_token_begin = B, L, table.shape[1], table.shape[0], action_token_begin
    _lib.call("ovla_language_average", g, _stream())
    return out


def language_average_ragged(ids, labels, lens, table, out, *, action_token_begin=31743):
    """language_average of a right-padded batch in one launch (ovla.h: ovla_language_average_ragged): row b averages positions i < lens[b]
    only; out[b] is bit for bit language_average(ids[b:b+1, :lens[b]], labels[b:b+1, :lens[b]]).  lens int32 [B] on the device, each in [1, L]."""
    B, L = ids.shape
    assert ids.dtype == torch.int64 and labels.dtype == torch.int64 and ids.is_contiguous() and labels.is_contiguous() and ids.is_cuda and labels.is_cuda
    assert labels.shape == ids.shape and lens.dtype == torch.int32 and lens.numel() == B and lens.is_contiguous() and lens.is_cuda
    assert out.shape[0] >= B and out.shape[1] == table.shape[1] and out.is_contiguous()
    g = STRUCTS["ovla_language_average_ragged_args"]()
    g.ids, g.labels, g.lens, g.embed_table, g.out = ids.data_ptr(), labels.data_ptr(), lens.data_ptr(), table.data_ptr(), out.data_ptr()
    g.B, g.L, g.D, g.vocab, g.action_token_begin = B, L, table.shape[1], table.shape[0], action_token_begin
    _lib.call("ovla_language_average_ragged", g, _stream())
    return out


def image_prep(images_u8, *, crop: bool, crop_scale: float = 0.9, out_size: int = 224,
               mean=(0.485, 0.456, 0.406, 0.5, 0.5, 0.5), std=(0.229, 0.224, 0.225, 0.5, 0.5, 0.5)):
    """uint8 [n_img, H, W, 3] (device) -> bf16 [1, 6 * n_img, out, out] pixel_values: center crop (TF crop_and_resize rule) +
    uint8 re-quantisation + DINOv2 / SigLIP normalisation in one launch (openvla_utils.py:542-622, processing_prismatic.py:128-145)."""
    assert images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[-1] == 3 and images_u8.is_contiguous() and images_u8.is_cuda
    n, H, W, _ = images_u8.shape
    out = torch.empty((1, 6 * n, out_size, out_size), dtype=BF16, device=images_u8.device)
    g = STRUCTS["ovla_image_prep_args"]()
    g.src, g.dst, g.n_img, g.H, g.W, g.out, g.crop = images_u8.data_ptr(), out.data_ptr(), n, H, W, out_size, int(crop)
    g.crop_scale = float(crop_scale)
    for i in range(6):
        g.mean[i], g.std[i] = mean[i], std[i]
    _lib.call("ovla_image_prep", g, _stream())
    return out


def image_resize(images_u8, row_spans, col_spans):
    """uint8 [n, H, W, 3] (device) -> uint8 [n, out_h, out_w, 3]: separable span resampling (ovla.h: ovla_image_resize; TF's
    scale_and_translate kernel, rows first).  `*_spans` = (starts int32 [out], weights fp32 [out, span]) on the device
    (image_prep.lanczos3_spans)."""
    assert images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[-1] == 3 and images_u8.is_contiguous() and images_u8.is_cuda
    n, H, W, _ = images_u8.shape
    (rs, rw), (cs, cw) = row_spans, col_spans
    for st, wt in ((rs, rw), (cs, cw)):
        assert st.dtype == torch.int32 and wt.dtype == torch.float32 and wt.dim() == 2 and wt.shape[0] == st.shape[0] and st.is_cuda and wt.is_cuda
        assert st.is_contiguous() and wt.is_contiguous()
    oh, ow = rs.shape[0], cs.shape[0]
    out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=images_u8.device)
    wsb = int(_lib.lib().ovla_image_resize_workspace_bytes(n, W, oh))
    ws = torch.empty(wsb, dtype=torch.uint8, device=images_u8.device)
    g = STRUCTS["ovla_image_resize_args"]()
    g.src, g.dst, g.workspace, g.workspace_bytes = images_u8.data_ptr(), out.data_ptr(), ws.data_ptr(), wsb
    g.row_starts, g.row_weights, g.col_starts, g.col_weights = rs.data_ptr(), rw.data_ptr(), cs.data_ptr(), cw.data_ptr()
    g.n_img, g.H, g.W, g.out_h, g.out_w, g.row_span, g.col_span = n, H, W, oh, ow, rw.shape[1], cw.shape[1]
    _lib.call("ovla_image_resize", g, _stream())
    return out


def jpeg_roundtrip(images_u8, quality: int = 95):
    """uint8 [n, H, W, 3] (device) -> the same frames after a baseline 4:2:0 JPEG encode + decode at `quality` (ovla.h: ovla_jpeg_roundtrip;
    tf.image.encode_jpeg + tf.io.decode_image of experiments/robot/openvla_utils.py:532-533)."""
    assert images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[-1] == 3 and images_u8.is_contiguous() and images_u8.is_cuda
    n, H, W, _ = images_u8.shape
    out = torch.empty_like(images_u8)
    wsb = int(_lib.lib().ovla_jpeg_roundtrip_workspace_bytes(n, H, W))
    ws = torch.empty(wsb, dtype=torch.uint8, device=images_u8.device)
    g = STRUCTS["ovla_jpeg_roundtrip_args"]()
    g.src, g.dst, g.workspace, g.workspace_bytes = images_u8.data_ptr(), out.data_ptr(), ws.data_ptr(), wsb
    g.n_img, g.H, g.W, g.quality = n, H, W, int(quality)
    _lib.call("ovla_jpeg_roundtrip", g, _stream())
    return out


AUG_CROP, AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION, AUG_HUE = 1, 2, 4, 8, 16
AUG_ALL = 31


def image_augment(images_u8, params, *, ops_mask: int = AUG_ALL, out_size: int = 224,
                  mean=(0.485, 0.456, 0.406, 0.5, 0.5, 0.5), std=(0.229, 0.224, 0.225, 0.5, 0.5, 0.5)):
    """Training-time frames: uint8 [n, H, W, 3] + fp32 params [n, 8] (both on the device) -> bf16 [n, 6, out, out]: dlimp's
    augment_image ops (crop-and-resize box, brightness, contrast, saturation, hue; `ops_mask` selects them), uint8 re-quantisation
    and both backbones' normalisations (ovla.h: ovla_image_augment).  ops_mask = 0 is the evaluation path."""
    assert images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[-1] == 3 and images_u8.is_contiguous() and images_u8.is_cuda
    n, H, W, _ = images_u8.shape
    assert params.dtype == torch.float32 and tuple(params.shape) == (n, 8) and params.is_contiguous() and params.device == images_u8.device
    out = torch.empty((n, 6, out_size, out_size), dtype=BF16, device=images_u8.device)
    wsb = int(_lib.lib().ovla_image_augment_workspace_bytes(n, out_size))
    ws = torch.empty(wsb, dtype=torch.uint8, device=images_u8.device)
    g = STRUCTS["ovla_image_augment_args"]()
    g.src, g.dst, g.params, g.workspace, g.workspace_bytes = images_u8.data_ptr(), out.data_ptr(), params.data_ptr(), ws.data_ptr(), wsb
    g.n_img, g.H, g.W, g.out, g.ops_mask = n, H, W, out_size, int(ops_mask)
    for i in range(6):
        g.mean[i], g.std[i] = mean[i], std[i]
    _lib.call("ovla_image_augment", g, _stream())
    return out


def assemble_multimodal(ids, labels, table, patches, *, A, noisy=None, ignore_index=-100, action_token_begin=31743, action_dim=7,
                        out=None, action_pos=None):
    """ids/labels int64 [B,L]; table bf16 [V,D]; patches bf16 [B,P,D] -> (out [B,P+L,D], action_rows int32 [B,A]:
    flattened row of the hidden state that predicts each action slot).  `out` / `action_pos`: contiguous tensors of those shapes to
    write into; a given `action_pos` is the caller's to pre-fill (-1 = slot not found: the kernel writes found slots only)."""
    B, L = ids.shape
    P, D = patches.shape[1], patches.shape[2]
    if out is None:
        out = torch.empty((B, P + L, D), dtype=BF16, device=table.device)
    if action_pos is None:
        action_pos = torch.full((B, A), -1, dtype=torch.int32, device=table.device)
    assert out.shape == (B, P + L, D) and out.dtype == BF16 and out.is_contiguous()
    assert action_pos.shape == (B, A) and action_pos.dtype == torch.int32 and action_pos.is_contiguous()
    g = STRUCTS["ovla_assemble_args"]()
    g.ids, g.labels, g.embed_table, g.patches, g.noisy = ids.data_ptr(), labels.data_ptr(), table.data_ptr(), patches.data_ptr(), _p(noisy)
    g.out, g.action_pos = out.data_ptr(), action_pos.data_ptr()
    g.B, g.L, g.P, g.D, g.A, g.vocab = B, L, P, D, A, table.shape[0]
    g.ignore_index, g.action_token_begin, g.action_dim = ignore_index, action_token_begin, action_dim
    _lib.call("ovla_assemble_multimodal", g, _stream())
    return out, action_pos


def gather_rows(src, index, dim, *, dst=None, scatter_add=False, n_dst_rows=None):
    """gather: dst[i] = src[index[i]];  scatter_add: dst[index[i]] += src[i].  An index < 0 is "no row" (the -1 assemble_multimodal leaves
    for an action slot it did not find): the gather writes a zero row there, the scatter-add skips the entry."""
    n = index.numel()
    if dst is None:
        dst = torch.empty((n, dim), dtype=BF16, device=src.device)
    g = STRUCTS["ovla_gather_rows_args"]()
    g.src, g.index, g.dst, g.n, g.dim = src.data_ptr(), index.data_ptr(), dst.data_ptr(), n, dim
    g.src_ld, g.dst_ld, g.scatter_add = src.stride(0), dst.stride(0), int(scatter_add)
    _lib.call("ovla_gather_rows", g, _stream())
    return dst


def _host_slots(obs_slot, host_slots):
    """The optional host copy of the assignment as a ctypes int32 array (None without one); the library validates it (OVLA_EINVAL).  The
    caller holds the array until the call has returned."""
    if host_slots is None:
        return None
    vals = [int(v) for v in host_slots]
    assert len(vals) == obs_slot.numel(), "host_slots must mirror obs_slot"
    return (ctypes.c_int32 * len(vals))(*vals)


def lora_route(t, obs_slot, *, G, n, r, rows_per_obs, host_slots=None):
    """Multi-adapter routing, in place (ovla.h: ovla_lora_route): t bf16 [M, ld >= G*n*r] keeps, per row, the r columns of its own observation's
    slot in every group and gets +0 stored over the other slots' columns.  obs_slot: device int32 [n_obs]; row m belongs to observation
    m // rows_per_obs.  host_slots (optional, the same values on the host): an entry outside [0, n) raises before anything is launched."""
    _chk(t, name="t"); _chk(obs_slot, torch.int32, "obs_slot")
    assert t.dim() == 2 and t.stride(1) == 1 and obs_slot.is_contiguous()
    hs = _host_slots(obs_slot, host_slots)
    g = STRUCTS["ovla_lora_route_args"]()
    g.t, g.ld, g.obs_slot = t.data_ptr(), t.stride(0), obs_slot.data_ptr()
    g.obs_slot_host = ctypes.cast(hs, ctypes.c_void_p).value if hs is not None else None
    g.M, g.G, g.n, g.r, g.rows_per_obs, g.n_obs = t.shape[0], G, n, r, rows_per_obs, obs_slot.numel()
    e0 = _prof_begin()
    _lib.call("ovla_lora_route", g, _stream())
    _prof_end(e0, "lora_route", 0.0)
    return t


def select_by_slot(src, obs_slot, *, rows_per_obs, rows=None, out=None, host_slots=None):
    """out[m] = src[obs_slot[m // rows_per_obs], m] (ovla.h: ovla_select_by_slot): src bf16 / fp32 [n, R, dim] (dim contiguous, rows contiguous
    inside a slot), the first `rows` (default R) rows of every slot are candidates -> out [rows, dim]."""
    assert src.dim() == 3 and src.is_cuda and src.dtype in (BF16, torch.float32) and src.stride(2) == 1 and src.stride(1) == src.shape[2]
    _chk(obs_slot, torch.int32, "obs_slot")
    n, R, dim = src.shape
    rows = R if rows is None else rows
    assert 0 < rows <= R and obs_slot.is_contiguous()
    if out is None:
        out = torch.empty((rows, dim), dtype=src.dtype, device=src.device)
    assert out.shape == (rows, dim) and out.dtype == src.dtype and out.is_contiguous()
    hs = _host_slots(obs_slot, host_slots)
    g = STRUCTS["ovla_select_by_slot_args"]()
    g.src, g.dst, g.obs_slot = src.data_ptr(), out.data_ptr(), obs_slot.data_ptr()
    g.obs_slot_host = ctypes.cast(hs, ctypes.c_void_p).value if hs is not None else None
    g.src_slot_stride = src.stride(0)
    g.n, g.rows, g.dim, g.rows_per_obs, g.n_obs, g.elem_bytes = n, rows, dim, rows_per_obs, obs_slot.numel(), src.element_size()
    _lib.call("ovla_select_by_slot", g, _stream())
    return out


FILM_ITEM_COLS = 4   # OVLA_FILM_ITEM_COLS (ovla.h)
FILM_MAX_OBS = 64    # OVLA_FILM_MAX_OBS


def film_table(linears, device):
    """The descriptor table of ovla_film_vectors from [(W_slots bf16 [n, out_f, D], b_slots bf16 [n, out_f], out bf16 [rows, out_f])], built once
    per slot allocation (the tensors never move: the table keeps them).  Table order = list order; item_start is the running sum of
    ceil(out_f / FILM_ITEM_COLS).  -> dict(table (device bytes), host (the ctypes array), n_linears, n, D, rows)."""
    T = STRUCTS["ovla_film_linear"]
    assert linears, "film_table: no linears"
    n, _, D = linears[0][0].shape
    rows = min(o.shape[0] for _, _, o in linears)
    arr = (T * len(linears))()
    start = 0
    for j, (W, b, out) in enumerate(linears):
        _chk(W, name="W_slots"); _chk(b, name="b_slots"); _chk(out, name="out")
        out_f = W.shape[1]
        assert W.shape == (n, out_f, D) and b.shape == (n, out_f) and out.dim() == 2 and out.shape[1] == out_f
        assert W.is_contiguous() and b.is_contiguous() and out.is_contiguous()
        arr[j].W, arr[j].bias, arr[j].out, arr[j].out_f, arr[j].item_start = W.data_ptr(), b.data_ptr(), out.data_ptr(), out_f, start
        start += (out_f + FILM_ITEM_COLS - 1) // FILM_ITEM_COLS
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    return dict(table=raw, host=arr, n_linears=len(linears), n=n, D=D, rows=rows, keep=list(linears))


def film_vectors(tab, avg, obs_slot, *, host_slots=None):
    """Per-policy FiLM vectors, ONE launch on the current stream (ovla.h: ovla_film_vectors): for every linear of `tab` (film_table) and every
    observation b < n_obs, out[b] = bf16(bias[slot(b)] + W[slot(b)] . avg[b]).  avg bf16 [>= n_obs, D] (unit inner stride); obs_slot device
    int32 [n_obs]; host_slots (optional, the same values on the host): an entry outside [0, n) raises before anything is launched."""
    _chk(avg, name="avg"); _chk(obs_slot, torch.int32, "obs_slot")
    assert avg.dim() == 2 and avg.stride(1) == 1 and avg.shape[1] == tab["D"] and obs_slot.is_contiguous()
    n_obs = obs_slot.numel()
    assert n_obs <= avg.shape[0] and n_obs <= tab["rows"], "film_vectors: more observations than avg / out rows"
    hs = _host_slots(obs_slot, host_slots)
    g = STRUCTS["ovla_film_vectors_args"]()
    g.table, g.table_host = tab["table"].data_ptr(), ctypes.cast(tab["host"], ctypes.c_void_p).value
    g.avg, g.ld_avg, g.obs_slot = avg.data_ptr(), avg.stride(0), obs_slot.data_ptr()
    g.obs_slot_host = ctypes.cast(hs, ctypes.c_void_p).value if hs is not None else None
    g.n_linears, g.n_obs, g.n, g.D = tab["n_linears"], n_obs, tab["n"], tab["D"]
    e0 = _prof_begin()
    _lib.call("ovla_film_vectors", g, _stream())
    _prof_end(e0, "film_vectors", 2.0 * n_obs * tab["D"] * sum(W.shape[1] for W, _, _ in tab["keep"]))
    return tab


# ----------------------------------------------------------------------------------------------------------------------
def _dropout_key(g, modules, p, seed, call):
    """The mask-contract fields shared by the three LoRA-dropout argument structs (ovla.h "LoRA dropout")."""
    if not 1 <= len(modules) <= 4:
        raise ValueError(f"lora dropout: {len(modules)} groups (1 .. 4 supported)")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"lora dropout: p = {p} is outside [0, 1)")
    g.module = (ctypes.c_uint32 * 4)(*[int(v) & 0xFFFFFFFF for v in modules])
    g.seed_lo, g.seed_hi, g.call, g.p, g.G = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, int(call) & 0xFFFFFFFF, p, len(modules)


def lora_dropout_apply(x, *, modules, p, seed, call, out=None):
    """xd_g = dropout_g(x) for every module id in `modules` (ovla.h: ovla_lora_dropout_apply): x bf16 [M, K] (row stride free) is read once,
    returns bf16 [G, M, K] contiguous."""
    _chk(x, name="x")
    assert x.dim() == 2 and x.stride(1) == 1
    M, K = x.shape
    if out is None:
        out = torch.empty((len(modules), M, K), dtype=BF16, device=x.device)
    assert out.shape == (len(modules), M, K) and out.dtype == BF16 and out.is_contiguous()
    g = STRUCTS["ovla_lora_dropout_apply_args"]()
    _dropout_key(g, modules, p, seed, call)
    g.x, g.ldx, g.M, g.K = x.data_ptr(), x.stride(0), M, K
    g.out = (ctypes.c_void_p * 4)(*[out[i].data_ptr() for i in range(len(modules))])
    e0 = _prof_begin()
    _lib.call("ovla_lora_dropout_apply", g, _stream())
    _prof_end(e0, "lora_dropout", 0.0)
    return out


def lora_dropout_proj(x, A, *, alpha, modules, p, seed, call, out=None):
    """t[:, g r : (g + 1) r] = bf16(alpha * dropout_g(x) . A_g^T) for all groups in one launch (ovla.h: ovla_lora_dropout_proj): x bf16 [M, K],
    A bf16 [G * 32, K] -> t bf16 [M, G * 32].  The dropped activations exist in registers only."""
    _chk(x, name="x"); _chk(A, name="A")
    assert x.dim() == 2 and A.dim() == 2 and x.stride(1) == 1 and A.stride(1) == 1 and x.shape[1] == A.shape[1]
    M, K = x.shape
    G = len(modules)
    assert A.shape[0] % G == 0
    r = A.shape[0] // G
    if out is None:
        out = torch.empty((M, G * r), dtype=BF16, device=x.device)
    assert out.shape == (M, G * r) and out.dtype == BF16 and out.stride(1) == 1
    g = STRUCTS["ovla_lora_dropout_proj_args"]()
    _dropout_key(g, modules, p, seed, call)
    g.x, g.ldx, g.A, g.lda, g.t, g.ldt = x.data_ptr(), x.stride(0), A.data_ptr(), A.stride(0), out.data_ptr(), out.stride(0)
    g.alpha, g.M, g.K, g.r = alpha, M, K, r
    e0 = _prof_begin()
    _lib.call("ovla_lora_dropout_proj", g, _stream())
    _prof_end(e0, "lora_dropout", 2.0 * M * G * r * K)
    return out


def lora_dropout_backproj(dx, dt, AT, *, modules, p, seed, call):
    """dx += sum_g keep_g ? inv * (dt_g . A_g) : 0, in place and rounded once (ovla.h: ovla_lora_dropout_backproj): dx bf16 [M, K] (row
    stride free), dt bf16 [M, G r], AT bf16 [K, G r]."""
    _chk(dx, name="dx"); _chk(dt, name="dt"); _chk(AT, name="AT")
    assert dx.dim() == 2 and dt.dim() == 2 and AT.dim() == 2 and dx.stride(1) == 1 and dt.stride(1) == 1 and AT.stride(1) == 1
    M, K = dx.shape
    G = len(modules)
    assert dt.shape[0] == M and AT.shape[0] == K and dt.shape[1] == AT.shape[1] and dt.shape[1] % G == 0
    g = STRUCTS["ovla_lora_dropout_backproj_args"]()
    _dropout_key(g, modules, p, seed, call)
    g.dx, g.ld, g.dt, g.ld_dt, g.AT, g.ld_at = dx.data_ptr(), dx.stride(0), dt.data_ptr(), dt.stride(0), AT.data_ptr(), AT.stride(0)
    g.M, g.K, g.r = M, K, dt.shape[1] // G
    e0 = _prof_begin()
    _lib.call("ovla_lora_dropout_backproj", g, _stream())
    _prof_end(e0, "lora_dropout", 2.0 * M * dt.shape[1] * K)
    return dx


# ----------------------------------------------------------------------------------------------------------------------
def token_ce(logits, targets, *, vocab=None, grad_scale=None, inplace_grad=True, dlogits=None):
    """Next-token cross entropy on gathered rows (ovla.h: ovla_token_ce): logits bf16 [rows, ld >= vocab], targets int64 [rows] ->
    (loss_rows fp32 [rows], argmax int32 [rows], dlogits bf16 or None).  With grad_scale the gradient overwrites `logits`
    (inplace_grad), goes to `dlogits` (bf16 [rows, ld_d >= vocab]) when one is given, or to a new tensor."""
    _chk(logits)
    rows = logits.shape[0]
    vocab = logits.shape[1] if vocab is None else vocab
    assert targets.dtype == torch.int64 and targets.numel() == rows and targets.is_contiguous() and targets.device == logits.device
    loss_rows = torch.empty(rows, dtype=torch.float32, device=logits.device)
    amax = torch.empty(rows, dtype=torch.int32, device=logits.device)
    d = None
    if grad_scale is not None:
        d = dlogits if dlogits is not None else (logits if inplace_grad else torch.empty_like(logits))
        assert d.dtype == BF16 and d.shape[0] == rows and d.shape[1] >= vocab and d.stride(1) == 1
    g = STRUCTS["ovla_token_ce_args"]()
    g.logits, g.ld, g.targets, g.loss_rows, g.argmax = logits.data_ptr(), logits.stride(0), targets.data_ptr(), loss_rows.data_ptr(), amax.data_ptr()
    g.dlogits, g.ld_d = _p(d), (d.stride(0) if d is not None else 0)
    g.rows, g.vocab, g.grad_scale = rows, vocab, float(grad_scale or 0.0)
    _lib.call("ovla_token_ce", g, _stream())
    return loss_rows, amax, d


def argmax_bins(logits, *, n_tokens, n_bins, vocab=None, token=None, bins=None):
    """Greedy action-token decode (ovla.h: ovla_argmax_bins): logits bf16 [rows, ld >= vocab] -> (token int32 [rows] = lowest index of the row
    maximum over [0, vocab), bin int32 [rows] = clip(n_tokens - token - 1, 0, n_bins - 1))."""
    _chk(logits, name="logits")
    assert logits.dim() == 2 and logits.stride(1) == 1
    rows = logits.shape[0]
    vocab = logits.shape[1] if vocab is None else vocab
    token = torch.empty(rows, dtype=torch.int32, device=logits.device) if token is None else token
    bins = torch.empty(rows, dtype=torch.int32, device=logits.device) if bins is None else bins
    assert token.dtype == torch.int32 and bins.dtype == torch.int32 and token.numel() == rows and bins.numel() == rows
    g = STRUCTS["ovla_argmax_bins_args"]()
    g.logits, g.ld, g.token, g.bin = logits.data_ptr(), logits.stride(0), token.data_ptr(), bins.data_ptr()
    g.rows, g.vocab, g.n_tokens, g.n_bins = rows, vocab, n_tokens, n_bins
    _lib.call("ovla_argmax_bins", g, _stream())
    return token, bins


def _token_window(window, vocab):
    lo, hi = (0, vocab) if window is None else (int(window[0]), int(window[1]))
    return lo, hi


def sample_tokens(logits, *, n_tokens, n_bins, vocab=None, window=None, temperature=1.0, seed=0, call=0, state_dev=None, row_key=None,
                  entropy=True, token=None, bins=None, logprob=None, entropy_out=None):
    """Stochastic action-token decode (ovla.h "Token sampling and the policy-gradient objective": ovla_sample_tokens): logits bf16 [rows, ld >= vocab]
    -> (token int32, bin int32, logprob fp32, entropy fp32 or None), each [rows]: one Gumbel-max draw per row from softmax(logits[lo:hi] / T), a pure
    function of (seed, call, row key, token id).  `window` = (lo, hi), default the whole vocabulary.  `state_dev` (uint32 [3] on the device: seed_lo,
    seed_hi, call) overrides seed / call when the kernel runs; `row_key` int32 [rows] replaces the row index in the generator's counter."""
    _chk(logits, name="logits")
    assert logits.dim() == 2 and logits.stride(1) == 1
    rows, dev = logits.shape[0], logits.device
    vocab = logits.shape[1] if vocab is None else vocab
    lo, hi = _token_window(window, vocab)
    token = torch.empty(rows, dtype=torch.int32, device=dev) if token is None else token
    bins = torch.empty(rows, dtype=torch.int32, device=dev) if bins is None else bins
    logprob = torch.empty(rows, dtype=torch.float32, device=dev) if logprob is None else logprob
    if entropy_out is None and entropy:
        entropy_out = torch.empty(rows, dtype=torch.float32, device=dev)
    for t, dt, name in ((token, torch.int32, "token"), (bins, torch.int32, "bins"), (logprob, torch.float32, "logprob"), (entropy_out, torch.float32, "entropy"),
                        (row_key, torch.int32, "row_key")):
        if t is not None:
            _chk(t, dt, name)
            assert t.numel() == rows and t.is_contiguous(), f"{name}: expected {rows} contiguous elements"
    if state_dev is not None:
        assert state_dev.is_cuda and state_dev.numel() == 3 and state_dev.is_contiguous() and state_dev.element_size() == 4 and not state_dev.is_floating_point(), \
            "state_dev: three 32-bit integers on the device (seed_lo, seed_hi, call)"
    g = STRUCTS["ovla_sample_tokens_args"]()
    g.logits, g.ld, g.token, g.bin, g.logprob, g.entropy = logits.data_ptr(), logits.stride(0), token.data_ptr(), bins.data_ptr(), logprob.data_ptr(), _p(entropy_out)
    g.state_dev, g.row_key = _p(state_dev), _p(row_key)
    g.seed_lo, g.seed_hi, g.call = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, int(call) & 0xFFFFFFFF
    g.temperature = float(temperature)
    g.rows, g.vocab, g.lo, g.hi, g.n_tokens, g.n_bins = rows, vocab, lo, hi, n_tokens, n_bins
    _lib.call("ovla_sample_tokens", g, _stream())
    return token, bins, logprob, entropy_out


def token_pg(logits, tokens, advantage, *, vocab=None, window=None, temperature=1.0, old_logprob=None, clip=(0.8, 1.2), grad_scale=None, inplace_grad=True,
             dlogits=None, logprob=None, entropy=None, ratio=None, clipped=None):
    """Clipped policy-gradient objective on given tokens (ovla.h: ovla_token_pg): logits bf16 [rows, ld >= vocab], tokens int32 [rows], advantage fp32
    [rows] (and old_logprob fp32 [rows]) on the device -> (logprob, entropy, ratio fp32 [rows], clipped int32 [rows], dlogits bf16 or None).  With
    grad_scale the gradient overwrites `logits` (inplace_grad), goes to `dlogits` when one is given, or to a new tensor, as in token_ce."""
    _chk(logits, name="logits")
    assert logits.dim() == 2 and logits.stride(1) == 1
    rows, dev = logits.shape[0], logits.device
    vocab = logits.shape[1] if vocab is None else vocab
    lo, hi = _token_window(window, vocab)
    logprob = torch.empty(rows, dtype=torch.float32, device=dev) if logprob is None else logprob
    entropy = torch.empty(rows, dtype=torch.float32, device=dev) if entropy is None else entropy
    ratio = torch.empty(rows, dtype=torch.float32, device=dev) if ratio is None else ratio
    clipped = torch.empty(rows, dtype=torch.int32, device=dev) if clipped is None else clipped
    for t, dt, name in ((tokens, torch.int32, "tokens"), (advantage, torch.float32, "advantage"), (old_logprob, torch.float32, "old_logprob"),
                        (logprob, torch.float32, "logprob"), (entropy, torch.float32, "entropy"), (ratio, torch.float32, "ratio"), (clipped, torch.int32, "clipped")):
        if t is not None:
            _chk(t, dt, name)
            assert t.numel() == rows and t.is_contiguous(), f"{name}: expected {rows} contiguous elements"
    d = None
    if grad_scale is not None:
        d = dlogits if dlogits is not None else (logits if inplace_grad else torch.empty_like(logits))
        assert d.dtype == BF16 and d.shape[0] == rows and d.shape[1] >= vocab and d.stride(1) == 1
    g = STRUCTS["ovla_token_pg_args"]()
    g.logits, g.ld, g.tokens, g.advantage, g.old_logprob = logits.data_ptr(), logits.stride(0), _p(tokens), _p(advantage), _p(old_logprob)
    g.logprob, g.entropy, g.ratio, g.clipped = logprob.data_ptr(), entropy.data_ptr(), ratio.data_ptr(), clipped.data_ptr()
    g.dlogits, g.ld_d = _p(d), (d.stride(0) if d is not None else 0)
    g.temperature, g.clip_lo, g.clip_hi, g.grad_scale = float(temperature), float(clip[0]), float(clip[1]), float(grad_scale or 0.0)
    g.rows, g.vocab, g.lo, g.hi = rows, vocab, lo, hi
    _lib.call("ovla_token_pg", g, _stream())
    return logprob, entropy, ratio, clipped, d


PG_GROUP_MAX = 64          # ovla.h: OVLA_PG_GROUP_MAX


def sample_tokens_group(logits, G, *, n_tokens, n_bins, vocab=None, window=None, temperature=1.0, seed=0, call=0, state_dev=None, row_key=None,
                        entropy=True, token=None, bins=None, logprob=None, entropy_out=None):
    """G draws per row in one launch (ovla.h: ovla_sample_tokens_group): logits bf16 [rows, ld >= vocab] -> (token int32, bin int32, logprob fp32,
    each [rows, G]; entropy fp32 [rows] or None).  Draw (r, g) is sample_tokens' draw of row r under row key row_key[r, g] (default r * G + g),
    bit for bit.  The remaining arguments are sample_tokens'."""
    _chk(logits, name="logits")
    assert logits.dim() == 2 and logits.stride(1) == 1
    rows, dev, G = logits.shape[0], logits.device, int(G)
    vocab = logits.shape[1] if vocab is None else vocab
    lo, hi = _token_window(window, vocab)
    token = torch.empty((rows, G), dtype=torch.int32, device=dev) if token is None else token
    bins = torch.empty((rows, G), dtype=torch.int32, device=dev) if bins is None else bins
    logprob = torch.empty((rows, G), dtype=torch.float32, device=dev) if logprob is None else logprob
    if entropy_out is None and entropy:
        entropy_out = torch.empty(rows, dtype=torch.float32, device=dev)
    for t, dt, name, n in ((token, torch.int32, "token", rows * G), (bins, torch.int32, "bins", rows * G), (logprob, torch.float32, "logprob", rows * G),
                           (entropy_out, torch.float32, "entropy", rows), (row_key, torch.int32, "row_key", rows * G)):
        if t is not None:
            _chk(t, dt, name)
            assert t.numel() == n and t.is_contiguous(), f"{name}: expected {n} contiguous elements"
    if state_dev is not None:
        assert state_dev.is_cuda and state_dev.numel() == 3 and state_dev.is_contiguous() and state_dev.element_size() == 4 and not state_dev.is_floating_point(), \
            "state_dev: three 32-bit integers on the device (seed_lo, seed_hi, call)"
    g = STRUCTS["ovla_sample_tokens_group_args"]()
    g.logits, g.ld, g.token, g.bin, g.logprob, g.entropy = logits.data_ptr(), logits.stride(0), token.data_ptr(), bins.data_ptr(), logprob.data_ptr(), _p(entropy_out)
    g.state_dev, g.row_key = _p(state_dev), _p(row_key)
    g.seed_lo, g.seed_hi, g.call = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, int(call) & 0xFFFFFFFF
    g.temperature = float(temperature)
    g.rows, g.vocab, g.lo, g.hi, g.n_tokens, g.n_bins, g.G = rows, vocab, lo, hi, n_tokens, n_bins, G
    _lib.call("ovla_sample_tokens_group", g, _stream())
    return token, bins, logprob, entropy_out


def token_pg_group(logits, tokens, advantage, *, vocab=None, window=None, temperature=1.0, old_logprob=None, ref_logprob=None, kl_coef=0.0, ent_scale=0.0,
                   clip=(0.8, 1.2), grad_scale=None, inplace_grad=True, dlogits=None, logprob=None, ratio=None, clipped=None, kl=None, entropy=None):
    """Clipped policy-gradient objective with a KL penalty and an entropy bonus on G given samples per row (ovla.h: ovla_token_pg_group): logits bf16
    [rows, ld >= vocab], tokens int32 / advantage fp32 [rows, G] (and old_logprob / ref_logprob fp32 [rows, G]) on the device -> (logprob, ratio fp32
    [rows, G], clipped int32 [rows, G], kl fp32 [rows, G] or None, entropy fp32 [rows], dlogits bf16 or None).  `kl` exists exactly when ref_logprob is
    given.  The gradient's destination follows token_pg."""
    _chk(logits, name="logits")
    assert logits.dim() == 2 and logits.stride(1) == 1 and tokens.dim() == 2 and tokens.shape[0] == logits.shape[0]
    rows, dev, G = logits.shape[0], logits.device, tokens.shape[1]
    vocab = logits.shape[1] if vocab is None else vocab
    lo, hi = _token_window(window, vocab)
    logprob = torch.empty((rows, G), dtype=torch.float32, device=dev) if logprob is None else logprob
    ratio = torch.empty((rows, G), dtype=torch.float32, device=dev) if ratio is None else ratio
    clipped = torch.empty((rows, G), dtype=torch.int32, device=dev) if clipped is None else clipped
    entropy = torch.empty(rows, dtype=torch.float32, device=dev) if entropy is None else entropy
    if kl is None and ref_logprob is not None:
        kl = torch.empty((rows, G), dtype=torch.float32, device=dev)
    for t, dt, name, n in ((tokens, torch.int32, "tokens", rows * G), (advantage, torch.float32, "advantage", rows * G),
                           (old_logprob, torch.float32, "old_logprob", rows * G), (ref_logprob, torch.float32, "ref_logprob", rows * G),
                           (logprob, torch.float32, "logprob", rows * G), (ratio, torch.float32, "ratio", rows * G), (clipped, torch.int32, "clipped", rows * G),
                           (kl, torch.float32, "kl", rows * G), (entropy, torch.float32, "entropy", rows)):
        if t is not None:
            _chk(t, dt, name)
            assert t.numel() == n and t.is_contiguous(), f"{name}: expected {n} contiguous elements"
    d = None
    if grad_scale is not None:
        d = dlogits if dlogits is not None else (logits if inplace_grad else torch.empty_like(logits))
        assert d.dtype == BF16 and d.shape[0] == rows and d.shape[1] >= vocab and d.stride(1) == 1
    g = STRUCTS["ovla_token_pg_group_args"]()
    g.logits, g.ld, g.tokens, g.advantage = logits.data_ptr(), logits.stride(0), _p(tokens), _p(advantage)
    g.old_logprob, g.ref_logprob = _p(old_logprob), _p(ref_logprob)
    g.logprob, g.ratio, g.clipped, g.kl, g.entropy = logprob.data_ptr(), ratio.data_ptr(), clipped.data_ptr(), _p(kl), entropy.data_ptr()
    g.dlogits, g.ld_d = _p(d), (d.stride(0) if d is not None else 0)
    g.temperature, g.clip_lo, g.clip_hi, g.grad_scale = float(temperature), float(clip[0]), float(clip[1]), float(grad_scale or 0.0)
    g.kl_coef, g.ent_scale = float(kl_coef), float(ent_scale)
    g.rows, g.G, g.vocab, g.lo, g.hi = rows, G, vocab, lo, hi
    _lib.call("ovla_token_pg_group", g, _stream())
    return logprob, ratio, clipped, kl, entropy, d


LAPLACE_MAX_ADIM = 16      # ovla.h "Laplace policy on the L1 head": 1 <= adim <= 16


def laplace_scales(scale, adim):
    """A scalar or per-dimension scale b -> (b fp32 [adim], log_norm fp32 [adim] = float32(log(2 b)) formed in double), numpy arrays: the by-value
    arguments of the two Laplace kernels.  The kernels refuse a scale that is not positive and finite."""
    b = np.asarray(scale.detach().cpu().numpy() if torch.is_tensor(scale) else scale, dtype=np.float64).reshape(-1)
    if b.size == 1:
        b = np.repeat(b, adim)
    if b.size != adim:
        raise ValueError(f"scale: {b.size} values for {adim} action dimensions (a scalar or one per dimension)")
    b32 = b.astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        log_norm = np.log(2.0 * b32.astype(np.float64)).astype(np.float32)
    return b32, log_norm


def _set_laplace_scales(g, scale, adim):
    b, ln = laplace_scales(scale, adim)
    for d in range(adim):
        g.scale[d], g.log_norm[d] = float(b[d]), float(ln[d])


def laplace_sample(pred, scale, G=1, *, seed=0, call=0, state_dev=None, row_key=None, action=None, logprob=None):
    """G Laplace draws per row around the L1 head's prediction (ovla.h "Laplace policy on the L1 head": ovla_laplace_sample): pred bf16 [rows, adim],
    scale a scalar or [adim] -> (action fp32 [rows, G, adim], logprob fp32 [rows, G]), a pure function of (seed, call, row key, dimension) and the
    prediction.  `row_key` int32 [rows, G] replaces r * G + g in the generator's counter; `state_dev` as in sample_tokens."""
    _chk(pred, name="pred")
    assert pred.dim() == 2 and pred.is_contiguous()
    (rows, adim), dev, G = pred.shape, pred.device, int(G)
    action = torch.empty((rows, G, adim), dtype=torch.float32, device=dev) if action is None else action
    logprob = torch.empty((rows, G), dtype=torch.float32, device=dev) if logprob is None else logprob
    for t, dt, name, n in ((action, torch.float32, "action", rows * G * adim), (logprob, torch.float32, "logprob", rows * G), (row_key, torch.int32, "row_key", rows * G)):
        if t is not None:
            _chk(t, dt, name)
            assert t.numel() == n and t.is_contiguous(), f"{name}: expected {n} contiguous elements"
    if state_dev is not None:
        assert state_dev.is_cuda and state_dev.numel() == 3 and state_dev.is_contiguous() and state_dev.element_size() == 4 and not state_dev.is_floating_point(), \
            "state_dev: three 32-bit integers on the device (seed_lo, seed_hi, call)"
    g = STRUCTS["ovla_laplace_sample_args"]()
    g.pred, g.action, g.logprob, g.state_dev, g.row_key = pred.data_ptr(), action.data_ptr(), logprob.data_ptr(), _p(state_dev), _p(row_key)
    g.seed_lo, g.seed_hi, g.call = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, int(call) & 0xFFFFFFFF
    g.rows, g.adim, g.G = rows, adim, G
    if 1 <= adim <= LAPLACE_MAX_ADIM:                      # (otherwise the kernel's own refusal speaks)
        _set_laplace_scales(g, scale, adim)
    _lib.call("ovla_laplace_sample", g, _stream())
    return action, logprob


def laplace_pg(pred, actions, advantage, scale, *, old_logprob=None, ref_pred=None, kl_coef=0.0, clip=(0.8, 1.2), grad_scale=None, kl_scale=0.0, dpred=None,
               logprob=None, ratio=None, clipped=None, kl=None):
    """Clipped policy-gradient objective and closed-form KL of the Laplace policy on G given draws per row (ovla.h: ovla_laplace_pg): pred bf16
    [rows, adim], actions fp32 [rows, G, adim], advantage fp32 [rows, G] (and old_logprob fp32 [rows, G], ref_pred bf16 [rows, adim]) on the device
    -> (logprob, ratio fp32 [rows, G], clipped int32 [rows, G], kl fp32 [rows] or None, dpred bf16 [rows, adim] or None).  `kl` exists exactly when
    ref_pred is given; with grad_scale the gradient with respect to pred goes to `dpred` (a new tensor without one)."""
    _chk(pred, name="pred")
    assert pred.dim() == 2 and pred.is_contiguous() and actions.dim() == 3 and actions.shape[0] == pred.shape[0] and actions.shape[2] == pred.shape[1]
    (rows, adim), dev, G = pred.shape, pred.device, actions.shape[1]
    logprob = torch.empty((rows, G), dtype=torch.float32, device=dev) if logprob is None else logprob
    ratio = torch.empty((rows, G), dtype=torch.float32, device=dev) if ratio is None else ratio
    clipped = torch.empty((rows, G), dtype=torch.int32, device=dev) if clipped is None else clipped
    if kl is None and ref_pred is not None:
        kl = torch.empty(rows, dtype=torch.float32, device=dev)
    if grad_scale is not None and dpred is None:
        dpred = torch.empty((rows, adim), dtype=BF16, device=dev)
    for t, dt, name, n in ((actions, torch.float32, "actions", rows * G * adim), (advantage, torch.float32, "advantage", rows * G),
                           (old_logprob, torch.float32, "old_logprob", rows * G), (ref_pred, BF16, "ref_pred", rows * adim),
                           (logprob, torch.float32, "logprob", rows * G), (ratio, torch.float32, "ratio", rows * G), (clipped, torch.int32, "clipped", rows * G),
                           (kl, torch.float32, "kl", rows), (dpred, BF16, "dpred", rows * adim)):
        if t is not None:
            _chk(t, dt, name)
            assert t.numel() == n and t.is_contiguous(), f"{name}: expected {n} contiguous elements"
    g = STRUCTS["ovla_laplace_pg_args"]()
    g.pred, g.ref_pred, g.actions, g.advantage, g.old_logprob = pred.data_ptr(), _p(ref_pred), actions.data_ptr(), advantage.data_ptr(), _p(old_logprob)
    g.logprob, g.ratio, g.clipped, g.kl, g.dpred = logprob.data_ptr(), ratio.data_ptr(), clipped.data_ptr(), _p(kl), _p(dpred)
    g.clip_lo, g.clip_hi, g.grad_scale, g.kl_coef, g.kl_scale = float(clip[0]), float(clip[1]), float(grad_scale or 0.0), float(kl_coef), float(kl_scale)
    g.rows, g.adim, g.G = rows, adim, G
    if 1 <= adim <= LAPLACE_MAX_ADIM:
        _set_laplace_scales(g, scale, adim)
    _lib.call("ovla_laplace_pg", g, _stream())
    return logprob, ratio, clipped, kl, dpred


LAPLACE_SCALE_BOUNDS = (-6.0, 1.0)     # the default clamp of a learned log-scale: b in about [0.0025, 2.7] normalised units (a design choice)


def laplace_sample_rows(pred, log_scale, bounds, G=1, *, seed=0, call=0, state_dev=None, row_key=None, action=None, logprob=None, entropy=None):
    """laplace_sample with a scale per element (ovla.h "Laplace policy with a learned scale": ovla_laplace_sample_rows): pred, log_scale bf16
    [rows, adim], bounds = (s_lo, s_hi) the clamp of the log-scale -> (action fp32 [rows, G, adim], logprob fp32 [rows, G], entropy fp32 [rows]).
    With log_scale == 0 the first two are laplace_sample(pred, 1.0, ...)'s bits."""
    _chk(pred, name="pred"), _chk(log_scale, name="log_scale")
    assert pred.dim() == 2 and pred.is_contiguous() and log_scale.shape == pred.shape and log_scale.is_contiguous()
    (rows, adim), dev, G = pred.shape, pred.device, int(G)
    action = torch.empty((rows, G, adim), dtype=torch.float32, device=dev) if action is None else action
    logprob = torch.empty((rows, G), dtype=torch.float32, device=dev) if logprob is None else logprob
    entropy = torch.empty(rows, dtype=torch.float32, device=dev) if entropy is None else entropy
    for t, dt, name, n in ((action, torch.float32, "action", rows * G * adim), (logprob, torch.float32, "logprob", rows * G),
                           (entropy, torch.float32, "entropy", rows), (row_key, torch.int32, "row_key", rows * G)):
        if t is not None:
            _chk(t, dt, name)
            assert t.numel() == n and t.is_contiguous(), f"{name}: expected {n} contiguous elements"
    if state_dev is not None:
        assert state_dev.is_cuda and state_dev.numel() == 3 and state_dev.is_contiguous() and state_dev.element_size() == 4 and not state_dev.is_floating_point(), \
            "state_dev: three 32-bit integers on the device (seed_lo, seed_hi, call)"
    g = STRUCTS["ovla_laplace_sample_rows_args"]()
    g.pred, g.log_scale, g.action, g.logprob, g.entropy = pred.data_ptr(), log_scale.data_ptr(), action.data_ptr(), logprob.data_ptr(), entropy.data_ptr()
    g.state_dev, g.row_key = _p(state_dev), _p(row_key)
    g.seed_lo, g.seed_hi, g.call = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, int(call) & 0xFFFFFFFF
    g.s_lo, g.s_hi = float(bounds[0]), float(bounds[1])
    g.rows, g.adim, g.G = rows, adim, G
    _lib.call("ovla_laplace_sample_rows", g, _stream())
    return action, logprob, entropy


def laplace_pg_rows(pred, log_scale, bounds, actions, advantage, *, old_logprob=None, ref_pred=None, ref_log_scale=None, kl_coef=0.0, clip=(0.8, 1.2),
                    grad_scale=None, kl_scale=0.0, entropy_coef=0.0, ent_scale=0.0, dpred=None, dlog_scale=None, want_dpred=True, want_dlog_scale=True,
                    logprob=None, ratio=None, clipped=None, kl=None, entropy=None):
    """laplace_pg with a scale per element and its gradient (ovla.h: ovla_laplace_pg_rows): pred, log_scale bf16 [rows, adim], bounds = (s_lo,
    s_hi), actions fp32 [rows, G, adim], advantage fp32 [rows, G] (and old_logprob fp32 [rows, G]; ref_pred with ref_log_scale bf16 [rows, adim])
    -> (logprob, ratio fp32 [rows, G], clipped int32 [rows, G], kl fp32 [rows] or None, entropy fp32 [rows], dpred, dlog_scale bf16 [rows, adim] or
    None).  `kl` exists exactly when the reference is given; with grad_scale the gradients go to `dpred` / `dlog_scale` (new tensors without
    them; want_dpred=False / want_dlog_scale=False leaves that one out of the launch)."""
    _chk(pred, name="pred"), _chk(log_scale, name="log_scale")
    assert pred.dim() == 2 and pred.is_contiguous() and actions.dim() == 3 and actions.shape[0] == pred.shape[0] and actions.shape[2] == pred.shape[1]
    assert log_scale.shape == pred.shape and log_scale.is_contiguous()
    (rows, adim), dev, G = pred.shape, pred.device, actions.shape[1]
    logprob = torch.empty((rows, G), dtype=torch.float32, device=dev) if logprob is None else logprob
    ratio = torch.empty((rows, G), dtype=torch.float32, device=dev) if ratio is None else ratio
    clipped = torch.empty((rows, G), dtype=torch.int32, device=dev) if clipped is None else clipped
    entropy = torch.empty(rows, dtype=torch.float32, device=dev) if entropy is None else entropy
    if kl is None and ref_pred is not None:
        kl = torch.empty(rows, dtype=torch.float32, device=dev)
    if grad_scale is not None and dpred is None and want_dpred:
        dpred = torch.empty((rows, adim), dtype=BF16, device=dev)
    if grad_scale is not None and dlog_scale is None and want_dlog_scale:
        dlog_scale = torch.empty((rows, adim), dtype=BF16, device=dev)
    for t, dt, name, n in ((actions, torch.float32, "actions", rows * G * adim), (advantage, torch.float32, "advantage", rows * G),
                           (old_logprob, torch.float32, "old_logprob", rows * G), (ref_pred, BF16, "ref_pred", rows * adim),
                           (ref_log_scale, BF16, "ref_log_scale", rows * adim), (logprob, torch.float32, "logprob", rows * G),
                           (ratio, torch.float32, "ratio", rows * G), (clipped, torch.int32, "clipped", rows * G), (kl, torch.float32, "kl", rows),
                           (entropy, torch.float32, "entropy", rows), (dpred, BF16, "dpred", rows * adim), (dlog_scale, BF16, "dlog_scale", rows * adim)):
        if t is not None:
            _chk(t, dt, name)
            assert t.numel() == n and t.is_contiguous(), f"{name}: expected {n} contiguous elements"
    g = STRUCTS["ovla_laplace_pg_rows_args"]()
    g.pred, g.log_scale, g.ref_pred, g.ref_log_scale = pred.data_ptr(), log_scale.data_ptr(), _p(ref_pred), _p(ref_log_scale)
    g.actions, g.advantage, g.old_logprob = actions.data_ptr(), advantage.data_ptr(), _p(old_logprob)
    g.logprob, g.ratio, g.clipped, g.kl, g.entropy = logprob.data_ptr(), ratio.data_ptr(), clipped.data_ptr(), _p(kl), entropy.data_ptr()
    g.dpred, g.dlog_scale = _p(dpred), _p(dlog_scale)
    g.s_lo, g.s_hi, g.clip_lo, g.clip_hi = float(bounds[0]), float(bounds[1]), float(clip[0]), float(clip[1])
    g.grad_scale, g.kl_coef, g.kl_scale, g.entropy_coef, g.ent_scale = float(grad_scale or 0.0), float(kl_coef), float(kl_scale), float(entropy_coef), float(ent_scale)
    g.rows, g.adim, g.G = rows, adim, G
    _lib.call("ovla_laplace_pg_rows", g, _stream())
    return logprob, ratio, clipped, kl, entropy, dpred, dlog_scale


DPO_CHUNK_MAX = 64         # ovla.h: OVLA_DPO_CHUNK_MAX
DPO_LOSS_TYPES = {"sigmoid": 0, "ipo": 1}


def laplace_dpo(pred, ref_pred, chosen, rejected, chunk, scale=None, *, log_scale=None, ref_log_scale=None, bounds=LAPLACE_SCALE_BOUNDS, weight=None, beta,
                label_smoothing=0.0, loss_type="sigmoid", grad_scale=None, nll_coef=0.0, nll_scale=0.0, dpred=None, dlog_scale=None, want_dpred=True,
                want_dlog_scale=None, want_logprob=True, logprob=None, ref_logprob=None, h=None, margin=None, loss=None, coef=None):
    """The preference loss of a chosen and a rejected chunk per observation under the Laplace policy, and its gradient, in one launch (ovla.h
    "Preference optimisation on the Laplace policy": ovla_laplace_dpo): pred, ref_pred bf16 [B * chunk, adim], chosen, rejected fp32
    [B * chunk, adim], weight fp32 [B] (optional); the scale either `scale` (a scalar or [adim], shared by both policies) or log_scale with
    ref_log_scale bf16 [B * chunk, adim] and `bounds`; loss_type "sigmoid" / "ipo" (or 0 / 1)
    -> dict(logprob, ref_logprob fp32 [B * chunk, 2] (chosen, rejected), h fp32 [B, 2], margin, loss, coef fp32 [B], dpred, dlog_scale bf16
    [B * chunk, adim] or None).  With grad_scale the gradients go to `dpred` / `dlog_scale` (new tensors without them; dlog_scale by default
    only under a per-element scale; want_dpred=False / want_dlog_scale=False leaves that one out of the launch)."""
    _chk(pred, name="pred")
    chunk = int(chunk)
    assert pred.dim() == 2 and pred.is_contiguous() and chunk > 0 and pred.shape[0] % chunk == 0, f"pred: {tuple(pred.shape)} is not whole observations of {chunk} steps"
    (rows, adim), dev = pred.shape, pred.device
    B = rows // chunk
    rows_form = log_scale is not None or ref_log_scale is not None
    assert rows_form != (scale is not None), "the scale is either `scale` or log_scale with ref_log_scale"
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
    if want_logprob:
        logprob = f32(rows, 2) if logprob is None else logprob
        ref_logprob = f32(rows, 2) if ref_logprob is None else ref_logprob
    h, margin = f32(B, 2) if h is None else h, f32(B) if margin is None else margin
    loss, coef = f32(B) if loss is None else loss, f32(B) if coef is None else coef
    if want_dlog_scale is None:
        want_dlog_scale = rows_form
    if grad_scale is not None and dpred is None and want_dpred:
        dpred = torch.empty((rows, adim), dtype=BF16, device=dev)
    if grad_scale is not None and dlog_scale is None and want_dlog_scale:
        dlog_scale = torch.empty((rows, adim), dtype=BF16, device=dev)
    for t, dt, name, n in ((ref_pred, BF16, "ref_pred", rows * adim), (log_scale, BF16, "log_scale", rows * adim), (ref_log_scale, BF16, "ref_log_scale", rows * adim),
                           (chosen, torch.float32, "chosen", rows * adim), (rejected, torch.float32, "rejected", rows * adim), (weight, torch.float32, "weight", B),
                           (logprob, torch.float32, "logprob", rows * 2), (ref_logprob, torch.float32, "ref_logprob", rows * 2), (h, torch.float32, "h", B * 2),
                           (margin, torch.float32, "margin", B), (loss, torch.float32, "loss", B), (coef, torch.float32, "coef", B),
                           (dpred, BF16, "dpred", rows * adim), (dlog_scale, BF16, "dlog_scale", rows * adim)):
        if t is not None:
            _chk(t, dt, name)
            assert t.numel() == n and t.is_contiguous(), f"{name}: expected {n} contiguous elements"
    g = STRUCTS["ovla_laplace_dpo_args"]()
    g.pred, g.ref_pred, g.log_scale, g.ref_log_scale = pred.data_ptr(), _p(ref_pred), _p(log_scale), _p(ref_log_scale)
    g.chosen, g.rejected, g.weight = _p(chosen), _p(rejected), _p(weight)
    g.logprob, g.ref_logprob, g.h, g.margin, g.loss, g.coef = _p(logprob), _p(ref_logprob), h.data_ptr(), margin.data_ptr(), loss.data_ptr(), coef.data_ptr()
    g.dpred, g.dlog_scale = _p(dpred), _p(dlog_scale)
    g.s_lo, g.s_hi, g.beta, g.label_smoothing = float(bounds[0]), float(bounds[1]), float(beta), float(label_smoothing)
    g.grad_scale, g.nll_coef, g.nll_scale = float(grad_scale or 0.0), float(nll_coef), float(nll_scale)
    g.loss_type = DPO_LOSS_TYPES[loss_type] if isinstance(loss_type, str) else int(loss_type)
    g.B, g.chunk, g.adim = B, chunk, adim
    if not rows_form and 1 <= adim <= LAPLACE_MAX_ADIM:            # (otherwise the kernel's own refusal speaks)
        _set_laplace_scales(g, scale, adim)
    _lib.call("ovla_laplace_dpo", g, _stream())
    return dict(logprob=logprob, ref_logprob=ref_logprob, h=h, margin=margin, loss=loss, coef=coef, dpred=dpred, dlog_scale=dlog_scale)


def _chk_n(t, dtype, name, n):
    if t is not None:
        _chk(t, dtype, name)
        assert t.numel() == n and t.is_contiguous(), f"{name}: expected {n} contiguous elements"


def value_loss(u, chunk, *, returns=None, old_value=None, valid=None, value_clip=0.0, grad_scale=None, value=None, du=None, stats=None):
    """A value head's output pooled into one value per observation, and its clipped squared-error loss (ovla.h "Value head and generalised
    advantage estimation": ovla_value_loss): u bf16 [B * chunk, 1] -> value fp32 [B]; with `returns` fp32 [B] (and old_value fp32 [B] under
    value_clip > 0, valid int32 [B]) -> (value, du bf16 [B * chunk, 1] or None, stats fp32 [8]).  du exists with a grad_scale (or when given)."""
    _chk(u, name="u")
    chunk = int(chunk)
    assert u.is_contiguous() and chunk > 0 and u.numel() % chunk == 0, f"u: {tuple(u.shape)} is not whole observations of {chunk} steps"
    B, dev = u.numel() // chunk, u.device
    value = torch.empty(B, dtype=torch.float32, device=dev) if value is None else value
    if returns is not None:
        stats = torch.empty(8, dtype=torch.float32, device=dev) if stats is None else stats
        if grad_scale is not None and du is None:
            du = torch.empty((B * chunk, 1), dtype=BF16, device=dev)
    for t, dt, name, n in ((value, torch.float32, "value", B), (returns, torch.float32, "returns", B), (old_value, torch.float32, "old_value", B),
                           (valid, torch.int32, "valid", B), (du, BF16, "du", B * chunk), (stats, torch.float32, "stats", 8)):
        _chk_n(t, dt, name, n)
    g = STRUCTS["ovla_value_loss_args"]()
    g.u, g.returns, g.old_value, g.valid = u.data_ptr(), _p(returns), _p(old_value), _p(valid)
    g.value, g.du, g.stats = value.data_ptr(), _p(du), _p(stats)
    g.value_clip, g.grad_scale, g.B, g.chunk = float(value_clip), float(grad_scale or 0.0), B, chunk
    _lib.call("ovla_value_loss", g, _stream())
    return value if returns is None else (value, du, stats)


def _host_lengths(length, host_lengths):
    """The optional host copy of the trajectory lengths as a ctypes int32 array (None without one); the library validates it (OVLA_EINVAL)."""
    if host_lengths is None:
        return None
    vals = [int(v) for v in host_lengths]
    assert length is not None and len(vals) == length.numel(), "host_lengths must mirror length"
    return (ctypes.c_int32 * len(vals))(*vals)


def gae(reward, value, bootstrap, done, *, length=None, host_lengths=None, gamma=0.99, lam=0.95, adv=None, ret=None):
    """Generalised advantage estimation over a rollout buffer (ovla.h: ovla_gae): reward, value fp32 [N, T], bootstrap fp32 [N], done uint8
    [N, T] (1: the episode ended after this step), length int32 [N] (default T) -> (adv, ret fp32 [N, T]), +0 beyond a trajectory's length.
    host_lengths (optional, the same values on the host): an entry outside [0, T] raises before anything is launched."""
    _chk(reward, torch.float32, "reward")
    assert reward.dim() == 2 and reward.is_contiguous()
    (N, T), dev = reward.shape, reward.device
    adv = torch.empty((N, T), dtype=torch.float32, device=dev) if adv is None else adv
    ret = torch.empty((N, T), dtype=torch.float32, device=dev) if ret is None else ret
    for t, dt, name, n in ((value, torch.float32, "value", N * T), (bootstrap, torch.float32, "bootstrap", N), (done, torch.uint8, "done", N * T),
                           (length, torch.int32, "length", N), (adv, torch.float32, "adv", N * T), (ret, torch.float32, "ret", N * T)):
        _chk_n(t, dt, name, n)
    hl = _host_lengths(length, host_lengths)
    g = STRUCTS["ovla_gae_args"]()
    g.reward, g.value, g.bootstrap, g.done, g.length = reward.data_ptr(), _p(value), _p(bootstrap), _p(done), _p(length)
    g.length_host = ctypes.cast(hl, ctypes.c_void_p).value if hl is not None else None
    g.adv, g.ret = adv.data_ptr(), ret.data_ptr()
    g.gamma, g.gamma_lambda = float(gamma), float(np.float32(np.float64(gamma) * np.float64(lam)))   # gamma * lam in double, rounded once
    g.N, g.T = N, T
    _lib.call("ovla_gae", g, _stream())
    return adv, ret


def advantage_normalize(adv, *, length=None, host_lengths=None, eps=1e-8):
    """adv fp32 [N, T] in place <- (adv - mean) / (std + eps) over the elements inside their trajectory's length, mean and population std in
    double in the contract's fixed order (ovla.h: ovla_advantage_normalize).  N * T <= 2^20."""
    _chk(adv, torch.float32, "adv")
    assert adv.dim() == 2 and adv.is_contiguous()
    N, T = adv.shape
    _chk_n(length, torch.int32, "length", N)
    hl = _host_lengths(length, host_lengths)
    g = STRUCTS["ovla_advantage_normalize_args"]()
    g.adv, g.length = adv.data_ptr(), _p(length)
    g.length_host = ctypes.cast(hl, ctypes.c_void_p).value if hl is not None else None
    g.eps, g.N, g.T = float(eps), N, T
    _lib.call("ovla_advantage_normalize", g, _stream())
    return adv


def _chk_step(step):
    assert step.dtype == torch.int32 and step.numel() == 1 and step.is_cuda, "the DDIM step index is one int32 on the device"


def ddim_prepare(step, temb_table, temb, sample, noisy):
    """Top of DDIM step k = *step (ovla.h: ovla_ddim_prepare): temb[b] = temb_table[k] for every row of temb bf16 [B, D], noisy = bf16(sample)
    (sample fp32, noisy bf16, n elements each).  k outside [0, n_steps): nothing is written."""
    _chk_step(step)
    _chk(temb_table, name="temb_table"), _chk(temb, name="temb"), _chk(noisy, name="noisy"), _chk(sample, torch.float32, "sample")
    assert temb_table.dim() == 2 and temb.dim() == 2 and temb.shape[1] == temb_table.shape[1]
    assert temb_table.is_contiguous() and temb.is_contiguous() and sample.is_contiguous() and noisy.is_contiguous() and noisy.numel() == sample.numel()
    g = STRUCTS["ovla_ddim_prepare_args"]()
    g.step, g.temb_table, g.temb, g.sample, g.noisy = step.data_ptr(), temb_table.data_ptr(), temb.data_ptr(), sample.data_ptr(), noisy.data_ptr()
    g.n_steps, g.B, g.D, g.n = temb_table.shape[0], temb.shape[0], temb.shape[1], sample.numel()
    _lib.call("ovla_ddim_prepare", g, _stream())


def ddim_step(sample, eps, coef, step):
    """End of DDIM step k = *step (ovla.h: ovla_ddim_step): sample (fp32, in place) <- DDIMScheduler.step(eps, t_k, sample).prev_sample rounded
    through bf16, with eps the head's bf16 output and coef fp32 [n_steps, 4] from DDIMScheduler.step_coefficients(); then *step = k + 1.
    k outside [0, n_steps): nothing is written."""
    _chk_step(step)
    _chk(sample, torch.float32, "sample"), _chk(eps, name="eps"), _chk(coef, torch.float32, "coef")
    assert coef.dim() == 2 and coef.shape[1] == 4 and coef.is_contiguous() and sample.is_contiguous() and eps.is_contiguous()
    assert eps.numel() == sample.numel()
    g = STRUCTS["ovla_ddim_step_args"]()
    g.sample, g.eps, g.coef, g.step = sample.data_ptr(), eps.data_ptr(), coef.data_ptr(), step.data_ptr()
    g.n_steps, g.n = coef.shape[0], sample.numel()
    _lib.call("ovla_ddim_step", g, _stream())
    return sample


def diffusion_noise(actions, ab, temb_table, *, seed, call, stream=0, noise=None, noisy=None, temb=None, timesteps=None):
    """sample_noisy_actions in one launch (ovla.h "Diffusion noise": ovla_diffusion_noise): actions bf16 [B, n] (row stride free), ab fp32 [T, 2]
    (DDIMScheduler.add_noise_coefficients()), temb_table bf16 [T, D] -> (noise bf16 [B, n], noisy bf16 [B, n], temb bf16 [B, D], timesteps int32
    [B]), every one a pure function of (seed, call, stream, sample, element).  `stream`: 0 training noise, 2 the sampler's start noise.  Outputs
    given by the caller may have row strides of their own."""
    _chk(actions, name="actions"), _chk(ab, torch.float32, "ab"), _chk(temb_table, name="temb_table")
    assert actions.dim() == 2 and actions.stride(1) == 1 and ab.dim() == 2 and ab.shape[1] == 2 and ab.is_contiguous()
    assert temb_table.dim() == 2 and temb_table.is_contiguous() and temb_table.shape[0] == ab.shape[0]
    (B, n), (T, D), dev = actions.shape, temb_table.shape, actions.device
    noise = torch.empty((B, n), dtype=BF16, device=dev) if noise is None else noise
    noisy = torch.empty((B, n), dtype=BF16, device=dev) if noisy is None else noisy
    temb = torch.empty((B, D), dtype=BF16, device=dev) if temb is None else temb
    timesteps = torch.empty(B, dtype=torch.int32, device=dev) if timesteps is None else timesteps
    for t, name, cols in ((noise, "noise", n), (noisy, "noisy", n), (temb, "temb", D)):
        _chk(t, name=name)
        assert t.dim() == 2 and t.shape == (B, cols) and t.stride(1) == 1, f"{name}: expected [{B}, {cols}] with unit column stride"
    _chk(timesteps, torch.int32, "timesteps")
    assert timesteps.shape == (B,) and timesteps.is_contiguous()
    g = STRUCTS["ovla_diffusion_noise_args"]()
    g.actions, g.ld_actions, g.ab, g.temb_table = actions.data_ptr(), actions.stride(0), ab.data_ptr(), temb_table.data_ptr()
    g.noise, g.ld_noise, g.noisy, g.ld_noisy, g.temb, g.ld_temb = noise.data_ptr(), noise.stride(0), noisy.data_ptr(), noisy.stride(0), temb.data_ptr(), temb.stride(0)
    g.timesteps = timesteps.data_ptr()
    g.seed_lo, g.seed_hi, g.call, g.stream = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, int(call) & 0xFFFFFFFF, int(stream) & 0xFFFFFFFF
    g.B, g.n, g.D, g.T = B, n, D, T
    _lib.call("ovla_diffusion_noise", g, _stream())
    return noise, noisy, temb, timesteps


def head_out_fwd(x, W, b, target=None, loss_sum=None, mse=False, out=None):
    rows, dim = x.shape
    adim = W.shape[0]
    pred = torch.empty((rows, adim), dtype=BF16, device=x.device) if out is None else out
    assert pred.shape == (rows, adim) and pred.dtype == BF16 and pred.is_contiguous()
    g = STRUCTS["ovla_head_out_fwd_args"]()
    g.x, g.W, g.b, g.pred, g.target, g.loss_sum = x.data_ptr(), W.data_ptr(), _p(b), pred.data_ptr(), _p(target), _p(loss_sum)
    g.rows, g.dim, g.adim, g.mse = rows, dim, adim, int(mse)
    _lib.call("ovla_head_out_fwd", g, _stream())
    return pred


def head_out_bwd(x, W, pred, target, dloss_scale, dW, db, mse=False, dpred=None, out=None):
    """Backward of the head tail.  Either (pred, target, dloss_scale) -- fused L1/MSE gradient -- or an explicit dpred."""
    rows, dim = x.shape
    adim = W.shape[0]
    dx = torch.empty_like(x) if out is None else out
    assert dx.shape == x.shape and dx.dtype == BF16 and dx.is_contiguous()
    g = STRUCTS["ovla_head_out_bwd_args"]()
    g.x, g.W, g.pred, g.target, g.dpred = x.data_ptr(), W.data_ptr(), _p(pred), _p(target), _p(dpred)
    g.dloss_scale, g.mse = dloss_scale, int(mse)
    g.dx, g.dW, g.db, g.rows, g.dim, g.adim = dx.data_ptr(), _p(dW), _p(db), rows, dim, adim
    _lib.call("ovla_head_out_bwd", g, _stream())
    return dx


def adamw(param, exp_avg, exp_avg_sq, grad, *, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0):
    g = STRUCTS["ovla_adamw_args"]()
    g.param, g.exp_avg, g.exp_avg_sq, g.grad = param.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), grad.data_ptr()
    g.n, g.is_bf16, g.step = param.numel(), int(param.dtype == BF16), step
    g.lr, g.beta1, g.beta2, g.eps, g.weight_decay, g.grad_scale = lr, beta1, beta2, eps, weight_decay, grad_scale
    assert grad.dtype == torch.float32 and exp_avg.dtype == param.dtype and exp_avg_sq.dtype == param.dtype
    _lib.call("ovla_adamw", g, _stream())


def ema_update(param, shadow, one_minus_decay):
    """shadow <- shadow - omd * (shadow - float(param)) in place (ovla.h "Weight EMA"); `one_minus_decay` is a Python float that the argument
    struct rounds to fp32 once."""
    assert shadow.dtype == torch.float32 and param.dtype in (BF16, torch.float32) and shadow.numel() == param.numel()
    assert param.is_contiguous() and shadow.is_contiguous()
    g = STRUCTS["ovla_ema_update_args"]()
    g.param, g.shadow, g.n, g.is_bf16, g.one_minus_decay = param.data_ptr(), shadow.data_ptr(), param.numel(), int(param.dtype == BF16), one_minus_decay
    _lib.call("ovla_ema_update", g, _stream())


# -- gradient-norm clipping and the non-finite step guard (ovla.h "Gradient-norm clipping") ---------------------------------------------------
GRAD_SUMSQ_CHUNK = 8192   # OVLA_GRAD_SUMSQ_CHUNK: elements one workgroup reduces to one partial


def grad_sumsq_workspace_elems(n: int) -> int:
    """Doubles of workspace ovla_grad_sumsq needs for n elements (one partial per chunk)."""
    return (int(n) + GRAD_SUMSQ_CHUNK - 1) // GRAD_SUMSQ_CHUNK


def grad_clip_state(device):
    """A zeroed device ovla_grad_clip_state as six 32-bit words: (coef, norm) fp32, then skip, n_steps, n_clipped, n_skipped int32."""
    assert ctypes.sizeof(STRUCTS["ovla_grad_clip_state"]) == 24
    return torch.zeros(6, dtype=torch.int32, device=device)


def read_grad_clip_state(state) -> dict:
    """The state on the host (this synchronises): {norm, coef, skip, steps, clipped, skipped}."""
    raw = state.detach().cpu().contiguous().numpy().tobytes()
    s = STRUCTS["ovla_grad_clip_state"].from_buffer_copy(raw)
    return {"norm": float(s.norm), "coef": float(s.coef), "skip": int(s.skip), "steps": int(s.n_steps), "clipped": int(s.n_clipped),
            "skipped": int(s.n_skipped)}


def grad_sumsq(grad, slots, slot, workspace, *, is_bf16, grad_scale=1.0, n=None):
    """slots[slot] <- sum of squares, in double and in the contract's fixed order, of the first n (default: all) elements of the flat fp32
    gradient buffer `grad` as AdamW sees them (times grad_scale, rounded to bf16 for a bf16 parameter buffer)."""
    assert grad.dtype == torch.float32 and slots.dtype == torch.float64 and workspace.dtype == torch.float64
    assert grad.is_contiguous() and slots.is_contiguous() and workspace.is_contiguous() and 0 <= slot < slots.numel()
    g = STRUCTS["ovla_grad_sumsq_args"]()
    g.grad, g.n, g.is_bf16, g.grad_scale = grad.data_ptr(), grad.numel() if n is None else n, int(is_bf16), grad_scale
    g.slots, g.slot, g.workspace, g.workspace_bytes = slots.data_ptr(), slot, workspace.data_ptr(), workspace.numel() * 8
    _lib.call("ovla_grad_sumsq", g, _stream())


# -- per-tensor statistics (ovla.h "Per-tensor statistics"): the segmented form of grad_sumsq -------------------------------------------------
TENSOR_STATS_PARTIAL_BYTES = 32   # OVLA_TENSOR_STATS_PARTIAL_BYTES: one ovla_tensor_stat record per chunk
TENSOR_STAT_DTYPE = [("grad_sumsq", "<f8"), ("param_sumsq", "<f8"), ("grad_absmax", "<f4"), ("n_bad_steps", "<i4"), ("n_nonfinite", "<i8")]


def tensor_stats_plan(segments, buffer_n: int, device=None) -> dict:
    """Checks a segment table [(offset, n), ...] (elements of a flat buffer of `buffer_n` elements: ascending, disjoint, offset % 8 == 0) on
    the host and returns the plan of ovla_tensor_stats for it: `chunk_start` (numpy int32 [n_segs + 1], the prefix sums of the segments'
    chunk counts), `total_chunks`, `n_segs`, the table as `segs_host`, and with `device` the device copies `segs` / `chunk_start_dev` (made
    here, once).  Host only when `device` is None: no device call."""
    import numpy as np

    assert ctypes.sizeof(STRUCTS["ovla_tensor_seg"]) == 16 and ctypes.sizeof(STRUCTS["ovla_tensor_stat"]) == TENSOR_STATS_PARTIAL_BYTES
    segs = np.ascontiguousarray(np.asarray(list(segments), dtype=np.int64).reshape(-1, 2))
    chunk_start = np.zeros(segs.shape[0] + 1, np.int32)
    rc = _lib.lib().ovla_tensor_stats_plan(ctypes.cast(segs.ctypes.data, ctypes.POINTER(STRUCTS["ovla_tensor_seg"])), segs.shape[0], int(buffer_n),
                                           chunk_start.ctypes.data)
    _lib.check(rc, "ovla_tensor_stats_plan")
    plan = dict(segs_host=segs, chunk_start=chunk_start, n_segs=int(segs.shape[0]), total_chunks=int(chunk_start[-1]))
    if device is not None:
        plan["segs"] = torch.from_numpy(segs.reshape(-1)).to(device)
        plan["chunk_start_dev"] = torch.from_numpy(chunk_start).to(device)
    return plan


def tensor_stats_buffers(n_segs: int, total_chunks: int, device):
    """(out, partials): `out` zeroed int64 [n_segs, 4] (one 32-byte ovla_tensor_stat per segment: the n_bad_steps latches start at 0),
    `partials` int64 [max(1, total_chunks), 4] (one record per chunk; its contents never matter)."""
    return (torch.zeros((n_segs, 4), dtype=torch.int64, device=device), torch.empty((max(1, total_chunks), 4), dtype=torch.int64, device=device))


def tensor_stats_args(plan, grad, param, out, partials, *, grad_round_bf16, grad_scale=1.0):
    """The ovla_tensor_stats_args of tensor_stats, as that call fills them (the tests change one field at a time for the refusals)."""
    assert grad.dtype == torch.float32 and param.dtype in (BF16, torch.float32) and grad.is_contiguous() and param.is_contiguous()
    assert out.dtype == torch.int64 and partials.dtype == torch.int64 and out.is_contiguous() and partials.is_contiguous()
    assert out.numel() * 8 >= TENSOR_STATS_PARTIAL_BYTES * plan["n_segs"]
    g = STRUCTS["ovla_tensor_stats_args"]()
    g.grad, g.param, g.param_is_bf16, g.grad_round_bf16, g.grad_scale = grad.data_ptr(), param.data_ptr(), int(param.dtype == BF16), int(grad_round_bf16), grad_scale
    g.segs, g.chunk_start, g.n_segs, g.total_chunks = plan["segs"].data_ptr(), plan["chunk_start_dev"].data_ptr(), plan["n_segs"], plan["total_chunks"]
    g.partials, g.partials_bytes, g.out = partials.data_ptr(), partials.numel() * 8, out.data_ptr()
    return g


def tensor_stats(plan, grad, param, out, partials, *, grad_round_bf16, grad_scale=1.0):
    """out[t] <- the statistics of segment t of the flat fp32 gradient buffer `grad` as AdamW sees it (times grad_scale, rounded to bf16 when
    `grad_round_bf16`) and of the flat parameter buffer `param` (bf16 or fp32), one launch pair for the whole table; out[t].n_bad_steps is
    incremented where the segment holds a non-finite gradient.  `plan` is tensor_stats_plan(..., device=...)'s.  Nothing is read back."""
    _lib.call("ovla_tensor_stats", tensor_stats_args(plan, grad, param, out, partials, grad_round_bf16=grad_round_bf16, grad_scale=grad_scale), _stream())


def read_tensor_stats(out, n_segs=None):
    """`out` on the host (this synchronises) as a numpy structured array of ovla_tensor_stat records: grad_sumsq, param_sumsq (double),
    grad_absmax (float), n_bad_steps (int32), n_nonfinite (int64)."""
    import numpy as np

    raw = out.detach().cpu().contiguous().numpy().reshape(-1, 4)
    rec = raw.view(np.dtype(TENSOR_STAT_DTYPE)).reshape(-1)
    return rec if n_segs is None else rec[:n_segs]


def grad_clip_coef(slots, state, max_norm, skip_nonfinite=True, n_slots=None):
    """state <- norm over slots[0 .. n_slots), clip coefficient, skip flag and counters (one tiny launch, nothing read back)."""
    assert slots.dtype == torch.float64 and slots.is_contiguous() and state.dtype == torch.int32 and state.numel() == 6 and state.is_contiguous()
    g = STRUCTS["ovla_grad_clip_coef_args"]()
    g.slots, g.n_slots, g.max_norm, g.skip_nonfinite, g.state = slots.data_ptr(), slots.numel() if n_slots is None else n_slots, max_norm, int(skip_nonfinite), state.data_ptr()
    _lib.call("ovla_grad_clip_coef", g, _stream())


def adamw_clipped(param, exp_avg, exp_avg_sq, grad, state, *, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0):
    """ops.adamw on the gradient scaled by the state's coefficient; changes nothing when the state says skip."""
    g = STRUCTS["ovla_adamw_clipped_args"]()
    g.param, g.exp_avg, g.exp_avg_sq, g.grad = param.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), grad.data_ptr()
    g.n, g.is_bf16, g.step = param.numel(), int(param.dtype == BF16), step
    g.lr, g.beta1, g.beta2, g.eps, g.weight_decay, g.grad_scale = lr, beta1, beta2, eps, weight_decay, grad_scale
    g.clip_state = state.data_ptr()
    assert grad.dtype == torch.float32 and exp_avg.dtype == param.dtype and exp_avg_sq.dtype == param.dtype
    assert state.dtype == torch.int32 and state.numel() == 6
    _lib.call("ovla_adamw_clipped", g, _stream())


# -- AdamW on fp32 master weights (ovla.h "AdamW on fp32 master weights") ----------------------------------------------------------------------
ADAMW_MASTER_MAX_BLOCKS = 2048   # OVLA_ADAMW_MASTER_MAX_BLOCKS: workgroups (of 256 lanes, 4 elements each) one trip of the grid-stride loop covers


def adamw_master(master, exp_avg, exp_avg_sq, param, grad, *, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0,
                 clip_state=None):
    """The fp32 AdamW update of (master, exp_avg, exp_avg_sq) with the fp32 gradient, and param <- bf16_rne(master), in one launch.  With
    `clip_state` the gradient is scaled by the state's coefficient, and nothing is written when the state says skip."""
    assert master.dtype == exp_avg.dtype == exp_avg_sq.dtype == grad.dtype == torch.float32 and param.dtype == BF16
    assert master.numel() == exp_avg.numel() == exp_avg_sq.numel() == grad.numel() == param.numel()
    assert all(t.is_contiguous() for t in (master, exp_avg, exp_avg_sq, param, grad))
    g = STRUCTS["ovla_adamw_master_args"]()
    g.master, g.exp_avg, g.exp_avg_sq, g.param, g.grad = master.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), param.data_ptr(), grad.data_ptr()
    g.n, g.step = param.numel(), step
    g.lr, g.beta1, g.beta2, g.eps, g.weight_decay, g.grad_scale = lr, beta1, beta2, eps, weight_decay, grad_scale
    if clip_state is not None:
        assert clip_state.dtype == torch.int32 and clip_state.numel() == 6
        g.clip_state = clip_state.data_ptr()
    _lib.call("ovla_adamw_master", g, _stream())


def cvt_f32_to_bf16(src, dst=None, scale=1.0):
    if dst is None:
        dst = torch.empty(src.shape, dtype=BF16, device=src.device)
    g = STRUCTS["ovla_cvt_args"]()
    g.src, g.dst, g.n, g.scale = src.data_ptr(), dst.data_ptr(), src.numel(), scale
    _lib.call("ovla_cvt_f32_to_bf16", g, _stream())
    return dst


def cvt_bf16_to_f32(src, dst=None, scale=1.0):
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    _lib.check(_lib.lib().ovla_cvt_bf16_to_f32(src.data_ptr(), dst.data_ptr(), src.numel(), scale, _stream()), "ovla_cvt_bf16_to_f32")
    return dst


def transpose(src, dst=None):
    _chk(src)
    rows, cols = src.shape
    assert src.stride(1) == 1
    if dst is None:
        dst = torch.empty((cols, rows), dtype=BF16, device=src.device)
    g = STRUCTS["ovla_transpose_args"]()
    g.src, g.dst, g.rows, g.cols, g.lds, g.ldd = src.data_ptr(), dst.data_ptr(), rows, cols, src.stride(0), dst.stride(0)
    _lib.call("ovla_transpose_bf16", g, _stream())
    return dst


def selftest_layouts(device):
    out = torch.zeros((4, 64, 16), dtype=torch.float32, device=device)
    src = torch.arange(512, dtype=torch.float32, device=device).to(BF16)
    _lib.check(_lib.lib().ovla_selftest_layouts(out.data_ptr(), src.data_ptr(), _stream()), "ovla_selftest_layouts")
    return out
