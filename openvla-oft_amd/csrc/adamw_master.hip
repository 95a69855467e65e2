// adamw_master.hip -- the fused AdamW for a bf16 parameter buffer whose optimizer state is kept in fp32: an fp32 master copy and fp32 moments
// take adamw_elem.h's fp32 element update, and the bf16 parameter the forward reads is the master rounded to nearest even.  The reference
// (vla-scripts/finetune.py:952, torch.optim.AdamW on bf16 parameters) keeps all three in bf16, where exp_avg_sq.mul_(0.999) returns its input
// and an update below half an ulp of the parameter is lost; this is the opt-in alternative.  The contract is in ovla.h "AdamW on fp32 master
// weights"; the restatement is tests/adamw_master_reference.py.
#pragma clang fp contract(off)
// Elementwise and memory-bound, 30 bytes per element (grad 4 + master, m, v 12 read; 12 + 2 written).  The body moves four elements per lane
// and trip: 16-byte loads of grad, master, m and v, 16-byte stores of the three, one 8-byte store of the four bf16 values; the last n % 4
// elements go one per lane.  An element's result does not depend on which of the two paths, which lane or which trip computes it.  The
// arithmetic (two divisions and a square root per element, correctly rounded) is about a third of the VALU time the traffic leaves, so the
// grid-stride loop is software-pipelined one trip deep.
#include "adamw_elem.h"

namespace {

constexpr int kMaxBlocks = OVLA_ADAMW_MASTER_MAX_BLOCKS;   // 8 workgroups of 256 on each of the 256 compute units; the grid-stride loop takes the rest

// 16-byte group q of an fp32 stream, past the caches
OVLA_DEV f32x4 ld4(const float* p, int64_t q) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + q); }
OVLA_DEV void st4(float* p, int64_t q, f32x4 x) { __builtin_nontemporal_store(x, reinterpret_cast<f32x4*>(p) + q); }

template <bool CLIP>
OVLA_DEV AdamElemF32 master1(float p, float m, float v, float g, float coef, const AdamScalars& s) {
  float grad = g * s.grad_scale;     // the optimizer-side dtype is fp32: no bf16 rounding
  if (CLIP) grad = grad * coef;      // grad.mul_(clip_coef), as ovla_adamw_clipped does for an fp32 buffer
  return adamw_update_f32(p, m, v, grad, s);
}

template <bool CLIP>
__global__ __launch_bounds__(256) void adamw_master_kernel(float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
                                                           bf16_bits* __restrict__ param, const float* __restrict__ g, int64_t n, AdamScalars s,
                                                           const ovla_grad_clip_state* __restrict__ st) {
  float coef = 1.f;
  if (CLIP) {
    if (st->skip) return;   // uniform: every workgroup leaves before it writes anything
    coef = st->coef;
  }
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  const int64_t groups = n >> 2;
  // The next trip's four loads are issued before this trip's arithmetic and stores, and the fp32 streams, which nothing reads again before the
  // next optimizer step, go past the caches (nontemporal); the bf16 parameters are stored normally: refresh_derived reads them next.  Measured on
  // the 151 M-element head buffer, variants alternated in one process: 705-903 us against 846-941 us for the plain loop on the same box.
  int64_t q = tid;
  f32x4 gv, pv, mv, vv;
  if (q < groups) {
    gv = ld4(g, q); pv = ld4(master, q); mv = ld4(m, q); vv = ld4(v, q);
  }
  while (q < groups) {
    const int64_t qn = q + stride;
    f32x4 gn, pn, mn, vn;
    if (qn < groups) {
      gn = ld4(g, qn); pn = ld4(master, qn); mn = ld4(m, qn); vn = ld4(v, qn);
    }
    bf16x4_bits ob;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const AdamElemF32 r = master1<CLIP>(pv[j], mv[j], vv[j], gv[j], coef, s);
      pv[j] = r.p; mv[j] = r.m; vv[j] = r.v;
      ob[j] = (short)f2bf(r.p);
    }
    st4(master, q, pv);
    st4(m, q, mv);
    st4(v, q, vv);
    reinterpret_cast<bf16x4_bits*>(param)[q] = ob;
    gv = gn; pv = pn; mv = mn; vv = vn;
    q = qn;
  }
  const int64_t i = (groups << 2) + tid;   // scalar tail: fewer than 4 elements, the first lanes of the grid
  if (i < n) {
    const AdamElemF32 r = master1<CLIP>(master[i], m[i], v[i], g[i], coef, s);
    master[i] = r.p; m[i] = r.m; v[i] = r.v;
    param[i] = f2bf(r.p);
  }
}
}  // namespace

extern "C" int ovla_adamw_master(const ovla_adamw_master_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->master && a->exp_avg && a->exp_avg_sq && a->param && a->grad, "ovla_adamw_master: null pointer");
  OVLA_REQUIRE(a->n > 0 && a->step >= 1, "ovla_adamw_master: n = %lld, step = %d", (long long)a->n, a->step);
  OVLA_REQUIRE(aligned16(a->master) && aligned16(a->exp_avg) && aligned16(a->exp_avg_sq) && aligned16(a->param) && aligned16(a->grad),
               "ovla_adamw_master: master, exp_avg, exp_avg_sq, param and grad must be 16-byte aligned");
  const AdamScalars s = adam_scalars(*a);
  int64_t blocks = (a->n + 256 * 4 - 1) / (256 * 4);   // >= 1, so the tail's lanes (< 4 of them) always exist
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  const ovla_grad_clip_state* st = (const ovla_grad_clip_state*)a->clip_state;
  if (st)
    hipLaunchKernelGGL(adamw_master_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, a->master, a->exp_avg, a->exp_avg_sq,
                       (bf16_bits*)a->param, a->grad, a->n, s, st);
  else
    hipLaunchKernelGGL(adamw_master_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, a->master, a->exp_avg, a->exp_avg_sq,
                       (bf16_bits*)a->param, a->grad, a->n, s, st);
  OVLA_CHECK_LAUNCH("ovla_adamw_master");
  return OVLA_OK;
}
