// grad_clip.hip -- global gradient-norm clipping and the non-finite step guard in front of the fused AdamW (torch.nn.utils.clip_grad_norm_;
// the reference's loop, vla-scripts/finetune.py:952-1100, has neither).  The contract is in ovla.h "Gradient-norm clipping"; the numpy
// restatement is tests/grad_clip_reference.py.  Three kernels, each complete at its kernel boundary:
//   ovla_grad_sumsq      sum of squares of one flat gradient buffer in double, in a FIXED order: one workgroup per chunk -> partials, one
//                        workgroup over the partials -> slots[slot].  Reads 4 bytes per element (AdamW on the same buffer moves 16 / 28).
//   ovla_grad_clip_coef  one lane: total over the slots, norm, coefficient, skip flag and counters into the device state.
//   ovla_adamw_clipped   ovla_adamw's element update (adamw_elem.h) on the scaled gradient; a no-op when the state says skip.
// No atomics, no grid barrier, no spin-wait; nothing is read back.
#pragma clang fp contract(off)
#include "adamw_elem.h"
#include "sumsq_order.h"

namespace {

using namespace sumsq_order;   // kChunk, kLanes, kTrips, sq and THE TREE (block_tree): shared with tensor_stats.hip

template <bool BF>
__global__ __launch_bounds__(kLanes) void sumsq_chunk_kernel(const float* __restrict__ g, int64_t n, float scale, double* __restrict__ partials) {
  __shared__ double wave_total[4];
  const int t = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * kChunk;             // the grid is exactly ceil(n / kChunk) workgroups: c0 < n
  const int64_t left = n - c0;
  const int len = left < kChunk ? (int)left : kChunk;
  const f32x4* gv = reinterpret_cast<const f32x4*>(g + c0);    // 16-byte aligned: g is, and c0 is a multiple of 4
  double acc = 0.0;
  if (len == kChunk) {                                         // every load of the chunk in flight before the first add
    f32x4 x[kTrips];
#pragma unroll
    for (int k = 0; k < kTrips; ++k) x[k] = gv[k * kLanes + t];
#pragma unroll
    for (int k = 0; k < kTrips; ++k) {
      acc += sq<BF>(x[k][0], scale); acc += sq<BF>(x[k][1], scale); acc += sq<BF>(x[k][2], scale); acc += sq<BF>(x[k][3], scale);
    }
  } else {                                                     // the last chunk: the same lanes, the same order, bounds checked
    const int groups = len >> 2, rest = len & 3;
    for (int k = 0; k < kTrips; ++k) {
      const int gi = k * kLanes + t;
      if (gi < groups) {
        const f32x4 x = gv[gi];
        acc += sq<BF>(x[0], scale); acc += sq<BF>(x[1], scale); acc += sq<BF>(x[2], scale); acc += sq<BF>(x[3], scale);
      } else if (gi == groups) {                               // the scalar tail: n % 4 elements, read one by one by the lane that owns their group
        for (int j = 0; j < rest; ++j) acc += sq<BF>(g[c0 + 4 * (int64_t)gi + j], scale);
      }
    }
  }
  const double total = block_tree(acc, wave_total);
  if (t == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(kLanes) void sumsq_final_kernel(const double* __restrict__ partials, int64_t n_partials, double* __restrict__ out) {
  __shared__ double wave_total[4];
  double acc = 0.0;
  int64_t j = threadIdx.x;
  for (; j + 3 * kLanes < n_partials; j += 4 * kLanes) {   // four loads in flight, added in the same ascending order (a big buffer has 50+ per lane)
    double x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = partials[j + u * kLanes];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += x[u];
  }
  for (; j < n_partials; j += kLanes) acc += partials[j];
  const double total = block_tree(acc, wave_total);
  if (threadIdx.x == 0) *out = total;
}

__global__ __launch_bounds__(64) void clip_coef_kernel(const double* __restrict__ slots, int n_slots, float max_norm, int skip_nonfinite,
                                                       ovla_grad_clip_state* __restrict__ st) {
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int i = 0; i < n_slots; ++i) total += slots[i];
  const float norm = (float)sqrt(total);
  st->n_steps += 1;
  st->norm = norm;
  if (skip_nonfinite && !__builtin_isfinite(total)) {
    st->skip = 1;
    st->coef = 1.f;
    st->n_skipped += 1;
    return;
  }
  const float coef = fminf(1.f, max_norm / (norm + 1e-6f));
  st->skip = 0;
  st->coef = coef;
  if (coef < 1.f) st->n_clipped += 1;
}

template <bool BF, class T>
__global__ __launch_bounds__(256) void adamw_clipped_kernel(T* __restrict__ p, T* __restrict__ m, T* __restrict__ v, const float* __restrict__ g, int64_t n,
                                                            AdamScalars s, const ovla_grad_clip_state* __restrict__ st) {
  if (st->skip) return;   // uniform: every workgroup leaves before it writes anything
  const float coef = st->coef;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (BF) {
      const float grad = bfround(bfround(g[i] * s.grad_scale) * coef);   // grad.mul_(clip_coef) on the bf16 .grad
      adamw_elem_bf16(p, m, v, i, grad, s);
    } else {
      const float grad = (g[i] * s.grad_scale) * coef;
      adamw_elem_f32(p, m, v, i, grad, s);
    }
  }
}

static inline bool aligned8(const void* p) { return (((uintptr_t)p) & 7) == 0; }
}  // namespace

extern "C" int ovla_grad_sumsq(const ovla_grad_sumsq_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->grad && a->slots && a->workspace, "ovla_grad_sumsq: null pointer");
  OVLA_REQUIRE(a->n >= 0 && a->slot >= 0, "ovla_grad_sumsq: n = %lld, slot = %d", (long long)a->n, a->slot);
  OVLA_REQUIRE(aligned16(a->grad) && aligned8(a->slots) && aligned8(a->workspace),
               "ovla_grad_sumsq: grad must be 16-byte aligned, slots and workspace 8-byte aligned");
  const int64_t n_partials = (a->n + kChunk - 1) / kChunk;
  OVLA_REQUIRE(n_partials <= 0x7fffffffLL, "ovla_grad_sumsq: n = %lld is more than a grid covers", (long long)a->n);
  OVLA_REQUIRE(a->workspace_bytes >= 8 * n_partials, "ovla_grad_sumsq: workspace of %lld bytes, %lld needed", (long long)a->workspace_bytes,
               (long long)(8 * n_partials));
  if (n_partials > 0) {
    if (a->is_bf16)
      hipLaunchKernelGGL(sumsq_chunk_kernel<true>, dim3((unsigned)n_partials), dim3(kLanes), 0, stream, a->grad, a->n, a->grad_scale, a->workspace);
    else
      hipLaunchKernelGGL(sumsq_chunk_kernel<false>, dim3((unsigned)n_partials), dim3(kLanes), 0, stream, a->grad, a->n, a->grad_scale, a->workspace);
    OVLA_CHECK_LAUNCH("ovla_grad_sumsq");
  }
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(kLanes), 0, stream, (const double*)a->workspace, n_partials, a->slots + a->slot);   // n == 0: writes 0.0
  OVLA_CHECK_LAUNCH("ovla_grad_sumsq");
  return OVLA_OK;
}

extern "C" int ovla_grad_clip_coef(const ovla_grad_clip_coef_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->slots && a->state, "ovla_grad_clip_coef: null pointer");
  OVLA_REQUIRE(a->n_slots >= 1, "ovla_grad_clip_coef: n_slots = %d", a->n_slots);
  OVLA_REQUIRE(a->max_norm > 0.0f, "ovla_grad_clip_coef: max_norm = %g (a positive number or +inf)", (double)a->max_norm);   // false for NaN as well
  OVLA_REQUIRE(aligned8(a->slots) && (((uintptr_t)a->state) & 3) == 0, "ovla_grad_clip_coef: slots must be 8-byte, state 4-byte aligned");
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(64), 0, stream, a->slots, a->n_slots, a->max_norm, a->skip_nonfinite != 0,
                     (ovla_grad_clip_state*)a->state);
  OVLA_CHECK_LAUNCH("ovla_grad_clip_coef");
  return OVLA_OK;
}

extern "C" int ovla_adamw_clipped(const ovla_adamw_clipped_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->param && a->exp_avg && a->exp_avg_sq && a->grad && a->clip_state && a->n > 0 && a->step >= 1, "ovla_adamw_clipped: bad arguments");
  const AdamScalars s = adam_scalars(*a);
  int64_t blocks = (a->n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  const ovla_grad_clip_state* st = (const ovla_grad_clip_state*)a->clip_state;
  if (a->is_bf16)
    hipLaunchKernelGGL((adamw_clipped_kernel<true, bf16_bits>), dim3((unsigned)blocks), dim3(256), 0, stream, (bf16_bits*)a->param, (bf16_bits*)a->exp_avg,
                       (bf16_bits*)a->exp_avg_sq, a->grad, a->n, s, st);
  else
    hipLaunchKernelGGL((adamw_clipped_kernel<false, float>), dim3((unsigned)blocks), dim3(256), 0, stream, (float*)a->param, (float*)a->exp_avg,
                       (float*)a->exp_avg_sq, a->grad, a->n, s, st);
  OVLA_CHECK_LAUNCH("ovla_adamw_clipped");
  return OVLA_OK;
}
