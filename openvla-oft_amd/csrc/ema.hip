// ema.hip -- exponential moving average of a flat parameter buffer into an fp32 shadow: the step a fine-tune takes right after the optimizer
// step (vla-scripts/finetune.py:952 builds the optimizer; the reference has NO EMA -- this extends that call site with the update of
// diffusers' EMAModel, `s.sub_(omd * (s - p))`).  The contract is in ovla.h "Weight EMA":
//     shadow[i] = s - omd * (s - float(param[i]))
// three fp32 operations, each rounded on its own:
#pragma clang fp contract(off)
// Elementwise and memory-bound: 10 bytes per element for a bf16 parameter (2 read + 4 read + 4 written), 12 for fp32.  The body moves 16 bytes
// per lane and instruction (8 bf16 / 4 fp32 of the parameter, 4 fp32 of the shadow), the last n % 8 (n % 4) elements go one per lane.  An
// element's result does not depend on which of the two paths, which lane or which trip of the grid-stride loop computes it.
#include "common.h"

namespace {

OVLA_DEV float ema1(float s, float p, float omd) {
  const float d = s - p;
  const float u = omd * d;
  return s - u;
}
OVLA_DEV f32x4 ema4(f32x4 s, float p0, float p1, float p2, float p3, float omd) {
  f32x4 r;
  r[0] = ema1(s[0], p0, omd); r[1] = ema1(s[1], p1, omd); r[2] = ema1(s[2], p2, omd); r[3] = ema1(s[3], p3, omd);
  return r;
}

constexpr int kMaxBlocks = 2048;   // 8 workgroups of 256 on each of the 256 compute units; the grid-stride loop takes the rest

__global__ __launch_bounds__(256) void ema_bf16_kernel(const bf16_bits* __restrict__ p, float* __restrict__ s, int64_t n, float omd) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  const int64_t groups = n >> 3;
  for (int64_t g = tid; g < groups; g += stride) {
    const bf16x8_bits pv = reinterpret_cast<const bf16x8_bits*>(p)[g];
    f32x4* sp = reinterpret_cast<f32x4*>(s) + 2 * g;
    const f32x4 s0 = sp[0], s1 = sp[1];
    sp[0] = ema4(s0, bf2f((bf16_bits)pv[0]), bf2f((bf16_bits)pv[1]), bf2f((bf16_bits)pv[2]), bf2f((bf16_bits)pv[3]), omd);
    sp[1] = ema4(s1, bf2f((bf16_bits)pv[4]), bf2f((bf16_bits)pv[5]), bf2f((bf16_bits)pv[6]), bf2f((bf16_bits)pv[7]), omd);
  }
  const int64_t i = (groups << 3) + tid;   // scalar tail: fewer than 8 elements, the first lanes of the grid
  if (i < n) s[i] = ema1(s[i], bf2f(p[i]), omd);
}

__global__ __launch_bounds__(256) void ema_f32_kernel(const float* __restrict__ p, float* __restrict__ s, int64_t n, float omd) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  const int64_t groups = n >> 2;
  for (int64_t g = tid; g < groups; g += stride) {
    const f32x4 pv = reinterpret_cast<const f32x4*>(p)[g];
    f32x4* sp = reinterpret_cast<f32x4*>(s) + g;
    *sp = ema4(*sp, pv[0], pv[1], pv[2], pv[3], omd);
  }
  const int64_t i = (groups << 2) + tid;
  if (i < n) s[i] = ema1(s[i], p[i], omd);
}
}  // namespace

extern "C" int ovla_ema_update(const ovla_ema_update_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->param && a->shadow, "ovla_ema_update: null pointer");
  OVLA_REQUIRE(a->n >= 0, "ovla_ema_update: n = %lld", (long long)a->n);
  OVLA_REQUIRE(aligned16(a->param) && aligned16(a->shadow), "ovla_ema_update: param and shadow must be 16-byte aligned");
  OVLA_REQUIRE(a->one_minus_decay >= 0.0f && a->one_minus_decay <= 1.0f, "ovla_ema_update: one_minus_decay = %g is outside [0, 1]",
               (double)a->one_minus_decay);   // false for NaN as well
  if (a->n == 0) return OVLA_OK;
  const int per_lane = a->is_bf16 ? 8 : 4;
  int64_t blocks = (a->n + 256 * per_lane - 1) / (256 * per_lane);   // >= 1, so the tail's lanes (< per_lane of them) always exist
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  if (a->is_bf16)
    hipLaunchKernelGGL(ema_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const bf16_bits*)a->param, a->shadow, a->n, a->one_minus_decay);
  else
    hipLaunchKernelGGL(ema_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const float*)a->param, a->shadow, a->n, a->one_minus_decay);
  OVLA_CHECK_LAUNCH("ovla_ema_update");
  return OVLA_OK;
}
