// ddim.hip -- the DDIM sampler's per-step host work as two small kernels, so that a sampling step has no host-dependent argument and the
// whole loop can be replayed from a captured graph (engine.DiffusionGraph).  The step index lives in device memory: both kernels read it,
// ovla_ddim_step advances it.
#include "common.h"

namespace {

// Top of a step: row k of the timestep-embedding table into every observation's timestep slot, bf16(sample) as the noisy actions.
// One workgroup per observation; the n sample elements are dealt over the workgroups.
__global__ __launch_bounds__(256) void ddim_prepare_kernel(const int32_t* __restrict__ step, const bf16_bits* __restrict__ temb_table,
                                                           bf16_bits* __restrict__ temb, const float* __restrict__ sample,
                                                           bf16_bits* __restrict__ noisy, int n_steps, int D, int n) {
  const int k = *step;
  if (k < 0 || k >= n_steps) return;
  const bf16_bits* row = temb_table + (int64_t)k * D;
  bf16_bits* dst = temb + (int64_t)blockIdx.x * D;
  for (int j = threadIdx.x; j < D; j += blockDim.x) dst[j] = row[j];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) noisy[i] = f2bf(sample[i]);
}

// sample <- bf16(DDIMScheduler.step(eps, t_k, sample)) as fp32 (diffusion.py: epsilon prediction, clip_sample, eta = 0), every operation
// rounded on its own in torch's order.  coef row k = ((1 - a_t)^1/2, a_t^1/2, a_prev^1/2, (1 - a_prev)^1/2).  ONE workgroup: every thread has
// read the step index before the barrier behind which thread 0 advances it.
__global__ __launch_bounds__(256) void ddim_step_kernel(float* __restrict__ sample, const bf16_bits* __restrict__ eps, const float* __restrict__ coef,
                                                        int32_t* step, int n_steps, int n) {
#pragma clang fp contract(off)  // torch's separate mul / sub / div / add: no fused multiply-adds the reference lacks
  const int k = *step;
  if (k < 0 || k >= n_steps) return;   // (uniform over the workgroup: nobody reaches the barrier)
  const float c0 = coef[4 * k + 0], c1 = coef[4 * k + 1], c2 = coef[4 * k + 2], c3 = coef[4 * k + 3];
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float s = sample[i], e = bf2f(eps[i]);
    float x0 = (s - c0 * e) / c1;
    x0 = x0 < -1.0f ? -1.0f : (x0 > 1.0f ? 1.0f : x0);   // torch.clamp: NaN stays NaN
    const float e2 = (s - c1 * x0) / c0;
    sample[i] = bfround(c2 * x0 + c3 * e2);
  }
  __syncthreads();
  if (threadIdx.x == 0) *step = k + 1;
}
}  // namespace

extern "C" int ovla_ddim_prepare(const ovla_ddim_prepare_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->step && a->temb_table && a->temb && a->sample && a->noisy, "ovla_ddim_prepare: null pointer");
  OVLA_REQUIRE(a->n_steps > 0 && a->B > 0 && a->D > 0 && a->n > 0, "ovla_ddim_prepare: n_steps=%d B=%d D=%d n=%d", a->n_steps, a->B, a->D, a->n);
  hipLaunchKernelGGL(ddim_prepare_kernel, dim3(a->B), dim3(256), 0, stream, a->step, (const bf16_bits*)a->temb_table, (bf16_bits*)a->temb, a->sample,
                     (bf16_bits*)a->noisy, a->n_steps, a->D, a->n);
  OVLA_CHECK_LAUNCH("ovla_ddim_prepare");
  return OVLA_OK;
}

extern "C" int ovla_ddim_step(const ovla_ddim_step_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->sample && a->eps && a->coef && a->step, "ovla_ddim_step: null pointer");
  OVLA_REQUIRE(a->n_steps > 0 && a->n > 0, "ovla_ddim_step: n_steps=%d n=%d", a->n_steps, a->n);
  hipLaunchKernelGGL(ddim_step_kernel, dim3(1), dim3(256), 0, stream, a->sample, (const bf16_bits*)a->eps, a->coef, a->step, a->n_steps, a->n);
  OVLA_CHECK_LAUNCH("ovla_ddim_step");
  return OVLA_OK;
}
