// laplace_policy.hip -- the stochastic side of the continuous L1 head: L1 regression is maximum likelihood for a Laplace distribution of fixed
// scale around the head's prediction, so that distribution is the policy the head already is.  ovla_laplace_sample draws G chunks per row
// around the prediction and reports their log-probabilities; ovla_laplace_pg computes, for given draws, the same log-probabilities and the
// gradient of the clipped policy-gradient surrogate plus the closed-form KL to a reference prediction, with respect to the prediction (the
// `dpred` ovla_head_out_bwd takes).  THE CONTRACT is in ovla.h "Laplace policy on the L1 head"; tests/laplace_policy_reference.py restates it.
// A launch of a few hundred lanes: one lane per (row, draw) for the sampler; one 64-lane workgroup per row for the gradient (lane g forms
// sample g's outputs and its weight into LDS, a barrier, lane d sums over g).  No atomics, no workspace.
// Every operator below is one rounded fp32 operation, as the numpy restatement computes it:
#pragma clang fp contract(off)
#include "common.h"
#include <math.h>

namespace {

constexpr int MAX_ADIM = 16;   // ovla.h: 1 <= adim <= 16, as in head_optim.hip

// the scales as the kernels take them: inv_b = 1.0f / b is the host's IEEE division
struct Scales { float b[MAX_ADIM], inv_b[MAX_ADIM], log_norm[MAX_ADIM]; };

// acc = acc - (|a_d - mu_d| * inv_b_d + log_norm_d) over ascending d: the one body both kernels take the log-probability from
OVLA_DEV float logprob_step(float acc, float a, float mu, float inv_b, float log_norm) {
  const float q = fabsf(a - mu) * inv_b;
  return acc - (q + log_norm);
}

__global__ __launch_bounds__(64) void laplace_sample_kernel(const bf16_bits* __restrict__ pred, float* __restrict__ action, float* __restrict__ logprob,
                                                            const uint32_t* __restrict__ state_dev, const int* __restrict__ row_key, uint32_t seed_lo,
                                                            uint32_t seed_hi, uint32_t call, Scales sc, int rows, int adim, int G) {
  const int64_t o = (int64_t)blockIdx.x * 64 + threadIdx.x;     // draw (r, g) = o / G, o % G
  if (o >= (int64_t)rows * G) return;
  const int64_t r = o / G;
  if (state_dev) { seed_lo = state_dev[0]; seed_hi = state_dev[1]; call = state_dev[2]; }
  const uint32_t key = (uint32_t)(row_key ? row_key[o] : (int)o);
  const bf16_bits* mu_row = pred + r * adim;
  float* a_row = action + o * adim;
  float acc = 0.0f;
  uint32_t w[4];
#pragma unroll
  for (int d = 0; d < MAX_ADIM; ++d) {
    if (d < adim) {
      if ((d & 3) == 0) philox4x32_10((uint32_t)d >> 2, key, 4u, call, seed_lo, seed_hi, w);
      const float u = (float)(2u * (w[d & 3] >> 9) + 1u) * 0x1p-24f;
      const float x = u - 0.5f;                                  // exact, never 0
      const float t = 1.0f - 2.0f * fabsf(x);                    // exact, in [2^-23, 1 - 2^-23]
      const float e = copysignf(-logf(t), x);
      const float mu = bf2f(mu_row[d]);
      const float a = mu + sc.b[d] * e;
      a_row[d] = a;
      acc = logprob_step(acc, a, mu, sc.inv_b[d], sc.log_norm[d]);   // from the STORED a: what ovla_laplace_pg recomputes
    }
  }
  logprob[o] = acc;
}

__global__ __launch_bounds__(64) void laplace_pg_kernel(const bf16_bits* __restrict__ pred, const bf16_bits* __restrict__ ref_pred,
                                                        const float* __restrict__ actions, const float* __restrict__ advantage,
                                                        const float* __restrict__ old_logprob, float* __restrict__ logprob_out,
                                                        float* __restrict__ ratio_out, int* __restrict__ clipped_out, float* __restrict__ kl_out,
                                                        bf16_bits* __restrict__ dpred, Scales sc, float clip_lo, float clip_hi, float grad_scale,
                                                        float kl_coef, float kl_scale, int adim, int G) {
  __shared__ float g_c[OVLA_PG_GROUP_MAX];
  __shared__ float kl_d[MAX_ADIM];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const bf16_bits* mu_row = pred + row * adim;
  const float* a_row = actions + row * G * adim;
  if (tid < G) {
    const int64_t o = row * G + tid;
    const float* a = a_row + (int64_t)tid * adim;
    float lp = 0.0f;
#pragma unroll
    for (int d = 0; d < MAX_ADIM; ++d)
      if (d < adim) lp = logprob_step(lp, a[d], bf2f(mu_row[d]), sc.inv_b[d], sc.log_norm[d]);
    const float adv = advantage[o];
    const float ratio = old_logprob ? expf(lp - old_logprob[o]) : 1.0f;
    const bool gated = (adv >= 0.0f && ratio > clip_hi) || (adv < 0.0f && ratio < clip_lo);
    logprob_out[o] = lp;
    ratio_out[o] = ratio;
    clipped_out[o] = gated ? 1 : 0;
    g_c[tid] = (gated || adv == 0.0f) ? 0.0f : (adv * ratio) * grad_scale;   // set, never multiplied through: a padding draw may hold NaN
  }
  // the scale of lane d: one select chain over the by-value arrays (no dynamic indexing of kernel arguments)
  float inv_b = 0.0f;
#pragma unroll
  for (int d = 0; d < MAX_ADIM; ++d)
    if (d == tid) inv_b = sc.inv_b[d];
  float mu = 0.0f, x = 0.0f, sgn_delta = 0.0f;
  if (tid < adim) {
    mu = bf2f(mu_row[tid]);
    if (ref_pred) {
      const float ref = bf2f(ref_pred[row * adim + tid]);
      const float delta = mu - ref;
      const float q = fabsf(delta) * inv_b;
      x = -expm1f(-q);
      kl_d[tid] = q - x;
      sgn_delta = mu > ref ? 1.0f : (mu < ref ? -1.0f : 0.0f);
    }
  }
  __syncthreads();
  if (ref_pred && tid == 0) {
    float s = kl_d[0];
    for (int d = 1; d < adim; ++d) s = s + kl_d[d];
    kl_out[row] = s;
  }
  if (!dpred || tid >= adim) return;
  float acc = 0.0f;
  bool first = true;
  for (int g = 0; g < G; ++g) {
    const float c = g_c[g];
    if (c != 0.0f) {                                            // a skipped sample's action is not even read
      const float a = a_row[(int64_t)g * adim + tid];
      const float s = mu > a ? 1.0f : (mu < a ? -1.0f : 0.0f);
      const float t = (s * inv_b) * c;
      acc = first ? t : acc + t;
      first = false;
    }
  }
  if (ref_pred) acc = acc + ((kl_coef * x) * kl_scale) * (sgn_delta * inv_b);
  dpred[row * adim + tid] = f2bf(acc);
}

bool scales_ok(const float* b, int adim) {
  for (int d = 0; d < adim; ++d)
    if (!(b[d] > 0.0f && b[d] < INFINITY)) return false;
  return true;
}

Scales make_scales(const float* b, const float* log_norm, int adim) {
  Scales sc;
  for (int d = 0; d < MAX_ADIM; ++d) {
    const bool in = d < adim;
    sc.b[d] = in ? b[d] : 1.0f;
    sc.inv_b[d] = in ? 1.0f / b[d] : 1.0f;
    sc.log_norm[d] = in ? log_norm[d] : 0.0f;
  }
  return sc;
}
}  // namespace

extern "C" int ovla_laplace_sample(const ovla_laplace_sample_args* a, void* stream_) {
  OVLA_REQUIRE(a && a->pred && a->action && a->logprob, "ovla_laplace_sample: null pointer");
  OVLA_REQUIRE(a->rows > 0 && a->adim >= 1 && a->adim <= MAX_ADIM, "ovla_laplace_sample: rows=%d adim=%d (adim 1 .. %d)", a->rows, a->adim, MAX_ADIM);
  OVLA_REQUIRE(a->G >= 1 && a->G <= OVLA_PG_GROUP_MAX && (int64_t)a->rows * a->G <= 0x7fffffff, "ovla_laplace_sample: G = %d (1 .. %d), rows = %d", a->G,
               OVLA_PG_GROUP_MAX, a->rows);
  OVLA_REQUIRE(scales_ok(a->scale, a->adim), "ovla_laplace_sample: a scale is not positive and finite");
  const int64_t n = (int64_t)a->rows * a->G;
  hipLaunchKernelGGL(laplace_sample_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream_, (const bf16_bits*)a->pred, a->action, a->logprob,
                     a->state_dev, a->row_key, a->seed_lo, a->seed_hi, a->call, make_scales(a->scale, a->log_norm, a->adim), a->rows, a->adim, a->G);
  OVLA_CHECK_LAUNCH("ovla_laplace_sample");
  return OVLA_OK;
}

extern "C" int ovla_laplace_pg(const ovla_laplace_pg_args* a, void* stream_) {
  OVLA_REQUIRE(a && a->pred && a->actions && a->advantage && a->logprob && a->ratio && a->clipped, "ovla_laplace_pg: null pointer");
  OVLA_REQUIRE(a->rows > 0 && a->adim >= 1 && a->adim <= MAX_ADIM, "ovla_laplace_pg: rows=%d adim=%d (adim 1 .. %d)", a->rows, a->adim, MAX_ADIM);
  OVLA_REQUIRE(a->G >= 1 && a->G <= OVLA_PG_GROUP_MAX, "ovla_laplace_pg: G = %d (1 .. %d)", a->G, OVLA_PG_GROUP_MAX);
  OVLA_REQUIRE(scales_ok(a->scale, a->adim), "ovla_laplace_pg: a scale is not positive and finite");
  OVLA_REQUIRE(a->clip_lo <= a->clip_hi, "ovla_laplace_pg: clip_lo = %g > clip_hi = %g (or a NaN bound)", (double)a->clip_lo, (double)a->clip_hi);
  OVLA_REQUIRE(a->kl_coef >= 0.0f, "ovla_laplace_pg: kl_coef = %g (must not be negative or NaN)", (double)a->kl_coef);
  OVLA_REQUIRE((a->ref_pred != nullptr) == (a->kl != nullptr), "ovla_laplace_pg: ref_pred and kl come together (ref_pred %s, kl %s)",
               a->ref_pred ? "given" : "null", a->kl ? "given" : "null");
  hipLaunchKernelGGL(laplace_pg_kernel, dim3((unsigned)a->rows), dim3(64), 0, (hipStream_t)stream_, (const bf16_bits*)a->pred, (const bf16_bits*)a->ref_pred,
                     a->actions, a->advantage, a->old_logprob, a->logprob, a->ratio, a->clipped, a->kl, (bf16_bits*)a->dpred,
                     make_scales(a->scale, a->log_norm, a->adim), a->clip_lo, a->clip_hi, a->grad_scale, a->kl_coef, a->kl_scale, a->adim, a->G);
  OVLA_CHECK_LAUNCH("ovla_laplace_pg");
  return OVLA_OK;
}
