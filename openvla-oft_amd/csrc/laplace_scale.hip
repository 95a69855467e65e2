// laplace_scale.hip -- the Laplace policy of laplace_policy.hip with a LEARNED scale: a scale head predicts s = log b per chunk step and action
// dimension beside the L1 head's prediction.  ovla_laplace_sample_rows draws G chunks per row at the row's own widths;
// ovla_laplace_pg_rows computes, for given draws, the log-probabilities and the gradient of the clipped surrogate, of the closed-form KL to a
// reference of its own scale and of the entropy bonus, with respect to BOTH the prediction (`dpred`) and the log-scale (`dlog_scale`): each
// is what ovla_head_out_bwd takes.  At G = 1 without ratio, reference and entropy it is the gradient of the Laplace negative log-likelihood,
// so the maximum-likelihood fit of the scale needs no kernel of its own.
// THE CONTRACT is in ovla.h "Laplace policy with a learned scale"; tests/laplace_scale_reference.py restates it.  Launch shapes as in
// laplace_policy.hip: one lane per (row, draw) for the sampler; one 64-lane workgroup per row for the gradient (lane d forms the row's scales
// into LDS, a barrier, lane g forms sample g's outputs and its weight into LDS, a barrier, lane d sums over g).  No atomics, no workspace.
// Every operator below is one rounded fp32 operation, as the numpy restatement computes it:
#pragma clang fp contract(off)
#include "common.h"
#include <math.h>

namespace {

constexpr int MAX_ADIM = 16;            // ovla.h: 1 <= adim <= 16
constexpr float LN2F = 0x1.62e43p-1f;   // float32(ln 2)

// the scale of one element as both kernels take it from the scale head's raw output
struct ElemScale { float s_c, b, inv_b, log_norm; bool inside; };

OVLA_DEV ElemScale elem_scale(float s, float s_lo, float s_hi) {
  ElemScale e;
  e.s_c = fminf(fmaxf(s, s_lo), s_hi);     // a NaN s acts as s_lo
  e.inside = (s >= s_lo && s <= s_hi);     // false for NaN
  e.b = expf(e.s_c);
  e.inv_b = 1.0f / e.b;
  e.log_norm = e.s_c + LN2F;
  return e;
}

// laplace_policy.hip's body: acc = acc - (|a_d - mu_d| * inv_b_d + log_norm_d) over ascending d
OVLA_DEV float logprob_step(float acc, float a, float mu, float inv_b, float log_norm) {
  const float q = fabsf(a - mu) * inv_b;
  return acc - (q + log_norm);
}

__global__ __launch_bounds__(64) void laplace_sample_rows_kernel(const bf16_bits* __restrict__ pred, const bf16_bits* __restrict__ log_scale,
                                                                 float* __restrict__ action, float* __restrict__ logprob, float* __restrict__ entropy,
                                                                 const uint32_t* __restrict__ state_dev, const int* __restrict__ row_key, uint32_t seed_lo,
                                                                 uint32_t seed_hi, uint32_t call, float s_lo, float s_hi, int rows, int adim, int G) {
  const int64_t o = (int64_t)blockIdx.x * 64 + threadIdx.x;     // draw (r, g) = o / G, o % G
  if (o >= (int64_t)rows * G) return;
  const int64_t r = o / G;
  if (state_dev) { seed_lo = state_dev[0]; seed_hi = state_dev[1]; call = state_dev[2]; }
  const uint32_t key = (uint32_t)(row_key ? row_key[o] : (int)o);
  const bf16_bits* mu_row = pred + r * adim;
  const bf16_bits* s_row = log_scale + r * adim;
  float* a_row = action + o * adim;
  float acc = 0.0f, ent = 0.0f;
  uint32_t w[4];
#pragma unroll
  for (int d = 0; d < MAX_ADIM; ++d) {
    if (d < adim) {
      if ((d & 3) == 0) philox4x32_10((uint32_t)d >> 2, key, 4u, call, seed_lo, seed_hi, w);
      const float u = (float)(2u * (w[d & 3] >> 9) + 1u) * 0x1p-24f;
      const float x = u - 0.5f;                                  // exact, never 0
      const float t = 1.0f - 2.0f * fabsf(x);                    // exact, in [2^-23, 1 - 2^-23]
      const float e = copysignf(-logf(t), x);
      const ElemScale sc = elem_scale(bf2f(s_row[d]), s_lo, s_hi);
      const float mu = bf2f(mu_row[d]);
      const float a = mu + sc.b * e;
      a_row[d] = a;
      acc = logprob_step(acc, a, mu, sc.inv_b, sc.log_norm);     // from the STORED a: what ovla_laplace_pg_rows recomputes
      const float h = 1.0f + sc.log_norm;
      ent = d == 0 ? h : ent + h;
    }
  }
  logprob[o] = acc;
  if (entropy && o == r * G) entropy[r] = ent;
}

__global__ __launch_bounds__(64) void laplace_pg_rows_kernel(const bf16_bits* __restrict__ pred, const bf16_bits* __restrict__ log_scale,
                                                             const bf16_bits* __restrict__ ref_pred, const bf16_bits* __restrict__ ref_log_scale,
                                                             const float* __restrict__ actions, const float* __restrict__ advantage,
                                                             const float* __restrict__ old_logprob, float* __restrict__ logprob_out,
                                                             float* __restrict__ ratio_out, int* __restrict__ clipped_out, float* __restrict__ kl_out,
                                                             float* __restrict__ entropy_out, bf16_bits* __restrict__ dpred,
                                                             bf16_bits* __restrict__ dlog_scale, float s_lo, float s_hi, float clip_lo, float clip_hi,
                                                             float grad_scale, float kl_coef, float kl_scale, float entropy_coef, float ent_scale,
                                                             int adim, int G) {
  __shared__ float g_c[OVLA_PG_GROUP_MAX];
  __shared__ float sh_inv_b[MAX_ADIM], sh_log_norm[MAX_ADIM], kl_d[MAX_ADIM];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const bf16_bits* mu_row = pred + row * adim;
  const float* a_row = actions + row * G * adim;
  float mu = 0.0f;
  ElemScale sc = {0.0f, 1.0f, 1.0f, 0.0f, false};
  if (tid < adim) {
    mu = bf2f(mu_row[tid]);
    sc = elem_scale(bf2f(log_scale[row * adim + tid]), s_lo, s_hi);
    sh_inv_b[tid] = sc.inv_b;
    sh_log_norm[tid] = sc.log_norm;
  }
  __syncthreads();
  if (tid < G) {
    const int64_t o = row * G + tid;
    const float* a = a_row + (int64_t)tid * adim;
    float lp = 0.0f;
    for (int d = 0; d < adim; ++d) lp = logprob_step(lp, a[d], bf2f(mu_row[d]), sh_inv_b[d], sh_log_norm[d]);
    const float adv = advantage[o];
    const float ratio = old_logprob ? expf(lp - old_logprob[o]) : 1.0f;
    const bool gated = (adv >= 0.0f && ratio > clip_hi) || (adv < 0.0f && ratio < clip_lo);
    logprob_out[o] = lp;
    ratio_out[o] = ratio;
    clipped_out[o] = gated ? 1 : 0;
    g_c[tid] = (gated || adv == 0.0f) ? 0.0f : (adv * ratio) * grad_scale;   // set, never multiplied through: a padding draw may hold NaN
  }
  float q_ref = 0.0f, x = 0.0f, rho = 1.0f, sgn_delta = 0.0f;
  if (ref_pred && tid < adim) {
    const float ref = bf2f(ref_pred[row * adim + tid]);
    const float s_rc = fminf(fmaxf(bf2f(ref_log_scale[row * adim + tid]), s_lo), s_hi);
    const float u = sc.s_c - s_rc;
    const float delta = mu - ref;
    q_ref = fabsf(delta) * sc.inv_b;
    x = -expm1f(-q_ref);
    rho = expf(u);
    kl_d[tid] = (expm1f(u) - u) + rho * (q_ref - x);
    sgn_delta = mu > ref ? 1.0f : (mu < ref ? -1.0f : 0.0f);
  }
  __syncthreads();
  if (tid == 0) {
    if (ref_pred) {
      float s = kl_d[0];
      for (int d = 1; d < adim; ++d) s = s + kl_d[d];
      kl_out[row] = s;
    }
    float h = 1.0f + sh_log_norm[0];
    for (int d = 1; d < adim; ++d) h = h + (1.0f + sh_log_norm[d]);
    entropy_out[row] = h;
  }
  if ((!dpred && !dlog_scale) || tid >= adim) return;
  float acc_mu = 0.0f, acc_s = 0.0f;
  bool first = true;
  for (int g = 0; g < G; ++g) {
    const float c = g_c[g];
    if (c != 0.0f) {                                            // a skipped sample's action is not even read
      const float a = a_row[(int64_t)g * adim + tid];
      const float sg = mu > a ? 1.0f : (mu < a ? -1.0f : 0.0f);
      const float t_mu = (sg * sc.inv_b) * c;
      const float q = fabsf(a - mu) * sc.inv_b;
      const float t_s = (1.0f - q) * c;
      acc_mu = first ? t_mu : acc_mu + t_mu;
      acc_s = first ? t_s : acc_s + t_s;
      first = false;
    }
  }
  if (ref_pred) {
    acc_mu = acc_mu + (((kl_coef * x) * kl_scale) * (sgn_delta * sc.inv_b)) * rho;
    acc_s = acc_s + (kl_coef * kl_scale) * (((rho * (1.0f - x)) * (1.0f + q_ref)) - 1.0f);
  }
  if (entropy_coef != 0.0f) acc_s = acc_s - (entropy_coef * ent_scale);
  if (dpred) dpred[row * adim + tid] = f2bf(acc_mu);
  if (dlog_scale) dlog_scale[row * adim + tid] = sc.inside ? f2bf(acc_s) : (bf16_bits)0;
}

bool bounds_ok(float s_lo, float s_hi) { return s_lo <= s_hi && s_lo > -INFINITY && s_hi < INFINITY; }   // (a NaN fails the first comparison)
}  // namespace

extern "C" int ovla_laplace_sample_rows(const ovla_laplace_sample_rows_args* a, void* stream_) {
  OVLA_REQUIRE(a && a->pred && a->log_scale && a->action && a->logprob, "ovla_laplace_sample_rows: null pointer");
  OVLA_REQUIRE(a->rows > 0 && a->adim >= 1 && a->adim <= MAX_ADIM, "ovla_laplace_sample_rows: rows=%d adim=%d (adim 1 .. %d)", a->rows, a->adim, MAX_ADIM);
  OVLA_REQUIRE(a->G >= 1 && a->G <= OVLA_PG_GROUP_MAX && (int64_t)a->rows * a->G <= 0x7fffffff, "ovla_laplace_sample_rows: G = %d (1 .. %d), rows = %d",
               a->G, OVLA_PG_GROUP_MAX, a->rows);
  OVLA_REQUIRE(bounds_ok(a->s_lo, a->s_hi), "ovla_laplace_sample_rows: log-scale bounds [%g, %g] (finite, s_lo <= s_hi)", (double)a->s_lo, (double)a->s_hi);
  const int64_t n = (int64_t)a->rows * a->G;
  hipLaunchKernelGGL(laplace_sample_rows_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream_, (const bf16_bits*)a->pred,
                     (const bf16_bits*)a->log_scale, a->action, a->logprob, a->entropy, a->state_dev, a->row_key, a->seed_lo, a->seed_hi, a->call, a->s_lo,
                     a->s_hi, a->rows, a->adim, a->G);
  OVLA_CHECK_LAUNCH("ovla_laplace_sample_rows");
  return OVLA_OK;
}

extern "C" int ovla_laplace_pg_rows(const ovla_laplace_pg_rows_args* a, void* stream_) {
  OVLA_REQUIRE(a && a->pred && a->log_scale && a->actions && a->advantage && a->logprob && a->ratio && a->clipped && a->entropy,
               "ovla_laplace_pg_rows: null pointer");
  OVLA_REQUIRE(a->rows > 0 && a->adim >= 1 && a->adim <= MAX_ADIM, "ovla_laplace_pg_rows: rows=%d adim=%d (adim 1 .. %d)", a->rows, a->adim, MAX_ADIM);
  OVLA_REQUIRE(a->G >= 1 && a->G <= OVLA_PG_GROUP_MAX, "ovla_laplace_pg_rows: G = %d (1 .. %d)", a->G, OVLA_PG_GROUP_MAX);
  OVLA_REQUIRE(bounds_ok(a->s_lo, a->s_hi), "ovla_laplace_pg_rows: log-scale bounds [%g, %g] (finite, s_lo <= s_hi)", (double)a->s_lo, (double)a->s_hi);
  OVLA_REQUIRE(a->clip_lo <= a->clip_hi, "ovla_laplace_pg_rows: clip_lo = %g > clip_hi = %g (or a NaN bound)", (double)a->clip_lo, (double)a->clip_hi);
  OVLA_REQUIRE(a->kl_coef >= 0.0f, "ovla_laplace_pg_rows: kl_coef = %g (must not be negative or NaN)", (double)a->kl_coef);
  OVLA_REQUIRE(a->entropy_coef >= 0.0f, "ovla_laplace_pg_rows: entropy_coef = %g (must not be negative or NaN)", (double)a->entropy_coef);
  OVLA_REQUIRE((a->ref_pred != nullptr) == (a->kl != nullptr) && (a->ref_pred != nullptr) == (a->ref_log_scale != nullptr),
               "ovla_laplace_pg_rows: ref_pred, ref_log_scale and kl come together (ref_pred %s, ref_log_scale %s, kl %s)", a->ref_pred ? "given" : "null",
               a->ref_log_scale ? "given" : "null", a->kl ? "given" : "null");
  hipLaunchKernelGGL(laplace_pg_rows_kernel, dim3((unsigned)a->rows), dim3(64), 0, (hipStream_t)stream_, (const bf16_bits*)a->pred,
                     (const bf16_bits*)a->log_scale, (const bf16_bits*)a->ref_pred, (const bf16_bits*)a->ref_log_scale, a->actions, a->advantage,
                     a->old_logprob, a->logprob, a->ratio, a->clipped, a->kl, a->entropy, (bf16_bits*)a->dpred, (bf16_bits*)a->dlog_scale, a->s_lo, a->s_hi,
                     a->clip_lo, a->clip_hi, a->grad_scale, a->kl_coef, a->kl_scale, a->entropy_coef, a->ent_scale, a->adim, a->G);
  OVLA_CHECK_LAUNCH("ovla_laplace_pg_rows");
  return OVLA_OK;
}
