// laplace_dpo.hip -- direct preference optimisation on the Laplace policy of the L1 head: a pair of chunks per observation, the chosen and the
// rejected one, and a reference prediction.  The loss of an observation is a function of ONE scalar, the margin between the two chunks' summed
// log-ratios to the reference, and its gradient with respect to the head's prediction is the group policy gradient of the pair with the
// advantages +k and -k, k out of that margin.  ovla_laplace_dpo reduces the margin over the observation's chunk steps, forms k and applies it
// in the same launch: `dpred` (and `dlog_scale` under a learned scale) are what ovla_head_out_bwd takes, so a preference step costs the one
// training forward and the one backward of the L1 step.
// THE CONTRACT is in ovla.h "Preference optimisation on the Laplace policy"; tests/laplace_dpo_reference.py restates it.  One 64-lane workgroup
// per observation: lane c forms chunk step c's four log-probabilities and its two log-ratios into LDS, a barrier, every lane sums them in
// ascending c (the same bits in every lane), then lane e, e + 64, ... forms element e = c * adim + d of the gradient.  No atomics, no workspace.
// Every operator below is one rounded fp32 operation, as the numpy restatement computes it:
#pragma clang fp contract(off)
#include "common.h"
#include <math.h>

namespace {

constexpr int MAX_ADIM = 16;            // ovla.h: 1 <= adim <= 16
constexpr float LN2F = 0x1.62e43p-1f;   // float32(ln 2)

// the fixed scales as the kernel takes them (laplace_policy.hip's): inv_b = 1.0f / b is the host's IEEE division
struct Scales { float inv_b[MAX_ADIM], log_norm[MAX_ADIM]; };

// laplace_scale.hip's element rules
struct ElemScale { float inv_b, log_norm; bool inside; };

OVLA_DEV ElemScale elem_scale(float s, float s_lo, float s_hi) {
  ElemScale e;
  const float s_c = fminf(fmaxf(s, s_lo), s_hi);   // a NaN s acts as s_lo
  e.inside = (s >= s_lo && s <= s_hi);             // false for NaN
  const float b = expf(s_c);
  e.inv_b = 1.0f / b;
  e.log_norm = s_c + LN2F;
  return e;
}

// laplace_policy.hip's body: acc = acc - (|a_d - mu_d| * inv_b_d + log_norm_d) over ascending d
OVLA_DEV float logprob_step(float acc, float a, float mu, float inv_b, float log_norm) {
  const float q = fabsf(a - mu) * inv_b;
  return acc - (q + log_norm);
}

struct DpoScalars { float s_lo, s_hi, beta, eps, grad_scale, nll_coef, nll_scale; int loss_type, chunk, adim; };

template <bool ROWS>
__global__ __launch_bounds__(64) void laplace_dpo_kernel(const bf16_bits* __restrict__ pred, const bf16_bits* __restrict__ ref_pred,
                                                         const bf16_bits* __restrict__ log_scale, const bf16_bits* __restrict__ ref_log_scale,
                                                         const float* __restrict__ chosen, const float* __restrict__ rejected,
                                                         const float* __restrict__ weight, float* __restrict__ logprob_out,
                                                         float* __restrict__ ref_logprob_out, float* __restrict__ h_out, float* __restrict__ margin_out,
                                                         float* __restrict__ loss_out, float* __restrict__ coef_out, bf16_bits* __restrict__ dpred,
                                                         bf16_bits* __restrict__ dlog_scale, Scales sc, DpoScalars p) {
  __shared__ float sh_inv_b[MAX_ADIM], sh_log_norm[MAX_ADIM];
  __shared__ float sh_dw[OVLA_DPO_CHUNK_MAX], sh_dl[OVLA_DPO_CHUNK_MAX];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int chunk = p.chunk, adim = p.adim, n_elem = chunk * adim;   // <= 64 * 16
  const int64_t row0 = b * chunk, elem0 = row0 * adim;
  const float w = weight ? weight[b] : 1.0f;
  if (w == 0.0f) {                                               // the whole workgroup: no chunk is read, every output is SET to +0
    if (tid < chunk) {
      if (logprob_out) { logprob_out[(row0 + tid) * 2] = 0.0f; logprob_out[(row0 + tid) * 2 + 1] = 0.0f; }
      if (ref_logprob_out) { ref_logprob_out[(row0 + tid) * 2] = 0.0f; ref_logprob_out[(row0 + tid) * 2 + 1] = 0.0f; }
    }
    if (tid == 0) { h_out[b * 2] = 0.0f; h_out[b * 2 + 1] = 0.0f; margin_out[b] = 0.0f; loss_out[b] = 0.0f; coef_out[b] = 0.0f; }
    for (int e = tid; e < n_elem; e += 64) {
      if (dpred) dpred[elem0 + e] = (bf16_bits)0;
      if (dlog_scale) dlog_scale[elem0 + e] = (bf16_bits)0;
    }
    return;
  }
  if (!ROWS) {                                                   // lane d's scale: one select chain over the by-value arrays
    float inv_b = 1.0f, log_norm = 0.0f;
#pragma unroll
    for (int d = 0; d < MAX_ADIM; ++d)
      if (d == tid) { inv_b = sc.inv_b[d]; log_norm = sc.log_norm[d]; }
    if (tid < MAX_ADIM) { sh_inv_b[tid] = inv_b; sh_log_norm[tid] = log_norm; }
    __syncthreads();
  }
  if (tid < chunk) {
    const int64_t row = row0 + tid;
    const bf16_bits* mu_row = pred + row * adim;
    const bf16_bits* ref_row = ref_pred + row * adim;
    const float* aw = chosen + row * adim;
    const float* al = rejected + row * adim;
    float lp_w = 0.0f, lp_l = 0.0f, rlp_w = 0.0f, rlp_l = 0.0f;
    for (int d = 0; d < adim; ++d) {
      float inv_b, log_norm, r_inv_b, r_log_norm;
      if (ROWS) {
        const ElemScale el = elem_scale(bf2f(log_scale[row * adim + d]), p.s_lo, p.s_hi);
        const ElemScale er = elem_scale(bf2f(ref_log_scale[row * adim + d]), p.s_lo, p.s_hi);
        inv_b = el.inv_b, log_norm = el.log_norm, r_inv_b = er.inv_b, r_log_norm = er.log_norm;
      } else {
        inv_b = r_inv_b = sh_inv_b[d];
        log_norm = r_log_norm = sh_log_norm[d];
      }
      const float mu = bf2f(mu_row[d]), ref = bf2f(ref_row[d]), a_w = aw[d], a_l = al[d];
      lp_w = logprob_step(lp_w, a_w, mu, inv_b, log_norm);
      lp_l = logprob_step(lp_l, a_l, mu, inv_b, log_norm);
      rlp_w = logprob_step(rlp_w, a_w, ref, r_inv_b, r_log_norm);
      rlp_l = logprob_step(rlp_l, a_l, ref, r_inv_b, r_log_norm);
    }
    if (logprob_out) { logprob_out[row * 2] = lp_w; logprob_out[row * 2 + 1] = lp_l; }
    if (ref_logprob_out) { ref_logprob_out[row * 2] = rlp_w; ref_logprob_out[row * 2 + 1] = rlp_l; }
    sh_dw[tid] = lp_w - rlp_w;
    sh_dl[tid] = lp_l - rlp_l;
  }
  __syncthreads();
  float h_w = sh_dw[0], h_l = sh_dl[0];                          // every lane: the same sums in the same order
  for (int c = 1; c < chunk; ++c) {
    h_w = h_w + sh_dw[c];
    h_l = h_l + sh_dl[c];
  }
  const float m = h_w - h_l;
  float loss, k;
  if (p.loss_type == 0) {
    const float z = p.beta * m;
    const float az = fabsf(z);
    const float e = expf(-az);                                   // in (0, 1]: nothing overflows at any |z|
    const float den = 1.0f + e;
    const float l1p = logf(den);                                 // log(1 + e^-|z|)
    const float s_big = 1.0f / den, s_small = e / den;           // sigma(|z|), sigma(-|z|)
    const float sp_neg = (z < 0.0f ? az : 0.0f) + l1p;           // softplus(-z)
    const float sp_pos = (z > 0.0f ? az : 0.0f) + l1p;           // softplus(z)
    const float sig_neg = z >= 0.0f ? s_small : s_big;           // sigma(-z)
    const float sig_pos = z >= 0.0f ? s_big : s_small;           // sigma(z)
    const float one_m = 1.0f - p.eps;
    loss = (one_m * sp_neg) + (p.eps * sp_pos);
    k = ((one_m * sig_neg) - (p.eps * sig_pos)) * p.beta;
  } else {
    const float tau = 1.0f / (2.0f * p.beta);
    const float dm = m - tau;
    loss = dm * dm;
    k = -2.0f * dm;
  }
  const float coef = (k * w) * p.grad_scale;
  if (tid == 0) { h_out[b * 2] = h_w; h_out[b * 2 + 1] = h_l; margin_out[b] = m; loss_out[b] = loss; coef_out[b] = coef; }
  if (!dpred && !dlog_scale) return;
  // the pair as a group of two: g = 0 the chosen chunk with c_0, g = 1 the rejected one with c_1
  const float c0 = p.nll_coef > 0.0f ? coef + ((p.nll_coef * w) * p.nll_scale) : coef;
  const float c1 = -coef;
  for (int e = tid; e < n_elem; e += 64) {
    const int64_t i = elem0 + e;
    const float mu = bf2f(pred[i]);
    float inv_b;
    bool inside = true;
    if (ROWS) {
      const ElemScale el = elem_scale(bf2f(log_scale[i]), p.s_lo, p.s_hi);
      inv_b = el.inv_b, inside = el.inside;
    } else {
      inv_b = sh_inv_b[e % adim];
    }
    float acc_mu = 0.0f, acc_s = 0.0f;
    bool first = true;
    if (c0 != 0.0f) {                                            // a skipped sample's chunk is not even read
      const float a = chosen[i];
      const float sg = mu > a ? 1.0f : (mu < a ? -1.0f : 0.0f);
      const float q = fabsf(a - mu) * inv_b;
      acc_mu = (sg * inv_b) * c0;
      acc_s = (1.0f - q) * c0;
      first = false;
    }
    if (c1 != 0.0f) {
      const float a = rejected[i];
      const float sg = mu > a ? 1.0f : (mu < a ? -1.0f : 0.0f);
      const float q = fabsf(a - mu) * inv_b;
      const float t_mu = (sg * inv_b) * c1;
      const float t_s = (1.0f - q) * c1;
      acc_mu = first ? t_mu : acc_mu + t_mu;
      acc_s = first ? t_s : acc_s + t_s;
    }
    if (dpred) dpred[i] = f2bf(acc_mu);
    if (dlog_scale) dlog_scale[i] = inside ? f2bf(acc_s) : (bf16_bits)0;
  }
}

bool scales_ok(const float* b, int adim) {
  for (int d = 0; d < adim; ++d)
    if (!(b[d] > 0.0f && b[d] < INFINITY)) return false;
  return true;
}

bool bounds_ok(float s_lo, float s_hi) { return s_lo <= s_hi && s_lo > -INFINITY && s_hi < INFINITY; }   // (a NaN fails the first comparison)
}  // namespace

extern "C" int ovla_laplace_dpo(const ovla_laplace_dpo_args* a, void* stream_) {
  OVLA_REQUIRE(a && a->pred && a->ref_pred && a->chosen && a->rejected && a->h && a->margin && a->loss && a->coef, "ovla_laplace_dpo: null pointer");
  OVLA_REQUIRE(a->B > 0 && a->chunk >= 1 && a->chunk <= OVLA_DPO_CHUNK_MAX && a->adim >= 1 && a->adim <= MAX_ADIM && (int64_t)a->B * a->chunk <= 0x7fffffff,
               "ovla_laplace_dpo: B=%d chunk=%d adim=%d (chunk 1 .. %d, adim 1 .. %d)", a->B, a->chunk, a->adim, OVLA_DPO_CHUNK_MAX, MAX_ADIM);
  OVLA_REQUIRE((a->log_scale != nullptr) == (a->ref_log_scale != nullptr), "ovla_laplace_dpo: log_scale and ref_log_scale come together (log_scale %s, ref_log_scale %s)",
               a->log_scale ? "given" : "null", a->ref_log_scale ? "given" : "null");
  const bool rows = a->log_scale != nullptr;
  if (rows)
    OVLA_REQUIRE(bounds_ok(a->s_lo, a->s_hi), "ovla_laplace_dpo: log-scale bounds [%g, %g] (finite, s_lo <= s_hi)", (double)a->s_lo, (double)a->s_hi);
  else
    OVLA_REQUIRE(scales_ok(a->scale, a->adim), "ovla_laplace_dpo: a scale is not positive and finite");
  OVLA_REQUIRE(a->beta >= 0.0f && a->beta < INFINITY, "ovla_laplace_dpo: beta = %g (must be finite and not negative)", (double)a->beta);
  OVLA_REQUIRE(a->nll_coef >= 0.0f, "ovla_laplace_dpo: nll_coef = %g (must not be negative or NaN)", (double)a->nll_coef);
  OVLA_REQUIRE(a->label_smoothing >= 0.0f && a->label_smoothing < 0.5f, "ovla_laplace_dpo: label_smoothing = %g (0 <= eps < 0.5)", (double)a->label_smoothing);
  OVLA_REQUIRE(a->loss_type == 0 || a->loss_type == 1, "ovla_laplace_dpo: loss_type = %d (0 sigmoid, 1 IPO)", a->loss_type);
  OVLA_REQUIRE(a->loss_type == 0 || a->beta > 0.0f, "ovla_laplace_dpo: the IPO loss needs beta > 0 (tau = 1 / (2 beta))");
  Scales sc;
  for (int d = 0; d < MAX_ADIM; ++d) {
    const bool in = !rows && d < a->adim;
    sc.inv_b[d] = in ? 1.0f / a->scale[d] : 1.0f;
    sc.log_norm[d] = in ? a->log_norm[d] : 0.0f;
  }
  const DpoScalars p = {a->s_lo, a->s_hi, a->beta, a->label_smoothing, a->grad_scale, a->nll_coef, a->nll_scale, a->loss_type, a->chunk, a->adim};
  auto kernel = rows ? laplace_dpo_kernel<true> : laplace_dpo_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)a->B), dim3(64), 0, (hipStream_t)stream_, (const bf16_bits*)a->pred, (const bf16_bits*)a->ref_pred,
                     (const bf16_bits*)a->log_scale, (const bf16_bits*)a->ref_log_scale, a->chosen, a->rejected, a->weight, a->logprob, a->ref_logprob, a->h,
                     a->margin, a->loss, a->coef, (bf16_bits*)a->dpred, (bf16_bits*)a->dlog_scale, sc, p);
  OVLA_CHECK_LAUNCH("ovla_laplace_dpo");
  return OVLA_OK;
}
