// token_sample.hip -- the stochastic side of the discrete action-token path: ovla_sample_tokens draws each row's token from the tempered softmax
// over a token window by Gumbel-max and reports its log-probability and the row's entropy; ovla_token_pg computes, for given tokens, the same
// log-probability and entropy and the gradient of the clipped policy-gradient surrogate.  THE SAMPLING CONTRACT is in ovla.h "Token sampling and
// the policy-gradient objective"; the row reductions are token_row.h, the body ovla_token_ce is built from, so the three kernels agree bit for
// bit wherever they compute the same thing.  One workgroup of 256 lanes per row (rows are few -- B * A -- and 64 KB each: the passes re-read
// the row from L2); no LDS beyond the reduction slots, no atomics.  The group forms (GRPO: G draws per observation from one forward):
// ovla_sample_tokens_group is the sampler on a (rows, G) grid, one workgroup per draw; ovla_token_pg_group takes G given samples per row in
// one workgroup and stores the summed gradient of their surrogates, the KL penalty and the entropy bonus (G tokens and weights in LDS).
// s_j = z_j * invT, key_j = s_j + g and logprob = s_token - lse are separately rounded operations, as the numpy restatement computes them:
#pragma clang fp contract(off)
#include "common.h"
#include "token_row.h"
#include <math.h>

namespace {

struct Draw { uint32_t seed_lo, seed_hi, call, key; };

// the Gumbel variate of one generator word: u = (2 (w >> 9) + 1) 2^-24 is exact and strictly inside (0, 1)
OVLA_DEV float gumbel(uint32_t w) {
  const float u = (float)(2u * (w >> 9) + 1u) * 0x1p-24f;
  return -logf(-logf(u));
}

OVLA_DEV void take(float key, int j, float& m, int& mi) {
  if (key > m || (key == m && j < mi)) { m = key; mi = j; }
}

// VEC: 16-byte loads of the whole 8-column groups inside [lo, hi) (two generator calls per group), the head and the tail column by column.
// One workgroup per (row, draw): blockIdx.y is the draw g of gridDim.y = G (ovla_sample_tokens: G = 1); outputs and row keys are [rows, G],
// the entropy is the row's and draw 0 stores it.
template <bool VEC>
__global__ __launch_bounds__(256) void sample_tokens_kernel(const bf16_bits* __restrict__ logits, int64_t ld, int* __restrict__ token_out,
                                                            int* __restrict__ bin_out, float* __restrict__ logprob_out, float* __restrict__ entropy_out,
                                                            const uint32_t* __restrict__ state_dev, const int* __restrict__ row_key, Draw d, float invT,
                                                            int lo, int hi, int n_tokens, int n_bins) {
  __shared__ token_row::Shared sh;
  const int row = blockIdx.x, tid = threadIdx.x;
  const int out = row * (int)gridDim.y + (int)blockIdx.y;
  if (blockIdx.y != 0) entropy_out = nullptr;
  const bf16_bits* x = logits + (int64_t)row * ld;
  if (state_dev) { d.seed_lo = state_dev[0]; d.seed_hi = state_dev[1]; d.call = state_dev[2]; }
  d.key = (uint32_t)(row_key ? row_key[out] : out);
  const auto value = [x, invT](int j) { return bf2f(x[j]) * invT; };
  const auto scalar_key = [&](int j) {
    uint32_t o[4];
    philox4x32_10((uint32_t)j >> 2, d.key, 3u, d.call, d.seed_lo, d.seed_hi, o);
    return value(j) + gumbel(o[j & 3]);
  };

  // pass 1: the maximum key and the lowest index of it
  float km = -INFINITY; int ki = 0x7fffffff;
  int head_end = hi, tail0 = hi;
  if (VEC) {
    const int g0 = (lo + 7) >> 3, g1 = hi >> 3;
    if (g1 > g0) {
      head_end = g0 << 3; tail0 = g1 << 3;
      const uint4* xv = reinterpret_cast<const uint4*>(x);
      for (int g = g0 + tid; g < g1; g += 256) {
        const uint4 q = xv[g];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        uint32_t o[8];
        philox4x32_10(2u * (uint32_t)g, d.key, 3u, d.call, d.seed_lo, d.seed_hi, *reinterpret_cast<uint32_t(*)[4]>(&o[0]));
        philox4x32_10(2u * (uint32_t)g + 1u, d.key, 3u, d.call, d.seed_lo, d.seed_hi, *reinterpret_cast<uint32_t(*)[4]>(&o[4]));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float z = bf2f((bf16_bits)((k & 1) ? (w[k >> 1] >> 16) : (w[k >> 1] & 0xffffu)));
          take(z * invT + gumbel(o[k]), g * 8 + k, km, ki);
        }
      }
    }
  }
  for (int j = lo + tid; j < head_end; j += 256) take(scalar_key(j), j, km, ki);
  for (int j = tail0 + tid; j < hi; j += 256) take(scalar_key(j), j, km, ki);
  token_row::block_first_max(km, ki, lo, hi, sh);

  // pass 2, 3: the log-sum-exp and the entropy of s over the window (token_row.h)
  float m, s, es; int mi;
  token_row::row_max(value, lo, hi, sh, m, mi);
  if (entropy_out) token_row::row_sumexp<true>(value, lo, hi, m, sh, s, es);
  else token_row::row_sumexp<false>(value, lo, hi, m, sh, s, es);
  if (tid == 0) {
    const bool ok = fabsf(m) < INFINITY;   // a window without a finite maximum: lo / NaN
    const int tok = ok ? ki : lo;
    const float l = token_row::lse(s, m);
    int b = n_tokens - tok - 1;
    b = b < 0 ? 0 : (b > n_bins - 1 ? n_bins - 1 : b);
    token_out[out] = tok;
    bin_out[out] = b;
    logprob_out[out] = ok ? value(tok) - l : NAN;
    if (entropy_out) entropy_out[row] = ok ? l - es / s : NAN;
  }
}

__global__ __launch_bounds__(256) void token_pg_kernel(const bf16_bits* __restrict__ logits, int64_t ld, const int* __restrict__ tokens,
                                                       const float* __restrict__ advantage, const float* __restrict__ old_logprob,
                                                       float* __restrict__ logprob_out, float* __restrict__ entropy_out, float* __restrict__ ratio_out,
                                                       int* __restrict__ clipped_out, bf16_bits* dlogits, int64_t ld_d, float invT, float clip_lo,
                                                       float clip_hi, float grad_scale, int vocab, int lo, int hi) {
  __shared__ token_row::Shared sh;
  const int row = blockIdx.x, tid = threadIdx.x;
  const bf16_bits* x = logits + (int64_t)row * ld;
  int tok = tokens[row];
  tok = tok < lo ? lo : (tok >= hi ? hi - 1 : tok);   // no out-of-bounds read whatever the caller passed
  const auto value = [x, invT](int j) { return bf2f(x[j]) * invT; };
  const float s_tok = value(tok);             // read before the barriers below: the gradient pass may overwrite the row in place
  float m, s, es; int mi;
  token_row::row_max(value, lo, hi, sh, m, mi);
  token_row::row_sumexp<true>(value, lo, hi, m, sh, s, es);
  const float l = token_row::lse(s, m);
  const float logprob = s_tok - l;
  const float adv = advantage[row];
  const float ratio = old_logprob ? expf(logprob - old_logprob[row]) : 1.0f;
  const bool gated = (adv >= 0.0f && ratio > clip_hi) || (adv < 0.0f && ratio < clip_lo);
  if (tid == 0) {
    logprob_out[row] = logprob;
    entropy_out[row] = l - es / s;
    ratio_out[row] = ratio;
    clipped_out[row] = gated ? 1 : 0;
  }
  if (dlogits) {
    bf16_bits* dst = dlogits + (int64_t)row * ld_d;
    if (gated) {                              // stored as zeros, never multiplied through
      for (int j = tid; j < vocab; j += 256) dst[j] = 0;
      return;
    }
    const float c = ((adv * ratio) * grad_scale) * invT;
    const float inv = 1.0f / s;
    for (int j = tid; j < vocab; j += 256) {
      bf16_bits out = 0;
      if (j >= lo && j < hi) out = f2bf(token_row::grad_elem(__expf(value(j) - m), inv, j == tok ? 1.0f : 0.0f, c));
      dst[j] = out;
    }
  }
}

// G given samples per row (ovla.h: ovla_token_pg_group).  Lane g < G owns sample g: it reads s_tok_g before the first barrier (the gradient pass may
// overwrite the row in place), forms the sample's outputs and its weight w_g, and lane 0 compacts the samples with w_g != 0 in ascending g.
__global__ __launch_bounds__(256) void token_pg_group_kernel(const bf16_bits* __restrict__ logits, int64_t ld, const int* __restrict__ tokens,
                                                             const float* __restrict__ advantage, const float* __restrict__ old_logprob,
                                                             const float* __restrict__ ref_logprob, float* __restrict__ logprob_out,
                                                             float* __restrict__ ratio_out, int* __restrict__ clipped_out, float* __restrict__ kl_out,
                                                             float* __restrict__ entropy_out, bf16_bits* dlogits, int64_t ld_d, float invT, float clip_lo,
                                                             float clip_hi, float grad_scale, float kl_coef, float ent_scale, int G, int vocab, int lo,
                                                             int hi) {
  __shared__ token_row::Shared sh;
  __shared__ int g_tok[OVLA_PG_GROUP_MAX];
  __shared__ float g_w[OVLA_PG_GROUP_MAX];
  __shared__ int g_n;
  const int row = blockIdx.x, tid = threadIdx.x;
  const bf16_bits* x = logits + (int64_t)row * ld;
  const auto value = [x, invT](int j) { return bf2f(x[j]) * invT; };
  int tok = lo;
  float s_tok = 0.0f;
  if (tid < G) {
    tok = tokens[(int64_t)row * G + tid];
    tok = tok < lo ? lo : (tok >= hi ? hi - 1 : tok);
    s_tok = value(tok);
  }
  float m, s, es; int mi;
  token_row::row_max(value, lo, hi, sh, m, mi);
  token_row::row_sumexp<true>(value, lo, hi, m, sh, s, es);
  const float l = token_row::lse(s, m);
  const float H = l - es / s;
  if (tid < G) {
    const int64_t o = (int64_t)row * G + tid;
    const float logprob = s_tok - l;
    const float adv = advantage[o];
    const float ratio = old_logprob ? expf(logprob - old_logprob[o]) : 1.0f;
    const bool gated = (adv >= 0.0f && ratio > clip_hi) || (adv < 0.0f && ratio < clip_lo);
    float w = (gated || adv == 0.0f) ? 0.0f : ((adv * ratio) * grad_scale) * invT;   // (a zero advantage is set too: its ratio may be NaN)
    if (ref_logprob) {
      const float dd = ref_logprob[o] - logprob;
      const float em = expm1f(dd);
      kl_out[o] = em - dd;
      w = w + ((kl_coef * em) * grad_scale) * invT;
    }
    logprob_out[o] = logprob;
    ratio_out[o] = ratio;
    clipped_out[o] = gated ? 1 : 0;
    g_tok[tid] = tok;
    g_w[tid] = w;
  }
  if (tid == 0) entropy_out[row] = H;
  if (!dlogits) return;
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int g = 0; g < G; ++g) {
      const float w = g_w[g];
      if (w != 0.0f) { const int t = g_tok[g]; g_tok[n] = t; g_w[n] = w; ++n; }   // n <= g: a slot is read before it is overwritten
    }
    g_n = n;
  }
  __syncthreads();
  const int n = g_n;
  bf16_bits* dst = dlogits + (int64_t)row * ld_d;
  const bool ent = ent_scale != 0.0f;
  if (n == 0 && !ent) {                       // stored as zeros, never multiplied through
    for (int j = tid; j < vocab; j += 256) dst[j] = 0;
    return;
  }
  const float inv = 1.0f / s;
  const float ec = ent_scale * invT;
  for (int j = tid; j < vocab; j += 256) {
    bf16_bits out = 0;
    if (j >= lo && j < hi) {
      const float v = value(j);
      const float e = __expf(v - m);
      float acc = 0.0f;
      if (n > 0) {
        acc = token_row::grad_elem(e, inv, j == g_tok[0] ? 1.0f : 0.0f, g_w[0]);
        for (int g = 1; g < n; ++g) acc = acc + token_row::grad_elem(e, inv, j == g_tok[g] ? 1.0f : 0.0f, g_w[g]);
      }
      if (ent && e > 0.0f) acc = acc + (ec * (e * inv)) * ((v - l) + H);
      out = f2bf(acc);
    }
    dst[j] = out;
  }
}

bool window_ok(int vocab, int lo, int hi) { return lo >= 0 && lo < hi && hi <= vocab; }
}  // namespace

// the one launch behind ovla_sample_tokens (G = 1) and ovla_sample_tokens_group; `a` carries everything but G
template <class Args>
int launch_sample_tokens(const Args* a, int G, const char* name, hipStream_t stream) {
  const float invT = 1.0f / a->temperature;
  const Draw d{a->seed_lo, a->seed_hi, a->call, 0u};
  const bool vec = aligned16(a->logits) && (a->ld % 8) == 0;   // every row then starts on a 16-byte boundary
  if (vec)
    hipLaunchKernelGGL(sample_tokens_kernel<true>, dim3(a->rows, G), dim3(256), 0, stream, (const bf16_bits*)a->logits, a->ld, a->token, a->bin, a->logprob,
                       a->entropy, a->state_dev, a->row_key, d, invT, a->lo, a->hi, a->n_tokens, a->n_bins);
  else
    hipLaunchKernelGGL(sample_tokens_kernel<false>, dim3(a->rows, G), dim3(256), 0, stream, (const bf16_bits*)a->logits, a->ld, a->token, a->bin, a->logprob,
                       a->entropy, a->state_dev, a->row_key, d, invT, a->lo, a->hi, a->n_tokens, a->n_bins);
  OVLA_CHECK_LAUNCH(name);
  return OVLA_OK;
}

extern "C" int ovla_sample_tokens(const ovla_sample_tokens_args* a, void* stream_) {
  OVLA_REQUIRE(a && a->logits && a->token && a->bin && a->logprob, "ovla_sample_tokens: null pointer");
  OVLA_REQUIRE(a->rows > 0 && a->vocab > 0 && a->ld >= a->vocab && a->n_tokens > 0 && a->n_bins > 0, "ovla_sample_tokens: rows=%d vocab=%d ld=%lld n_tokens=%d n_bins=%d",
               a->rows, a->vocab, (long long)a->ld, a->n_tokens, a->n_bins);
  OVLA_REQUIRE(window_ok(a->vocab, a->lo, a->hi), "ovla_sample_tokens: window [%d, %d) is empty or leaves [0, %d)", a->lo, a->hi, a->vocab);
  OVLA_REQUIRE(a->temperature > 0.0f && a->temperature < INFINITY, "ovla_sample_tokens: temperature = %g (must be positive and finite)", (double)a->temperature);
  return launch_sample_tokens(a, 1, "ovla_sample_tokens", (hipStream_t)stream_);
}

extern "C" int ovla_sample_tokens_group(const ovla_sample_tokens_group_args* a, void* stream_) {
  OVLA_REQUIRE(a && a->logits && a->token && a->bin && a->logprob, "ovla_sample_tokens_group: null pointer");
  OVLA_REQUIRE(a->rows > 0 && a->vocab > 0 && a->ld >= a->vocab && a->n_tokens > 0 && a->n_bins > 0,
               "ovla_sample_tokens_group: rows=%d vocab=%d ld=%lld n_tokens=%d n_bins=%d", a->rows, a->vocab, (long long)a->ld, a->n_tokens, a->n_bins);
  OVLA_REQUIRE(a->G >= 1 && a->G <= OVLA_PG_GROUP_MAX && (int64_t)a->rows * a->G <= 0x7fffffff, "ovla_sample_tokens_group: G = %d (1 .. %d), rows = %d", a->G,
               OVLA_PG_GROUP_MAX, a->rows);
  OVLA_REQUIRE(window_ok(a->vocab, a->lo, a->hi), "ovla_sample_tokens_group: window [%d, %d) is empty or leaves [0, %d)", a->lo, a->hi, a->vocab);
  OVLA_REQUIRE(a->temperature > 0.0f && a->temperature < INFINITY, "ovla_sample_tokens_group: temperature = %g (must be positive and finite)",
               (double)a->temperature);
  return launch_sample_tokens(a, a->G, "ovla_sample_tokens_group", (hipStream_t)stream_);
}

extern "C" int ovla_token_pg(const ovla_token_pg_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->logits && a->tokens && a->advantage && a->logprob && a->entropy && a->ratio && a->clipped, "ovla_token_pg: null pointer");
  OVLA_REQUIRE(a->rows > 0 && a->vocab > 0 && a->ld >= a->vocab && (!a->dlogits || a->ld_d >= a->vocab), "ovla_token_pg: rows=%d vocab=%d ld=%lld ld_d=%lld", a->rows,
               a->vocab, (long long)a->ld, (long long)a->ld_d);
  OVLA_REQUIRE(window_ok(a->vocab, a->lo, a->hi), "ovla_token_pg: window [%d, %d) is empty or leaves [0, %d)", a->lo, a->hi, a->vocab);
  OVLA_REQUIRE(a->temperature > 0.0f && a->temperature < INFINITY, "ovla_token_pg: temperature = %g (must be positive and finite)", (double)a->temperature);
  OVLA_REQUIRE(a->clip_lo <= a->clip_hi, "ovla_token_pg: clip_lo = %g > clip_hi = %g (or a NaN bound)", (double)a->clip_lo, (double)a->clip_hi);
  hipLaunchKernelGGL(token_pg_kernel, dim3(a->rows), dim3(256), 0, stream, (const bf16_bits*)a->logits, a->ld, a->tokens, a->advantage, a->old_logprob, a->logprob,
                     a->entropy, a->ratio, a->clipped, (bf16_bits*)a->dlogits, a->ld_d, 1.0f / a->temperature, a->clip_lo, a->clip_hi, a->grad_scale, a->vocab, a->lo,
                     a->hi);
  OVLA_CHECK_LAUNCH("ovla_token_pg");
  return OVLA_OK;
}

extern "C" int ovla_token_pg_group(const ovla_token_pg_group_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->logits && a->tokens && a->advantage && a->logprob && a->entropy && a->ratio && a->clipped, "ovla_token_pg_group: null pointer");
  OVLA_REQUIRE(a->rows > 0 && a->vocab > 0 && a->ld >= a->vocab && (!a->dlogits || a->ld_d >= a->vocab), "ovla_token_pg_group: rows=%d vocab=%d ld=%lld ld_d=%lld",
               a->rows, a->vocab, (long long)a->ld, (long long)a->ld_d);
  OVLA_REQUIRE(a->G >= 1 && a->G <= OVLA_PG_GROUP_MAX, "ovla_token_pg_group: G = %d (1 .. %d)", a->G, OVLA_PG_GROUP_MAX);
  OVLA_REQUIRE(window_ok(a->vocab, a->lo, a->hi), "ovla_token_pg_group: window [%d, %d) is empty or leaves [0, %d)", a->lo, a->hi, a->vocab);
  OVLA_REQUIRE(a->temperature > 0.0f && a->temperature < INFINITY, "ovla_token_pg_group: temperature = %g (must be positive and finite)", (double)a->temperature);
  OVLA_REQUIRE(a->clip_lo <= a->clip_hi, "ovla_token_pg_group: clip_lo = %g > clip_hi = %g (or a NaN bound)", (double)a->clip_lo, (double)a->clip_hi);
  OVLA_REQUIRE(a->kl_coef >= 0.0f, "ovla_token_pg_group: kl_coef = %g (must not be negative or NaN)", (double)a->kl_coef);
  OVLA_REQUIRE(a->ent_scale == a->ent_scale, "ovla_token_pg_group: ent_scale is NaN");
  OVLA_REQUIRE((a->ref_logprob != nullptr) == (a->kl != nullptr), "ovla_token_pg_group: ref_logprob and kl come together (ref_logprob %s, kl %s)",
               a->ref_logprob ? "given" : "null", a->kl ? "given" : "null");
  hipLaunchKernelGGL(token_pg_group_kernel, dim3(a->rows), dim3(256), 0, stream, (const bf16_bits*)a->logits, a->ld, a->tokens, a->advantage, a->old_logprob,
                     a->ref_logprob, a->logprob, a->ratio, a->clipped, a->kl, a->entropy, (bf16_bits*)a->dlogits, a->ld_d, 1.0f / a->temperature, a->clip_lo,
                     a->clip_hi, a->grad_scale, a->kl_coef, a->ent_scale, a->G, a->vocab, a->lo, a->hi);
  OVLA_CHECK_LAUNCH("ovla_token_pg_group");
  return OVLA_OK;
}
