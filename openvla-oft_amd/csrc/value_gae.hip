// value_gae.hip -- the critic's side of PPO on the L1 head: a value head predicts one number per chunk step beside the head's prediction.
// ovla_value_loss pools that output into one value per observation and forms the (optionally clipped) squared-error loss against a return,
// its gradient in the layout ovla_head_out_bwd takes, and the sums the host turns into mean loss, clip fraction and explained variance.
// ovla_gae walks a rollout buffer backwards into advantages and returns; ovla_advantage_normalize standardises the advantages in place.
// Nothing is read back between them: a rollout buffer on the device goes into the training step as it is.
// THE CONTRACT is in ovla.h "Value head and generalised advantage estimation"; tests/value_gae_reference.py restates it.  Launch shapes:
// ovla_value_loss ONE 64-lane workgroup (lane b % 64 forms observation b's outputs into LDS, a barrier, lane 0 adds the tile's terms to the
// statistics in ascending b, a barrier, the next tile of 64); ovla_gae one lane per trajectory; ovla_advantage_normalize ONE 256-lane workgroup
// (strided per-lane sums in double, a halving tree through LDS).  No atomics, no workspace.
// Every operator below is one rounded operation of the type written, as the numpy restatement computes it:
#pragma clang fp contract(off)
#include "common.h"
#include <math.h>

namespace {

constexpr int NORM_LANES = 256;               // ovla.h: the lane count of the normalisation's fixed summation order
constexpr int64_t NORM_MAX = (int64_t)1 << 20;

// one observation's loss terms from its pooled value
struct ValueTerms { float loss, dl; bool clipped; };

OVLA_DEV ValueTerms value_terms(float v, float R, float old, float clip) {
  ValueTerms t;
  const float e = v - R;
  float l = e * e;
  t.dl = e;
  t.clipped = false;
  if (clip > 0.0f) {
    const float d = v - old;
    const float vc = old + fminf(fmaxf(d, -clip), clip);
    const float ec = vc - R;
    const float lc = ec * ec;
    if (lc > l) {                              // (false for a NaN: the unclipped branch; equality is the unclipped branch too)
      l = lc;
      t.dl = 0.0f;
      t.clipped = true;
    }
  }
  t.loss = 0.5f * l;
  return t;
}

__global__ __launch_bounds__(64) void value_loss_kernel(const bf16_bits* __restrict__ u, const float* __restrict__ returns, const float* __restrict__ old_value,
                                                        const int* __restrict__ valid, float* __restrict__ value, bf16_bits* __restrict__ du,
                                                        float* __restrict__ stats, float value_clip, float grad_scale, float inv_chunk, int B, int chunk) {
  __shared__ float sh_loss[64], sh_v[64], sh_R[64];
  __shared__ int sh_flag[64];                 // bit 0: counted (valid), bit 1: clipped
  const int tid = threadIdx.x;
  double n_valid = 0.0, n_clip = 0.0, s_loss = 0.0, s_v = 0.0, s_R = 0.0, s_err = 0.0, s_RR = 0.0;   // lane 0's
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + tid;
    int flag = 0;
    if (b < B) {
      const bf16_bits* u_row = u + (int64_t)b * chunk;
      float acc = 0.0f;
      for (int c = 0; c < chunk; ++c) acc = acc + bf2f(u_row[c]);
      const float v = acc / (float)chunk;
      value[b] = v;
      if (returns) {
        const bool is_valid = !valid || valid[b] != 0;
        float w = 0.0f;
        bool live = false;
        if (is_valid) {                        // an observation that is not valid: its return and old value are not even read
          const float R = returns[b];
          const ValueTerms t = value_terms(v, R, value_clip > 0.0f ? old_value[b] : 0.0f, value_clip);
          flag = 1 | (t.clipped ? 2 : 0);
          sh_loss[tid] = t.loss, sh_v[tid] = v, sh_R[tid] = R;
          if (t.dl != 0.0f) {
            w = t.dl * grad_scale;
            live = true;
          }
        }
        if (du) {
          const bf16_bits g = live ? f2bf(w * inv_chunk) : (bf16_bits)0;   // +0 set, never multiplied through
          bf16_bits* du_row = du + (int64_t)b * chunk;
          for (int c = 0; c < chunk; ++c) du_row[c] = g;
        }
      }
    }
    if (!returns) continue;                    // (uniform: no barrier is skipped by some lanes only)
    sh_flag[tid] = flag;
    __syncthreads();
    if (tid == 0) {
      const int m = B - b0 < 64 ? B - b0 : 64;
      for (int i = 0; i < m; ++i) {
        if (!(sh_flag[i] & 1)) continue;
        const double v = (double)sh_v[i], R = (double)sh_R[i];
        const double r = R - v;
        n_valid = n_valid + 1.0;
        if (sh_flag[i] & 2) n_clip = n_clip + 1.0;
        s_loss = s_loss + (double)sh_loss[i];
        s_v = s_v + v;
        s_R = s_R + R;
        s_err = s_err + r * r;
        s_RR = s_RR + R * R;
      }
    }
    __syncthreads();
  }
  if (returns && tid == 0) {
    stats[0] = (float)n_valid, stats[1] = (float)n_clip, stats[2] = (float)s_loss, stats[3] = (float)s_v;
    stats[4] = (float)s_R, stats[5] = (float)s_err, stats[6] = (float)s_RR, stats[7] = 0.0f;
  }
}

// the length of trajectory n as both rollout kernels take it: T without `length`; clamped to [0, T] so that no index formed from it leaves a buffer
// (the host refuses a length outside [0, T] when it is handed the host copy)
OVLA_DEV int traj_len(const int* __restrict__ length, int n, int T) {
  if (!length) return T;
  const int l = length[n];
  return l < 0 ? 0 : (l > T ? T : l);
}

__global__ __launch_bounds__(64) void gae_kernel(const float* __restrict__ reward, const float* __restrict__ value, const float* __restrict__ bootstrap,
                                                 const uint8_t* __restrict__ done, const int* __restrict__ length, float* __restrict__ adv,
                                                 float* __restrict__ ret, float gamma, float gamma_lambda, int N, int T) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  const int len = traj_len(length, n, T);
  const int64_t row = (int64_t)n * T;
  for (int t = T - 1; t >= len; --t) adv[row + t] = 0.0f, ret[row + t] = 0.0f;
  if (len == 0) return;                        // (the bootstrap is not read either)
  float carry = 0.0f;
  float vnext = bootstrap[n];
  for (int t = len - 1; t >= 0; --t) {
    const float nd = done[row + t] ? 0.0f : 1.0f;
    const float v = value[row + t];
    const float delta = (reward[row + t] + (gamma * vnext) * nd) - v;
    carry = delta + (gamma_lambda * nd) * carry;
    adv[row + t] = carry;
    ret[row + t] = carry + v;
    vnext = v;
  }
}

// halving tree over NORM_LANES doubles in LDS: s[i] = s[i] + s[i + h] for h = 128, 64, ..., 1; the total is left in s[0] and returned to every lane
OVLA_DEV double tree_sum(double* s, int tid, double mine) {
  __syncthreads();                             // the previous tree's s[0] has been read by every lane
  s[tid] = mine;
  __syncthreads();
  for (int h = NORM_LANES / 2; h > 0; h >>= 1) {
    if (tid < h) s[tid] = s[tid] + s[tid + h];
    __syncthreads();
  }
  return s[0];
}

__global__ __launch_bounds__(NORM_LANES) void advantage_normalize_kernel(float* __restrict__ adv, const int* __restrict__ length, float eps, int N, int T) {
  __shared__ double s[NORM_LANES];
  const int tid = threadIdx.x;
  const int total = N * T;                     // <= 2^20
  double sum = 0.0, cnt = 0.0;
  for (int e = tid; e < total; e += NORM_LANES) {
    const int n = e / T;
    if (e - n * T < traj_len(length, n, T)) {
      sum = sum + (double)adv[e];
      cnt = cnt + 1.0;
    }
  }
  const double count = tree_sum(s, tid, cnt);
  if (count == 0.0) return;                    // (uniform)
  const double mean = tree_sum(s, tid, sum) / count;
  double sq = 0.0;
  for (int e = tid; e < total; e += NORM_LANES) {
    const int n = e / T;
    if (e - n * T < traj_len(length, n, T)) {
      const double d = (double)adv[e] - mean;
      sq = sq + d * d;
    }
  }
  const double var = tree_sum(s, tid, sq) / count;
  const float mean_f = (float)mean;
  const float denom = (float)sqrt(var) + eps;
  for (int e = tid; e < total; e += NORM_LANES) {
    const int n = e / T;
    if (e - n * T < traj_len(length, n, T)) adv[e] = (adv[e] - mean_f) / denom;
  }
}

// the optional host copy of a device length array: an entry outside [0, T] is refused before anything is launched
int check_host_lengths(const int32_t* host, int N, int T, const char* who) {
  if (!host) return OVLA_OK;
  for (int i = 0; i < N; ++i) OVLA_REQUIRE(host[i] >= 0 && host[i] <= T, "%s: length[%d] = %d is outside [0, %d]", who, i, host[i], T);
  return OVLA_OK;
}
}  // namespace

extern "C" int ovla_value_loss(const ovla_value_loss_args* a, void* stream_) {
  OVLA_REQUIRE(a && a->u && a->value, "ovla_value_loss: null pointer");
  OVLA_REQUIRE(a->B > 0 && a->chunk > 0, "ovla_value_loss: B=%d chunk=%d", a->B, a->chunk);
  OVLA_REQUIRE(a->value_clip >= 0.0f, "ovla_value_loss: value_clip = %g (must not be negative or NaN)", (double)a->value_clip);
  if (a->returns) {
    OVLA_REQUIRE(a->stats, "ovla_value_loss: returns without stats");
    OVLA_REQUIRE(!(a->value_clip > 0.0f) || a->old_value, "ovla_value_loss: value_clip = %g needs old_value", (double)a->value_clip);
  }
  const float inv_chunk = 1.0f / (float)a->chunk;
  hipLaunchKernelGGL(value_loss_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, (const bf16_bits*)a->u, a->returns, a->old_value, a->valid, a->value,
                     (bf16_bits*)a->du, a->stats, a->value_clip, a->grad_scale, inv_chunk, a->B, a->chunk);
  OVLA_CHECK_LAUNCH("ovla_value_loss");
  return OVLA_OK;
}

extern "C" int ovla_gae(const ovla_gae_args* a, void* stream_) {
  OVLA_REQUIRE(a && a->reward && a->value && a->bootstrap && a->done && a->adv && a->ret, "ovla_gae: null pointer");
  OVLA_REQUIRE(a->N > 0 && a->T > 0, "ovla_gae: N=%d T=%d", a->N, a->T);
  OVLA_REQUIRE(a->gamma >= 0.0f && a->gamma <= 1.0f, "ovla_gae: gamma = %g (0 .. 1)", (double)a->gamma);
  OVLA_REQUIRE(a->gamma_lambda >= 0.0f && a->gamma_lambda <= 1.0f, "ovla_gae: gamma_lambda = %g (0 .. 1)", (double)a->gamma_lambda);
  OVLA_REQUIRE(!a->length_host || a->length, "ovla_gae: length_host without length");
  if (int rc = check_host_lengths(a->length_host, a->N, a->T, "ovla_gae")) return rc;
  hipLaunchKernelGGL(gae_kernel, dim3((unsigned)cdiv(a->N, 64)), dim3(64), 0, (hipStream_t)stream_, a->reward, a->value, a->bootstrap, a->done, a->length,
                     a->adv, a->ret, a->gamma, a->gamma_lambda, a->N, a->T);
  OVLA_CHECK_LAUNCH("ovla_gae");
  return OVLA_OK;
}

extern "C" int ovla_advantage_normalize(const ovla_advantage_normalize_args* a, void* stream_) {
  OVLA_REQUIRE(a && a->adv, "ovla_advantage_normalize: null pointer");
  OVLA_REQUIRE(a->N > 0 && a->T > 0 && (int64_t)a->N * a->T <= NORM_MAX, "ovla_advantage_normalize: N=%d T=%d (N * T <= 2^20)", a->N, a->T);
  OVLA_REQUIRE(a->eps > 0.0f && a->eps < INFINITY, "ovla_advantage_normalize: eps = %g (positive and finite)", (double)a->eps);
  OVLA_REQUIRE(!a->length_host || a->length, "ovla_advantage_normalize: length_host without length");
  if (int rc = check_host_lengths(a->length_host, a->N, a->T, "ovla_advantage_normalize")) return rc;
  hipLaunchKernelGGL(advantage_normalize_kernel, dim3(1), dim3(NORM_LANES), 0, (hipStream_t)stream_, a->adv, a->length, a->eps, a->N, a->T);
  OVLA_CHECK_LAUNCH("ovla_advantage_normalize");
  return OVLA_OK;
}
