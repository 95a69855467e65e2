// common.h -- shared device/host helpers for libovla_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/ovla.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8_bits;  // 8 bf16 bit patterns = one MFMA A/B fragment
typedef __attribute__((ext_vector_type(4))) short bf16x4_bits;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef unsigned short bf16_bits;

#define OVLA_DEV __device__ __forceinline__

OVLA_DEV float bf2f(bf16_bits u) { return __uint_as_float(((unsigned)u) << 16); }
// round-to-nearest-even via the hardware convert (NaN stays NaN; see MI355X_MICROARCH "Correctness boundaries")
OVLA_DEV bf16_bits f2bf(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(bf16_bits, b);
}
OVLA_DEV float bfround(float f) { return bf2f(f2bf(f)); }

// erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7): ~12 instructions (v_rcp, v_exp, 5 FMAs) instead of libm's branchy
// erff (~100 executed instructions per wave with divergent lanes: it made the GELU epilogue of a ViT fc1 GEMM cost 40 % of the
// launch).  The GELU outputs are rounded to bf16 (2^-9 relative) right after, three orders of magnitude coarser.
OVLA_DEV float fast_erf(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * ax);
  const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
  const float y = 1.0f - poly * __expf(-ax * ax);
  return copysignf(y, x);
}
OVLA_DEV float gelu_erf(float x) { return 0.5f * x * (1.0f + fast_erf(x * 0.70710678118654752440f)); }
OVLA_DEV float gelu_erf_grad(float x) {
  const float cdf = 0.5f * (1.0f + fast_erf(x * 0.70710678118654752440f));
  const float pdf = 0.39894228040143267794f * __expf(-0.5f * x * x);
  return cdf + x * pdf;
}
// The sigmoid family is 1 / (1 + e) with e = __expf(-x), which overflows to inf at x = -88.7 although the result does not underflow before
// x = -104: up to there the value is exp(x) (x exp(x) for SiLU) to fp32 accuracy, 1e-39 ... 4e-37 after the factors that multiply it -- normal
// bf16 numbers that the overflow turned into 0.  exp2f (unlike __expf's bare v_exp_f32) returns denormals.  The select is taken only when e
// is inf, where the old result was 0: every result computed from a finite e keeps its bits.
OVLA_DEV float exp_tail(float x) { return exp2f(x * 1.44269504088896340736f); }
OVLA_DEV float sigmoidf_(float x) {
  const float e = __expf(-x);
  return e == INFINITY ? exp_tail(x) : 1.0f / (1.0f + e);
}
// tanh-GELU, 0.5 x (1 + tanh u) with u = k (x + c x^3), evaluated as x * sigmoid(2 u): the same function, but 1 + tanhf(u) cancels in fp32 for
// x < -4 (tanhf returns -1 or its neighbour: the result was -0 or -1.5e-7 where the value is 1e-8 ... 1e-10, hundreds of bf16 ulps), and
// sigmoid keeps its relative accuracy down to x = -10.1, where __expf overflows (gelu_tanh then returns -0 for a value below 1e-37; its
// derivative goes on through sigmoidf_'s tail).
// The derivative likewise: 0.5 (1 + t) = s and 1 - t^2 = 4 s (1 - s).  Its polynomial factor takes x clamped to [-16, 16] (one v_med3): beyond
// |x| = 16 the sigmoid is exactly 0 or 1 in fp32, the factor only has to stay finite (unclamped it overflows from |x| = 2e13 and the product
// was 0 * inf = NaN), and inside the clamp is the identity, so every bit a finite result had is unchanged.  s keeps the raw x: NaN in, NaN out.
OVLA_DEV float gelu_tanh(float x) {
  const float k = 0.7978845608028654f, c = 0.044715f;
  return x / (1.0f + __expf(-2.0f * k * (x + c * x * x * x)));
}
OVLA_DEV float gelu_tanh_grad(float x) {
  const float k = 0.7978845608028654f, c = 0.044715f;
  const float s = sigmoidf_(2.0f * k * (x + c * x * x * x));
  const float xc = fminf(fmaxf(x, -16.0f), 16.0f);
  return s * (1.0f + 2.0f * xc * (1.0f - s) * k * (1.0f + 3.0f * c * xc * xc));
}
OVLA_DEV float silu(float x) {
  const float e = __expf(-x);
  return e == INFINITY ? x * exp_tail(x) : x / (1.0f + e);
}

OVLA_DEV float apply_act(float v, int act) {
  switch (act) {
    case OVLA_ACT_GELU: return gelu_erf(v);
    case OVLA_ACT_RELU: return v > 0.f ? v : 0.f;
    case OVLA_ACT_SILU: return silu(v);
    case OVLA_ACT_GELU_TANH: return gelu_tanh(v);
    default: return v;
  }
}
OVLA_DEV float act_grad(float z, int act) {
  switch (act) {
    case OVLA_ACT_GELU: return gelu_erf_grad(z);
    case OVLA_ACT_RELU: return z > 0.f ? 1.f : 0.f;
    case OVLA_ACT_SILU: { float s = sigmoidf_(z); return s * (1.f + z * (1.f - s)); }
    case OVLA_ACT_GELU_TANH: return gelu_tanh_grad(z);
    default: return 1.f;
  }
}

// LayerNorm output element, y = (x - mean) * rstd * w + b in fp32 with ONE explicit fma (every kernel that normalises -- the row kernels of
// elementwise.hip -- goes through this function, so they agree bit for bit by construction).
OVLA_DEV float ln_affine(float x, float mean, float rstd, float w, float b) { return __builtin_fmaf((x - mean) * rstd, w, b); }

// multi-policy serving: the adapter slot an observation is routed to, read from a device array and clamped, so that no index formed from it leaves a buffer
OVLA_DEV int clamp_slot(int s, int n) { return s < 0 ? 0 : (s >= n ? n - 1 : s); }

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter c, key k -> four 32-bit words.  The one
// generator of the library: the lora_dropout masks (lora_dropout.hip) and the diffusion noise (diffusion_noise.hip) are functions of its output.
OVLA_DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

OVLA_DEV float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
OVLA_DEV float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- host side -------------------------------------------------------------------------------------------------
void ovla_set_error(const char* fmt, ...);
#define OVLA_REQUIRE(cond, ...)                \
  do {                                         \
    if (!(cond)) {                             \
      ovla_set_error(__VA_ARGS__);             \
      return OVLA_EINVAL;                      \
    }                                          \
  } while (0)
#define OVLA_CHECK_LAUNCH(name)                                                   \
  do {                                                                            \
    hipError_t e_ = hipGetLastError();                                            \
    if (e_ != hipSuccess) {                                                       \
      ovla_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));       \
      return OVLA_ELAUNCH;                                                        \
    }                                                                             \
  } while (0)

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
// the optional host copy of a device obs_slot array: an entry outside [0, n) is refused before anything is launched
static inline int check_host_slots(const int32_t* host, int n_obs, int n, const char* who) {
  if (!host) return OVLA_OK;
  for (int i = 0; i < n_obs; ++i)
    OVLA_REQUIRE(host[i] >= 0 && host[i] < n, "%s: obs_slot[%d] = %d is outside [0, %d)", who, i, host[i], n);
  return OVLA_OK;
}
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
