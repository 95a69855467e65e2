// diffusion_noise.hip -- DiffusionActionHead.sample_noisy_actions (prismatic/models/action_heads.py:167-197) in ONE launch: for a batch of
// ground-truth action chunks, the N(0, 1) noise, the per-sample training timestep, the noisy actions and each sample's timestep embedding.
// Every output is a pure function of (seed, call, stream, sample b, element i) -- the contract in ovla.h "Diffusion noise" -- so the position
// of the stream is one 32-bit counter the caller checkpoints, and a draw does not depend on the batch it is part of.
// Elementwise and tiny (a chunk is 56 .. 350 numbers per sample): one workgroup per sample, no LDS, no atomics; the cost is the launch.
// add_noise's mul / mul / add stay three separately rounded operations, as torch computes them:
#pragma clang fp contract(off)
#include "common.h"

namespace {

struct NoiseParams {
  const bf16_bits* actions; int64_t ld_actions;
  const float* ab;
  const bf16_bits* temb_table;
  bf16_bits* noise; int64_t ld_noise;
  bf16_bits* noisy; int64_t ld_noisy;
  bf16_bits* temb; int64_t ld_temb;
  int32_t* timesteps;
  uint32_t seed_lo, seed_hi, call, stream;
  int n, D, T;
  int vec;   // the timestep-embedding row moves as 16-byte vectors (D % 8 == 0, ld_temb % 8 == 0, both bases 16-byte aligned)
};

// One Box-Muller pair from two generator words: u1 in (0, 1], u2 in [0, 1), both exact in fp32.  cos(2 pi u2) / sin(2 pi u2) are evaluated as
// sincospif(2 u2): 2 u2 is exact, so the argument reduction is, and the pair keeps its RELATIVE accuracy next to the zeros of sin and cos
// (a 2 pi u2 rounded to fp32 would not: at u2 = 1/2 it yields sin = -8.7e-8 where the exact value is 0).
OVLA_DEV void box_muller(uint32_t wa, uint32_t wb, float& z_even, float& z_odd) {
  const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f;
  const float u2 = (float)(wb >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif(2.0f * u2, &s, &c);
  z_even = r * c;
  z_odd = r * s;
}

__global__ __launch_bounds__(256) void diffusion_noise_kernel(const NoiseParams p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  uint32_t o[4];
  // every thread evaluates the sample's timestep itself (one generator call): no broadcast, no barrier
  philox4x32_10(0u, (uint32_t)b, 1u, p.call, p.seed_lo, p.seed_hi, o);
  const int t = (int)__umulhi(o[0], (uint32_t)p.T);   // uniform on [0, T): floor(o[0] * T / 2^32)
  if (tid == 0) p.timesteps[b] = t;
  const bf16_bits* trow = p.temb_table + (int64_t)t * p.D;
  bf16_bits* tdst = p.temb + (int64_t)b * p.ld_temb;
  if (p.vec) {
    for (int j = tid; j < (p.D >> 3); j += 256) reinterpret_cast<bf16x8_bits*>(tdst)[j] = reinterpret_cast<const bf16x8_bits*>(trow)[j];
  } else {
    for (int j = tid; j < p.D; j += 256) tdst[j] = trow[j];
  }
  const float a0 = p.ab[2 * t], a1 = p.ab[2 * t + 1];
  const bf16_bits* arow = p.actions + (int64_t)b * p.ld_actions;
  bf16_bits* nrow = p.noise + (int64_t)b * p.ld_noise;
  bf16_bits* yrow = p.noisy + (int64_t)b * p.ld_noisy;
  for (int j = tid; 4 * j < p.n; j += 256) {
    philox4x32_10((uint32_t)j, (uint32_t)b, p.stream, p.call, p.seed_lo, p.seed_hi, o);
    float z[4];
    box_muller(o[0], o[1], z[0], z[1]);
    box_muller(o[2], o[3], z[2], z[3]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * j + e;
      if (i >= p.n) break;
      const bf16_bits nb = f2bf(z[e]);
      nrow[i] = nb;
      const float x = a0 * bf2f(arow[i]);
      const float y = a1 * bf2f(nb);
      yrow[i] = f2bf(x + y);
    }
  }
}
}  // namespace

extern "C" int ovla_diffusion_noise(const ovla_diffusion_noise_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->actions && a->ab && a->temb_table && a->noise && a->noisy && a->temb && a->timesteps, "ovla_diffusion_noise: null pointer");
  OVLA_REQUIRE(a->B > 0 && a->n > 0 && a->D > 0 && a->T > 0, "ovla_diffusion_noise: B=%d n=%d D=%d T=%d", a->B, a->n, a->D, a->T);
  OVLA_REQUIRE(a->stream != 1u, "ovla_diffusion_noise: stream 1 is the timestep draw, not a noise stream");
  OVLA_REQUIRE(a->stream == 0u || a->stream == 2u, "ovla_diffusion_noise: stream = %u (0: training noise, 2: the sampler's start noise)", a->stream);
  OVLA_REQUIRE(a->ld_actions >= a->n && a->ld_noise >= a->n && a->ld_noisy >= a->n && a->ld_temb >= a->D,
               "ovla_diffusion_noise: ld_actions=%lld ld_noise=%lld ld_noisy=%lld (>= n = %d), ld_temb=%lld (>= D = %d)", (long long)a->ld_actions,
               (long long)a->ld_noise, (long long)a->ld_noisy, a->n, (long long)a->ld_temb, a->D);
  NoiseParams p{};
  p.actions = (const bf16_bits*)a->actions; p.ld_actions = a->ld_actions;
  p.ab = a->ab; p.temb_table = (const bf16_bits*)a->temb_table;
  p.noise = (bf16_bits*)a->noise; p.ld_noise = a->ld_noise;
  p.noisy = (bf16_bits*)a->noisy; p.ld_noisy = a->ld_noisy;
  p.temb = (bf16_bits*)a->temb; p.ld_temb = a->ld_temb;
  p.timesteps = a->timesteps;
  p.seed_lo = a->seed_lo; p.seed_hi = a->seed_hi; p.call = a->call; p.stream = a->stream;
  p.n = a->n; p.D = a->D; p.T = a->T;
  p.vec = a->D % 8 == 0 && a->ld_temb % 8 == 0 && aligned16(a->temb) && aligned16(a->temb_table);
  hipLaunchKernelGGL(diffusion_noise_kernel, dim3(a->B), dim3(256), 0, stream, p);
  OVLA_CHECK_LAUNCH("ovla_diffusion_noise");
  return OVLA_OK;
}
