// lora_dropout.hip -- peft's lora_dropout (an independent nn.Dropout(p) in front of every adapted nn.Linear's lora_A, training mode only):
//   y = W x + s B_g(A_g(dropout_g(x))),   dropout_g(x) = bf16(float(x) / (1 - p)) where kept, +0 where dropped.
// The mask is a pure function of (seed, call, module, row, column) -- the contract in ovla.h "LoRA dropout" -- so no mask and no dropped
// activation has to exist in HBM in the forward: every kernel here evaluates Philox4x32-10 in registers for the 16-byte vector it holds.
//   ovla_lora_dropout_apply     xd_g = dropout_g(x) for up to 4 groups, x read once                  (elementwise; the backward's dA operand)
//   ovla_lora_dropout_proj      t[:, g r + j] = bf16(alpha sum_k xd_g[m, k] A[g r + j, k]), r = 32      (forward; x streams once for all groups)
//   ovla_lora_dropout_backproj  dx += sum_g keep_g ? inv (dt_g A_g) : 0, one read-modify-write pass  (backward)
// No atomics: t and dx feed the bit-reproducible gradient chain.  The scale multiply must stay a multiply followed by an add:
#pragma clang fp contract(off)
#include "common.h"

namespace {

struct MaskKey {
  uint32_t seed_lo, seed_hi, call, thr;
  float inv;
};

// The 8 keep bits (generator: common.h philox4x32_10) of the vector that starts at column k (k % 8 == 0) of row m of a [*, K] matrix: bit e = column k + e is kept.
OVLA_DEV uint32_t keep_bits(const MaskKey& mk, uint32_t module, int m, int k, int K) {
  const uint64_t q = (uint64_t)m * (uint64_t)(K >> 3) + (uint64_t)(k >> 3);
  uint32_t o[4];
  philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), module, mk.call, mk.seed_lo, mk.seed_hi, o);
  uint32_t bits = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    bits |= ((o[w] & 0xffffu) >= mk.thr ? 1u : 0u) << (2 * w);
    bits |= ((o[w] >> 16) >= mk.thr ? 1u : 0u) << (2 * w + 1);
  }
  return bits;
}

// kept: bf16_rne(float(x) * inv); dropped: +0 STORED (never multiplied: a NaN in a dropped position does not survive)
OVLA_DEV bf16x8_bits drop_vec(bf16x8_bits x, uint32_t bits, float inv) {
  bf16x8_bits y;
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = (bits >> e) & 1u ? (short)f2bf(bf2f((bf16_bits)x[e]) * inv) : (short)0;
  return y;
}

struct ApplyParams {
  const bf16_bits* x; int64_t ldx;
  bf16_bits* out[4];
  uint32_t module[4];
  MaskKey mk;
  int M, K, G;
};

// one thread per 16-byte vector of x; every group's copy is written from the one load
__global__ __launch_bounds__(256) void lora_dropout_apply_kernel(const ApplyParams p) {
  const int nvec = p.K >> 3;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)p.M * nvec) return;
  const int m = (int)(idx / nvec), k = (int)(idx - (int64_t)m * nvec) * 8;
  const bf16x8_bits x = *reinterpret_cast<const bf16x8_bits*>(p.x + (int64_t)m * p.ldx + k);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    if (g >= p.G) break;
    const uint32_t bits = keep_bits(p.mk, p.module[g], m, k, p.K);
    *reinterpret_cast<bf16x8_bits*>(p.out[g] + (int64_t)m * p.K + k) = drop_vec(x, bits, p.mk.inv);
  }
}

struct ProjParams {
  const bf16_bits* x; int64_t ldx;
  const bf16_bits* A; int64_t lda;
  bf16_bits* t; int64_t ldt;
  uint32_t module[4];
  MaskKey mk;
  float alpha;
  int M, K;
};

// One workgroup owns 16 rows x all G*32 columns; its 4 waves split K and reduce through LDS in wave order (gemm_skinny_kernel's scheme at
// half its row block: M = 4864 gives 304 workgroups for 256 CUs).  Both operands are K-contiguous, so a lane's 16-byte load IS its
// mfma_f32_16x16x32_bf16 fragment: x[m = lane & 15][k + 8 (lane >> 4) ..] is loaded once and masked per group in registers.
template <int G>
__global__ __launch_bounds__(256) void lora_dropout_proj_kernel(const ProjParams p) {
  constexpr int LDW = G * 32 + 4;
  __shared__ __attribute__((aligned(16))) float red[4][16][LDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * 16;
  const int ksteps = (p.K + 31) / 32;
  const int per_wave = (ksteps + 3) / 4;
  const int ks0 = wave * per_wave, ks1 = (ks0 + per_wave) < ksteps ? (ks0 + per_wave) : ksteps;
  const int kq = 8 * (lane >> 4);
  int mrow = m0 + (lane & 15);
  mrow = mrow < p.M ? mrow : p.M - 1;   // rows past M compute a copy of the last row and are not stored
  const bf16_bits* xrow = p.x + (int64_t)mrow * p.ldx;
  const bf16_bits* arow = p.A + (int64_t)(lane & 15) * p.lda;
  f32x4 acc[G][2];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[g][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16x8_bits zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int ks = ks0; ks < ks1; ++ks) {
    const int k = ks * 32 + kq;
    const bool kin = k < p.K;   // K % 8 == 0: a vector is inside or outside as a whole
    const bf16x8_bits x = kin ? *reinterpret_cast<const bf16x8_bits*>(xrow + k) : zero;
    bf16x8_bits a[G][2];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int j = 0; j < 2; ++j) a[g][j] = kin ? *reinterpret_cast<const bf16x8_bits*>(arow + (int64_t)(g * 32 + j * 16) * p.lda + k) : zero;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const bf16x8_bits xd = drop_vec(x, keep_bits(p.mk, p.module[g], mrow, kin ? k : 0, p.K), p.mk.inv);
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[g][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[g][j], xd, acc[g][j], 0, 0, 0);
    }
  }
  // lane owns C[m = lane & 15][n = g*32 + j*16 + 4*(lane >> 4) .. +3]
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int j = 0; j < 2; ++j) *reinterpret_cast<f32x4*>(&red[wave][lane & 15][g * 32 + j * 16 + 4 * (lane >> 4)]) = acc[g][j];
  __syncthreads();
  constexpr int QUADS = G * 8;
  for (int idx = tid; idx < 16 * QUADS; idx += 256) {
    const int row = idx / QUADS, c4 = (idx % QUADS) * 4;
    const int m = m0 + row;
    if (m >= p.M) continue;
    f32x4 v = *reinterpret_cast<const f32x4*>(&red[0][row][c4]);
    v += *reinterpret_cast<const f32x4*>(&red[1][row][c4]);
    v += *reinterpret_cast<const f32x4*>(&red[2][row][c4]);
    v += *reinterpret_cast<const f32x4*>(&red[3][row][c4]);
    bf16x4_bits o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (short)f2bf(v[j] * p.alpha);
    *reinterpret_cast<bf16x4_bits*>(p.t + (int64_t)m * p.ldt + c4) = o;
  }
}

struct BackprojParams {
  bf16_bits* dx; int64_t ld;
  const bf16_bits* dt; int64_t ld_dt;
  const bf16_bits* AT; int64_t ld_at;
  uint32_t module[4];
  MaskKey mk;
  int M, K, G, r;
};

// A wave owns 16 rows x 64 columns of dx, a workgroup 64 x 64.  The contraction runs over r <= 128 only: per group ceil(r / 32) MFMA steps
// on four 16-column tiles whose A^T rows are PERMUTED -- tile t takes the rows  32 (t >> 1) + 8 (i >> 2) + 4 (t & 1) + (i & 3), i = lane & 15
// -- so that lane (m = lane & 15, q = lane >> 4) ends up with the 8 consecutive columns 32 h + 8 q .. + 7 of half h in acc[2h], acc[2h + 1]:
// exactly one mask vector, one Philox call and one 16-byte read-modify-write of dx.
__global__ __launch_bounds__(256) void lora_dropout_backproj_kernel(const BackprojParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 64;
  const int m = blockIdx.y * 64 + wave * 16 + (lane & 15);
  const int mc = m < p.M ? m : p.M - 1;
  const int q = lane >> 4, i = lane & 15;
  const bf16_bits* dtrow = p.dt + (int64_t)mc * p.ld_dt;
  const bf16_bits* atrow[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    int k = n0 + 32 * (t >> 1) + 8 * (i >> 2) + 4 * (t & 1) + (i & 3);
    k = k < p.K ? k : p.K - 1;   // columns past K are computed from the last row of A^T and not stored
    atrow[t] = p.AT + (int64_t)k * p.ld_at;
  }
  float sum[2][8];
  bool live[2];
  bf16x8_bits old[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = n0 + 32 * h + 8 * q;
    live[h] = m < p.M && k < p.K;
    if (live[h]) old[h] = *reinterpret_cast<const bf16x8_bits*>(p.dx + (int64_t)m * p.ld + k);
#pragma unroll
    for (int e = 0; e < 8; ++e) sum[h][e] = live[h] ? bf2f((bf16_bits)old[h][e]) : 0.f;
  }
  const bf16x8_bits zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const int jsteps = (p.r + 31) / 32;
  for (int g = 0; g < p.G; ++g) {
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int js = 0; js < jsteps; ++js) {
      const int j = js * 32 + 8 * q;
      const bool jin = j < p.r;   // r % 8 == 0; the fragment is zero-padded to the MFMA's K in registers
      const bf16x8_bits a = jin ? *reinterpret_cast<const bf16x8_bits*>(dtrow + g * p.r + j) : zero;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bf16x8_bits b = jin ? *reinterpret_cast<const bf16x8_bits*>(atrow[t] + g * p.r + j) : zero;
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, acc[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (!live[h]) continue;
      const uint32_t bits = keep_bits(p.mk, p.module[g], m, n0 + 32 * h + 8 * q, p.K);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float term = p.mk.inv * acc[2 * h + (e >> 2)][e & 3];
        sum[h][e] += (bits >> e) & 1u ? term : 0.f;
      }
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (!live[h]) continue;
    bf16x8_bits o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (short)f2bf(sum[h][e]);
    *reinterpret_cast<bf16x8_bits*>(p.dx + (int64_t)m * p.ld + n0 + 32 * h + 8 * q) = o;
  }
}

int make_key(float p, uint32_t seed_lo, uint32_t seed_hi, uint32_t call, const char* who, MaskKey* mk) {
  OVLA_REQUIRE(p >= 0.f && p < 1.f, "%s: p = %g is outside [0, 1)", who, (double)p);
  mk->seed_lo = seed_lo; mk->seed_hi = seed_hi; mk->call = call;
  mk->thr = (uint32_t)((double)p * 65536.0);   // floor: p >= 0
  mk->inv = 1.0f / (1.0f - p);
  return OVLA_OK;
}
}  // namespace

extern "C" int ovla_lora_dropout_apply(const ovla_lora_dropout_apply_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->x, "ovla_lora_dropout_apply: null pointer");
  OVLA_REQUIRE(a->M > 0 && a->K > 0 && a->G >= 1 && a->G <= 4, "ovla_lora_dropout_apply: M=%d K=%d G=%d (G in 1..4)", a->M, a->K, a->G);
  OVLA_REQUIRE(a->K % 8 == 0 && a->ldx % 8 == 0 && a->ldx >= a->K && aligned16(a->x), "ovla_lora_dropout_apply: K=%d ldx=%lld (K %% 8, ldx %% 8, ldx >= K, 16-byte base)",
               a->K, (long long)a->ldx);
  ApplyParams p{};
  p.x = (const bf16_bits*)a->x; p.ldx = a->ldx; p.M = a->M; p.K = a->K; p.G = a->G;
  for (int g = 0; g < a->G; ++g) {
    OVLA_REQUIRE(a->out[g] && aligned16(a->out[g]) && a->out[g] != a->x, "ovla_lora_dropout_apply: out[%d] is null, misaligned or aliases x", g);
    p.out[g] = (bf16_bits*)a->out[g];
    p.module[g] = a->module[g];
  }
  if (int rc = make_key(a->p, a->seed_lo, a->seed_hi, a->call, "ovla_lora_dropout_apply", &p.mk)) return rc;
  const int64_t total = (int64_t)a->M * (a->K / 8);
  OVLA_REQUIRE((total + 255) / 256 <= 0x7fffffffLL, "ovla_lora_dropout_apply: %lld vectors need more than 2^31 - 1 workgroups", (long long)total);
  hipLaunchKernelGGL(lora_dropout_apply_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, p);
  OVLA_CHECK_LAUNCH("ovla_lora_dropout_apply");
  return OVLA_OK;
}

extern "C" int ovla_lora_dropout_proj(const ovla_lora_dropout_proj_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->x && a->A && a->t, "ovla_lora_dropout_proj: null pointer");
  OVLA_REQUIRE(a->M > 0 && a->K > 0 && a->G >= 1 && a->G <= 4 && a->r == 32, "ovla_lora_dropout_proj: M=%d K=%d G=%d r=%d (G in 1..4, r == 32)", a->M, a->K, a->G, a->r);
  OVLA_REQUIRE(a->K % 8 == 0 && a->ldx % 8 == 0 && a->lda % 8 == 0 && a->ldx >= a->K && a->lda >= a->K && aligned16(a->x) && aligned16(a->A),
               "ovla_lora_dropout_proj: K=%d ldx=%lld lda=%lld (K %% 8, ld %% 8, ld >= K, 16-byte bases)", a->K, (long long)a->ldx, (long long)a->lda);
  OVLA_REQUIRE(a->ldt % 4 == 0 && a->ldt >= (int64_t)a->G * a->r && (((uintptr_t)a->t) & 7) == 0, "ovla_lora_dropout_proj: ldt=%lld (ldt %% 4, ldt >= G*r, 8-byte base)",
               (long long)a->ldt);
  ProjParams p{};
  p.x = (const bf16_bits*)a->x; p.ldx = a->ldx; p.A = (const bf16_bits*)a->A; p.lda = a->lda; p.t = (bf16_bits*)a->t; p.ldt = a->ldt;
  p.alpha = a->alpha; p.M = a->M; p.K = a->K;
  for (int g = 0; g < a->G; ++g) p.module[g] = a->module[g];
  if (int rc = make_key(a->p, a->seed_lo, a->seed_hi, a->call, "ovla_lora_dropout_proj", &p.mk)) return rc;
  const dim3 grid(cdiv(a->M, 16)), block(256);
  switch (a->G) {
    case 1: hipLaunchKernelGGL(lora_dropout_proj_kernel<1>, grid, block, 0, stream, p); break;
    case 2: hipLaunchKernelGGL(lora_dropout_proj_kernel<2>, grid, block, 0, stream, p); break;
    case 3: hipLaunchKernelGGL(lora_dropout_proj_kernel<3>, grid, block, 0, stream, p); break;
    default: hipLaunchKernelGGL(lora_dropout_proj_kernel<4>, grid, block, 0, stream, p); break;
  }
  OVLA_CHECK_LAUNCH("ovla_lora_dropout_proj");
  return OVLA_OK;
}

extern "C" int ovla_lora_dropout_backproj(const ovla_lora_dropout_backproj_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->dx && a->dt && a->AT, "ovla_lora_dropout_backproj: null pointer");
  OVLA_REQUIRE(a->M > 0 && a->K > 0 && a->G >= 1 && a->G <= 4 && a->r > 0 && a->r % 8 == 0 && a->r <= 128,
               "ovla_lora_dropout_backproj: M=%d K=%d G=%d r=%d (G in 1..4, r %% 8, r <= 128)", a->M, a->K, a->G, a->r);
  const int64_t width = (int64_t)a->G * a->r;
  OVLA_REQUIRE(a->K % 8 == 0 && a->ld % 8 == 0 && a->ld >= a->K && aligned16(a->dx), "ovla_lora_dropout_backproj: K=%d ld=%lld (K %% 8, ld %% 8, ld >= K, 16-byte base)", a->K,
               (long long)a->ld);
  OVLA_REQUIRE(a->ld_dt % 8 == 0 && a->ld_at % 8 == 0 && a->ld_dt >= width && a->ld_at >= width && aligned16(a->dt) && aligned16(a->AT),
               "ovla_lora_dropout_backproj: ld_dt=%lld ld_at=%lld G*r=%lld (ld %% 8, ld >= G*r, 16-byte bases)", (long long)a->ld_dt, (long long)a->ld_at, (long long)width);
  OVLA_REQUIRE(cdiv(a->M, 64) <= 65535, "ovla_lora_dropout_backproj: M=%d needs more than 65535 row blocks", a->M);
  BackprojParams p{};
  p.dx = (bf16_bits*)a->dx; p.ld = a->ld; p.dt = (const bf16_bits*)a->dt; p.ld_dt = a->ld_dt; p.AT = (const bf16_bits*)a->AT; p.ld_at = a->ld_at;
  p.M = a->M; p.K = a->K; p.G = a->G; p.r = a->r;
  for (int g = 0; g < a->G; ++g) p.module[g] = a->module[g];
  if (int rc = make_key(a->p, a->seed_lo, a->seed_hi, a->call, "ovla_lora_dropout_backproj", &p.mk)) return rc;
  hipLaunchKernelGGL(lora_dropout_backproj_kernel, dim3(cdiv(a->K, 64), cdiv(a->M, 64)), dim3(256), 0, stream, p);
  OVLA_CHECK_LAUNCH("ovla_lora_dropout_backproj");
  return OVLA_OK;
}
