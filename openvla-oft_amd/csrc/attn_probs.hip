// attn_probs.hip -- the attention probabilities the flash kernels of attention.hip never materialise, for a list of query rows.
//
// ovla_attn_fwd leaves everything that defines P in HBM: the post-RoPE q | k it consumed and the fp32 lse it wrote.  This read-only kernel
// recomputes  P[r, h, k] = exp2(fp32(q . k) * (scale * log2e) - lse * log2e)  (the expression of the backward kernels) for the listed rows,
// per head and / or averaged over the heads, without touching V or O.
//
// Lane mapping: one wave owns 16 gathered query rows x 32 keys (two mfma_f32_16x16x32_bf16 tiles) and loops over the heads.  Scores are
// computed TRANSPOSED as in attention.hip, S^T = K . Q^T: the query row sits on the lane (lane & 15) and a lane's 4 accumulator registers are
// 4 CONSECUTIVE keys (4 (lane >> 4) + j) of that row, so a lane stores 16 contiguous bytes of P (Q . K^T would leave one dword per lane).
// Both operands are contraction-contiguous in global memory: every A / B fragment is one 16-byte load, no LDS.  The head mean accumulates
// in those same registers in head order (no atomics: the same bits on every run), so with P == NULL the per-head tensor never exists.
//
// The 16 rows of a block come from a device list and may belong to different batch entries, whose K differ: the wave walks the distinct
// batch entries of its rows (a wave-uniform loop, one pass when the rows are sorted) and every lane keeps only the pass of its own row's
// entry.  An MFMA column depends on its own B column alone, so a row's result is a function of its q row, its entry's K, lse and kv_len --
// never of the other rows of the block, of R or of B.  Rows outside [0, B S) read nothing and write zeros.
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int ROWS = 16;          // query rows per workgroup (the MFMA's N)
constexpr int WAVE_KEYS = 32;     // keys per wave: 2 MFMA tiles
constexpr int NT = WAVE_KEYS / 16;
constexpr int BLOCK_KEYS = 4 * WAVE_KEYS;
constexpr int PF = 3;             // heads whose operands a wave holds: the one it computes and PF - 1 in flight

struct ProbsParams {
  const bf16_bits *Q, *K;
  int64_t q_stride, k_stride;
  const float* lse;
  const int32_t* kv_len;
  const int32_t* rows;
  float *P, *Pm;
  int B, H, S, R, causal;
  float scale, inv_h;
};

// 4 consecutive keys key0 .. key0+3 of one output row (dst points at key 0 of the row)
template <bool VEC>
OVLA_DEV void store4(float* dst, int key0, int S, f32x4 v) {
  if constexpr (VEC) {
    if (key0 < S) *reinterpret_cast<f32x4*>(dst + key0) = v;   // S % 4 == 0: the four keys are inside or outside together
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (key0 + j < S) dst[key0 + j] = v[j];
  }
}

template <int HD, bool VEC>
__global__ __launch_bounds__(256) void attn_probs_kernel(const ProbsParams p) {
  constexpr int KS = HD / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, i = lane & 15;
  const int k0 = blockIdx.y * BLOCK_KEYS + wave * WAVE_KEYS;
  if (k0 >= p.S) return;   // wave-uniform; the kernel has no barrier
  const int r = blockIdx.x * ROWS + i;
  const bool listed = r < p.R;
  int64_t row = -1;
  if (listed) row = p.rows ? (int64_t)p.rows[r] : (int64_t)r;
  const bool valid = listed && row >= 0 && row < (int64_t)p.B * p.S;   // the index is checked BEFORE anything is addressed with it
  const int b = valid ? (int)(row / p.S) : -1;
  const int s_q = valid ? (int)(row - (int64_t)b * p.S) : 0;
  const float sl2 = p.scale * LOG2E;
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};

  if (listed && !valid) {   // a bad index: a zero row, nothing read
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int key0 = k0 + 16 * t + 4 * g;
      if (p.P)
        for (int h = 0; h < p.H; ++h) store4<VEC>(p.P + ((int64_t)r * p.H + h) * p.S, key0, p.S, zero4);
      if (p.Pm) store4<VEC>(p.Pm + (int64_t)r * p.S, key0, p.S, zero4);
    }
  }

  unsigned long long pend = __ballot(valid);
  while (pend) {
    const int first = __ffsll((long long)pend) - 1;
    const int bb = __builtin_amdgcn_readfirstlane(__shfl(b, first, 64));       // the batch entry of this pass
    const int64_t row_first = ((int64_t)bb) * p.S + __builtin_amdgcn_readfirstlane(__shfl(s_q, first, 64));
    const bool mine = valid && b == bb;
    int kv_end = p.kv_len ? p.kv_len[bb] : p.S;
    kv_end = kv_end < p.S ? kv_end : p.S;
    // lanes of another entry's rows feed their (discarded) columns with a row of the list that belongs to this entry
    const bf16_bits* Qr = p.Q + (mine ? row : row_first) * p.q_stride + 8 * g;
    const bf16_bits* Kb = p.K + (int64_t)bb * p.S * p.k_stride + 8 * g;
    const float* lse_r = p.lse + (int64_t)bb * p.H * p.S + (mine ? s_q : 0);
    int64_t koff[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      int kr = k0 + 16 * t + i;
      kr = kr < p.S ? kr : p.S - 1;   // rows past the end are clamped, their results masked below
      koff[t] = (int64_t)kr * p.k_stride;
    }
    f32x4 macc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) macc[t] = zero4;

    // One head's operands: the lane's q fragments, its k fragments of both key tiles and its row's lse.  Loaded without a branch (a tile of
    // padding keys reads clamped, valid rows and is masked below), PF - 1 heads AHEAD of the head being computed, so a wave always has
    // two heads' loads in flight behind its MFMAs and exp2s: left in program order the loop was one memory round trip per tile and head.
    struct HeadOps {
      bf16x8_bits q[KS], k[NT][KS];
      float L;
    };
    auto load_head = [&](int h, HeadOps& o) {
#pragma unroll
      for (int s = 0; s < KS; ++s) o.q[s] = *reinterpret_cast<const bf16x8_bits*>(Qr + (int64_t)h * HD + 32 * s);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int s = 0; s < KS; ++s) o.k[t][s] = *reinterpret_cast<const bf16x8_bits*>(Kb + koff[t] + (int64_t)h * HD + 32 * s);
      o.L = lse_r[(int64_t)h * p.S];
    };
    auto head = [&](int h, const HeadOps& o) {
      const float Lq = o.L * LOG2E;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int kt = k0 + 16 * t;
        f32x4 acc = zero4, pv;
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(o.k[t][s], o.q[s], acc, 0, 0, 0);   // acc[j] = q(lane & 15) . k(kt + 4 g + j)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int key = kt + 4 * g + j;
          const float e = __builtin_amdgcn_exp2f(acc[j] * sl2 - Lq);
          const bool ok = key < kv_end && (!p.causal || key <= s_q);
          pv[j] = ok ? e : 0.f;   // a select: a NaN in a masked K row stops here
          macc[t][j] += pv[j];
        }
        if (p.P && mine) store4<VEC>(p.P + ((int64_t)r * p.H + h) * p.S, kt + 4 * g, p.S, pv);
      }
    };
    if (k0 < kv_end) {   // wave-uniform
      HeadOps o[PF];   // a ring of PF heads' operands, indexed statically (the inner loop is unrolled)
#pragma unroll
      for (int u = 0; u < PF - 1; ++u) load_head(u < p.H ? u : p.H - 1, o[u]);
      for (int h0 = 0; h0 < p.H; h0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
          const int h = h0 + u;
          if (h < p.H) {
            // no branch around the loads (the compiler drains every outstanding load where such a branch joins): past the last head the
            // slot re-reads the last head, which nothing consumes
            load_head(h + PF - 1 < p.H ? h + PF - 1 : p.H - 1, o[(u + PF - 1) % PF]);
            head(h, o[u]);
          }
        }
      }
    } else if (p.P && mine) {   // the wave's 32 keys are all padding: zeros, nothing loaded or multiplied
      for (int h = 0; h < p.H; ++h)
#pragma unroll
        for (int t = 0; t < NT; ++t) store4<VEC>(p.P + ((int64_t)r * p.H + h) * p.S, k0 + 16 * t + 4 * g, p.S, zero4);
    }
    if (p.Pm && mine) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f32x4 m;
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = macc[t][j] * p.inv_h;
        store4<VEC>(p.Pm + (int64_t)r * p.S, k0 + 16 * t + 4 * g, p.S, m);
      }
    }
    pend &= ~__ballot(mine);
  }
}

}  // namespace

extern "C" int ovla_attn_probs(const ovla_attn_probs_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->Q && a->K && a->lse, "ovla_attn_probs: null pointer (Q, K and lse are required)");
  OVLA_REQUIRE(a->P || a->P_mean, "ovla_attn_probs: at least one of P and P_mean must be given");
  OVLA_REQUIRE(a->B > 0 && a->H > 0 && a->S > 0, "ovla_attn_probs: empty problem B=%d H=%d S=%d", a->B, a->H, a->S);
  OVLA_REQUIRE(a->R > 0, "ovla_attn_probs: R = %d rows (must be > 0)", a->R);
  OVLA_REQUIRE(a->head_dim == 64 || a->head_dim == 128, "ovla_attn_probs: head_dim %d not supported (64, 128)", a->head_dim);
  OVLA_REQUIRE(a->rows || (int64_t)a->R == (int64_t)a->B * a->S, "ovla_attn_probs: rows == NULL needs R == B * S (R=%d, B*S=%lld)", a->R,
               (long long)a->B * a->S);
  OVLA_REQUIRE((a->q_stride % 8) == 0 && (a->k_stride % 8) == 0 && a->q_stride >= 0 && a->k_stride >= 0,
               "ovla_attn_probs: row strides must be non-negative multiples of 8 elements");
  OVLA_REQUIRE(aligned16(a->Q) && aligned16(a->K), "ovla_attn_probs: Q and K must be 16-byte aligned");
  OVLA_REQUIRE((((uintptr_t)a->lse) & 3) == 0 && (((uintptr_t)a->P) & 3) == 0 && (((uintptr_t)a->P_mean) & 3) == 0 &&
                   (((uintptr_t)a->rows) & 3) == 0 && (((uintptr_t)a->kv_len) & 3) == 0,
               "ovla_attn_probs: lse, P, P_mean, rows and kv_len must be 4-byte aligned");
  ProbsParams p = {};
  p.Q = (const bf16_bits*)a->Q; p.K = (const bf16_bits*)a->K; p.q_stride = a->q_stride; p.k_stride = a->k_stride;
  p.lse = a->lse; p.kv_len = a->kv_len; p.rows = a->rows; p.P = a->P; p.Pm = a->P_mean;
  p.B = a->B; p.H = a->H; p.S = a->S; p.R = a->R; p.causal = a->causal; p.scale = a->scale; p.inv_h = 1.0f / (float)a->H;
  const bool vec = (a->S % 4) == 0 && aligned16(a->P) && aligned16(a->P_mean);   // 16-byte stores when every row of 4 keys is aligned
  const dim3 grid((unsigned)cdiv(a->R, ROWS), (unsigned)cdiv(a->S, BLOCK_KEYS));
  if (a->head_dim == 64) {
    if (vec) hipLaunchKernelGGL((attn_probs_kernel<64, true>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((attn_probs_kernel<64, false>), grid, dim3(256), 0, stream, p);
  } else {
    if (vec) hipLaunchKernelGGL((attn_probs_kernel<128, true>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((attn_probs_kernel<128, false>), grid, dim3(256), 0, stream, p);
  }
  OVLA_CHECK_LAUNCH("ovla_attn_probs");
  return OVLA_OK;
}
