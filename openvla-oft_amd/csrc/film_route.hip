// film_route.hip -- per-policy FiLM in multi-policy serving (ovla_film_vectors): every scale / shift Linear of both towers, for every observation of
// the forward under ITS OWN policy's weights, in ONE launch.  out_j[b, c] = bf16(bias_j[slot(b)][c] + sum_k W_j[slot(b)][c, k] * avg[b, k]), fp32 sums.
//
// Shape (a batch of GEMVs: the weights are streamed once and shared by nothing, so they go straight to registers):
//   outer loops   slot s = 0 .. n-1, then the observations routed to s in ascending order, FILM_GOBS (or what fits in LDS) at a time.  A slot
//                 without observations is skipped before any address of it is formed; the group's avg rows are staged in LDS once.
//   items         4 consecutive output columns of one Linear; item i belongs to the Linear with item_start <= i (binary search).  Workgroup w takes
//                 the items 8 w + wave, grid-strided: one wave per item, 4 weight rows in flight per wave, two 16-byte loads deep per row.
//   arithmetic    lane l owns the 16-byte k-vectors l, l + 64, l + 128, ... of every row and adds them in that order (v_dot2c_f32_bf16, element pairs
//                 in order); the 64 lane sums go through one fixed exchange tree (lane distances 32, 16, 8, 4, 2, 1).  Nothing in that order depends
//                 on n_obs, on the observation's position or group, on n or on the grid, and a row's accumulators see its own avg row and its own
//                 slot's weights only (selected by address, never by a 0 / 1 factor): the bits of out_j[b, :] are a function of avg[b, :], the
//                 weights of slot(b), D and out_f.
// No atomics, no cross-workgroup communication; every loop is bounded by an argument.
#include "common.h"

namespace {

constexpr int FILM_THREADS = 512;
constexpr int FILM_WAVES = FILM_THREADS / 64;
constexpr int FILM_ROWS = OVLA_FILM_ITEM_COLS;   // weight rows (output columns) per wave item
constexpr int FILM_GOBS = 8;                     // observations per staged group (accumulators: FILM_ROWS * FILM_GOBS per lane)
constexpr int FILM_HEAD_BYTES = 512;             // LDS header: slot[64], group idx[8], count, scan position
constexpr int FILM_LDS_MAX = 160 * 1024;         // per workgroup on gfx950
constexpr int FILM_MAX_GRID = 1024;

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
#define OVLA_GLOBAL __attribute__((address_space(1)))

// acc[r][g] += w[r] . x_g over the 8 elements of one k-vector, element pairs in order, for the cnt staged observations (cnt is wave-uniform)
OVLA_DEV void mac_vec(float (&acc)[FILM_ROWS * FILM_GOBS], const u32x4 (&w)[FILM_ROWS], const u32x4* __restrict__ x, int ldx, int cnt) {
#pragma unroll
  for (int g = 0; g < FILM_GOBS; ++g) {
    if (g < cnt) {
      const u32x4 xv = x[g * ldx];
#pragma unroll
      for (int r = 0; r < FILM_ROWS; ++r)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const unsigned wp = w[r][p], xp = xv[p];   // (bit_cast of the element expression itself reads element 0 for every p)
          acc[r * FILM_GOBS + g] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, wp), __builtin_bit_cast(bf16x2_t, xp), acc[r * FILM_GOBS + g], false);
        }
    }
  }
}

// One level of the lane-sum tree: at lane distance X a lane keeps H of its 2 H values and hands the other H to its partner.
template <int H, int X>
OVLA_DEV void exchange(float (&acc)[FILM_ROWS * FILM_GOBS], int lane) {
  const bool up = (lane & X) != 0;
#pragma unroll
  for (int i = 0; i < H; ++i) {
    const float keep = up ? acc[i + H] : acc[i];
    const float send = up ? acc[i] : acc[i + H];
    acc[i] = keep + __shfl_xor(send, X, 64);
  }
}

__global__ __launch_bounds__(FILM_THREADS, 4) void film_vectors_kernel(const ovla_film_linear* __restrict__ table, int n_linears, int total_items,
                                                                    const bf16_bits* __restrict__ avg, int64_t ld_avg, const int32_t* __restrict__ obs_slot,
                                                                    int n_obs, int n, int D, int gmax) {
  extern __shared__ __attribute__((aligned(16))) char film_smem[];
  int* s_slot = reinterpret_cast<int*>(film_smem);          // [64]
  int* s_idx = s_slot + OVLA_FILM_MAX_OBS;                    // [FILM_GOBS]
  int* s_ctl = s_idx + FILM_GOBS;                             // count, next scan position
  u32x4* s_avg = reinterpret_cast<u32x4*>(film_smem + FILM_HEAD_BYTES);   // [gmax][D / 8]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nvec = D >> 3, nfull = nvec >> 6, rem = nvec & 63;

  if (tid < n_obs) s_slot[tid] = clamp_slot(obs_slot[tid], n);
  __syncthreads();

  for (int s = 0; s < n; ++s) {
    for (int b0 = 0; b0 < n_obs;) {
      if (tid == 0) {   // the next (at most gmax) observations routed to s, in ascending order
        int cnt = 0, b = b0;
        for (; b < n_obs && cnt < gmax; ++b)
          if (s_slot[b] == s) s_idx[cnt++] = b;
        s_ctl[0] = cnt;
        s_ctl[1] = b;
      }
      __syncthreads();
      const int cnt = __builtin_amdgcn_readfirstlane(s_ctl[0]);
      b0 = __builtin_amdgcn_readfirstlane(s_ctl[1]);
      if (cnt == 0) {   // (b0 == n_obs now: the scan ran to the end) nothing of slot s is read
        __syncthreads();
        break;
      }
      for (int i = tid; i < cnt * nvec; i += FILM_THREADS) {
        const int g = i / nvec, v = i - g * nvec;
        s_avg[g * nvec + v] = *reinterpret_cast<const u32x4*>(avg + (int64_t)s_idx[g] * ld_avg + (int64_t)v * 8);
      }
      __syncthreads();

      for (int64_t item = (int64_t)blockIdx.x * FILM_WAVES + wave; item < total_items; item += (int64_t)gridDim.x * FILM_WAVES) {
        int lo = 0, hi = n_linears - 1;
        while (lo < hi) {   // the LAST linear whose first item is <= item
          const int mid = (lo + hi + 1) >> 1;
          if (table[mid].item_start <= item) lo = mid; else hi = mid - 1;
        }
        const ovla_film_linear e = table[lo];
        const int c0 = ((int)item - e.item_start) * FILM_ROWS;
        if (c0 < 0 || c0 >= e.out_f) continue;   // a table that does not match its prefix sums writes nothing
        const OVLA_GLOBAL u32x4* wp[FILM_ROWS];
#pragma unroll
        for (int r = 0; r < FILM_ROWS; ++r) {   // columns past out_f re-read the last row; their sums are dropped below
          const int c = c0 + r < e.out_f ? c0 + r : e.out_f - 1;
          wp[r] = (const OVLA_GLOBAL u32x4*)((const bf16_bits*)e.W + ((int64_t)s * e.out_f + c) * D) + lane;
        }
        float acc[FILM_ROWS * FILM_GOBS];
#pragma unroll
        for (int i = 0; i < FILM_ROWS * FILM_GOBS; ++i) acc[i] = 0.f;
        int it = 0;
        for (; it + 2 <= nfull; it += 2) {   // 8 loads in flight per lane before the first use
          u32x4 w0[FILM_ROWS], w1[FILM_ROWS];
#pragma unroll
          for (int r = 0; r < FILM_ROWS; ++r) w0[r] = wp[r][it * 64];
#pragma unroll
          for (int r = 0; r < FILM_ROWS; ++r) w1[r] = wp[r][(it + 1) * 64];
          mac_vec(acc, w0, s_avg + it * 64 + lane, nvec, cnt);
          mac_vec(acc, w1, s_avg + (it + 1) * 64 + lane, nvec, cnt);
        }
        if (it < nfull) {
          u32x4 w0[FILM_ROWS];
#pragma unroll
          for (int r = 0; r < FILM_ROWS; ++r) w0[r] = wp[r][it * 64];
          mac_vec(acc, w0, s_avg + it * 64 + lane, nvec, cnt);
        }
        if (lane < rem) {   // D / 8 is no multiple of 64: the first `rem` lanes own one more vector
          u32x4 w0[FILM_ROWS];
#pragma unroll
          for (int r = 0; r < FILM_ROWS; ++r) w0[r] = wp[r][nfull * 64];
          mac_vec(acc, w0, s_avg + nfull * 64 + lane, nvec, cnt);
        }
        // 32 sums over 64 lanes by halving exchange: at lane distance x a lane keeps half of its values and hands the other half to its partner,
        // so each value's 64 addends meet in the same tree of pairs; lane l ends with value (l >> 1) & 31 (both lanes of a pair hold it).
        exchange<16, 32>(acc, lane);
        exchange<8, 16>(acc, lane);
        exchange<4, 8>(acc, lane);
        exchange<2, 4>(acc, lane);
        exchange<1, 2>(acc, lane);
        const float sum = acc[0] + __shfl_xor(acc[0], 1, 64);
        const int idx = lane >> 1, r = idx / FILM_GOBS, g = idx % FILM_GOBS;
        if (!(lane & 1) && g < cnt && c0 + r < e.out_f) {
          const float bias = bf2f(((const bf16_bits*)e.bias)[(int64_t)s * e.out_f + c0 + r]);
          ((bf16_bits*)e.out)[(int64_t)s_idx[g] * e.out_f + c0 + r] = f2bf(bias + sum);
        }
      }
      __syncthreads();   // every wave is done with s_avg / s_idx before the next group is staged
    }
  }
}
}  // namespace

extern "C" int ovla_film_vectors(const ovla_film_vectors_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->table && a->table_host && a->avg && a->obs_slot, "ovla_film_vectors: null pointer (table, table_host, avg, obs_slot)");
  OVLA_REQUIRE(a->n_linears > 0, "ovla_film_vectors: n_linears = %d", a->n_linears);
  OVLA_REQUIRE(a->D > 0 && a->D % 8 == 0, "ovla_film_vectors: D = %d must be a positive multiple of 8", a->D);
  OVLA_REQUIRE(a->n >= 1 && a->n <= OVLA_MAX_SLOTS, "ovla_film_vectors: n = %d slots (1 .. %d)", a->n, OVLA_MAX_SLOTS);
  OVLA_REQUIRE(a->n_obs >= 1 && a->n_obs <= OVLA_FILM_MAX_OBS, "ovla_film_vectors: n_obs = %d observations (1 .. %d)", a->n_obs, OVLA_FILM_MAX_OBS);
  OVLA_REQUIRE(aligned16(a->avg) && a->ld_avg % 8 == 0 && a->ld_avg >= a->D, "ovla_film_vectors: avg needs a 16-byte base and ld_avg = %lld a multiple of 8, >= D = %d",
               (long long)a->ld_avg, a->D);
  OVLA_REQUIRE((((uintptr_t)a->obs_slot) & 3) == 0, "ovla_film_vectors: misaligned obs_slot");
  const int gmax_fit = (int)((FILM_LDS_MAX - FILM_HEAD_BYTES) / ((int64_t)a->D * 2));
  OVLA_REQUIRE(gmax_fit >= 1, "ovla_film_vectors: D = %d: one avg row does not fit in LDS", a->D);
  const ovla_film_linear* t = (const ovla_film_linear*)a->table_host;
  int64_t items = 0;
  for (int j = 0; j < a->n_linears; ++j) {
    OVLA_REQUIRE(t[j].W && t[j].bias && t[j].out, "ovla_film_vectors: linear %d has a null pointer (W, bias, out)", j);
    OVLA_REQUIRE(t[j].out_f >= 1, "ovla_film_vectors: linear %d has out_f = %d", j, t[j].out_f);
    OVLA_REQUIRE(aligned16(t[j].W) && ((((uintptr_t)t[j].bias) | ((uintptr_t)t[j].out)) & 1) == 0,
                 "ovla_film_vectors: linear %d: W needs a 16-byte base, bias and out 2-byte ones", j);
    OVLA_REQUIRE(t[j].item_start == items, "ovla_film_vectors: linear %d has item_start = %d, the prefix sum of ceil(out_f / %d) is %lld", j, t[j].item_start,
                 FILM_ROWS, (long long)items);
    items += (t[j].out_f + FILM_ROWS - 1) / FILM_ROWS;
    OVLA_REQUIRE(items <= 0x7fffffffLL, "ovla_film_vectors: more than 2^31 - 1 items");
  }
  if (int rc = check_host_slots(a->obs_slot_host, a->n_obs, a->n, "ovla_film_vectors")) return rc;
  const int gmax = gmax_fit < FILM_GOBS ? gmax_fit : FILM_GOBS;
  const int gneed = a->n_obs < gmax ? a->n_obs : gmax;
  const size_t lds = FILM_HEAD_BYTES + (size_t)gneed * a->D * 2;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)film_vectors_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FILM_LDS_MAX);
    attr_set = true;
  }
  const int wg_items = cdiv(items, FILM_WAVES);
  const int grid = wg_items < FILM_MAX_GRID ? wg_items : FILM_MAX_GRID;
  hipLaunchKernelGGL(film_vectors_kernel, dim3(grid), dim3(FILM_THREADS), lds, stream, (const ovla_film_linear*)a->table, a->n_linears, (int)items,
                     (const bf16_bits*)a->avg, a->ld_avg, a->obs_slot, a->n_obs, a->n, a->D, gneed);
  OVLA_CHECK_LAUNCH("ovla_film_vectors");
  return OVLA_OK;
}
