// token_row.h -- the row reductions of the token kernels, shared by ovla_token_ce (head_optim.hip) and by ovla_sample_tokens / ovla_token_pg
// (token_sample.hip): the maximum and the lowest index of it, the sum of exponentials in its fixed order, the log-sum-exp and the softmax
// gradient element.  One workgroup of 256 lanes owns a row and walks the columns [lo, hi) with lane t taking lo + t, lo + t + 256, ...; the
// three kernels call these functions for everything between loading a value and storing a result, so a full window at temperature 1 gives
// ovla_token_ce's bits by construction (ovla.h "Token sampling and the policy-gradient objective").
// `value(j)` is the fp32 value of column j: the logit itself, or the logit times 1 / T.
#pragma once
#include "common.h"

namespace token_row {

struct Shared {   // LDS of one workgroup
  float red_f[4];
  int red_i[4];
  float bc_f[3];
  int bc_i;
};

// (maximum, lowest index of it) of one lane's candidates -> of the row, valid in every lane.  A row in which no value ever compared greater
// than -inf (all -inf, or only NaN) leaves mi >= hi and reports `lo`.
OVLA_DEV void block_first_max(float& m, int& mi, int lo, int hi, Shared& sh) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(m, off); const int oi = __shfl_xor(mi, off);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
  if (lane == 0) { sh.red_f[wave] = m; sh.red_i[wave] = mi; }
  __syncthreads();
  if (tid == 0) {
    float bm = sh.red_f[0]; int bi = sh.red_i[0];
    for (int w = 1; w < 4; ++w) if (sh.red_f[w] > bm || (sh.red_f[w] == bm && sh.red_i[w] < bi)) { bm = sh.red_f[w]; bi = sh.red_i[w]; }
    sh.bc_f[0] = bm; sh.bc_i = bi >= hi ? lo : bi;
  }
  __syncthreads();
  m = sh.bc_f[0]; mi = sh.bc_i;
}

template <class V>
OVLA_DEV void row_max(V value, int lo, int hi, Shared& sh, float& m, int& mi) {
  m = -INFINITY; mi = 0x7fffffff;
  for (int j = lo + (int)threadIdx.x; j < hi; j += 256) {
    const float v = value(j);
    if (v > m) { m = v; mi = j; }            // j ascends per lane: the first maximum wins
  }
  block_first_max(m, mi, lo, hi, sh);
}

// s = sum_j __expf(value(j) - m);  ENT: es = sum_j e_j value(j) over the terms with e_j > 0 (a -inf column has probability 0, not 0 * inf).
// Lane sums in column order, the wave butterfly, then (w0 + w1) + (w2 + w3).  Both valid in every lane.
template <bool ENT, class V>
OVLA_DEV void row_sumexp(V value, int lo, int hi, float m, Shared& sh, float& s, float& es) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  s = 0.0f; es = 0.0f;
  for (int j = lo + tid; j < hi; j += 256) {
    const float v = value(j);
    const float e = __expf(v - m);
    s += e;
    if (ENT) es += e > 0.0f ? e * v : 0.0f;
  }
  s = wave_sum(s);
  if (lane == 0) sh.red_f[wave] = s;
  __syncthreads();
  if (tid == 0) sh.bc_f[1] = (sh.red_f[0] + sh.red_f[1]) + (sh.red_f[2] + sh.red_f[3]);
  __syncthreads();
  s = sh.bc_f[1];
  if (ENT) {
    es = wave_sum(es);
    if (lane == 0) sh.red_f[wave] = es;
    __syncthreads();
    if (tid == 0) sh.bc_f[2] = (sh.red_f[0] + sh.red_f[1]) + (sh.red_f[2] + sh.red_f[3]);
    __syncthreads();
    es = sh.bc_f[2];
  }
}

OVLA_DEV float lse(float s, float m) { return __logf(s) + m; }

// (softmax_j - onehot_j) * c with e = __expf(value(j) - m) and inv = 1.0f / s: ONE explicit fma, then the multiply
OVLA_DEV float grad_elem(float e, float inv, float onehot, float c) { return __builtin_fmaf(e, inv, -onehot) * c; }

}  // namespace token_row
