// sumsq_order.h -- the fixed order of the clip contract's double sums (ovla.h "Gradient-norm clipping"), shared by ovla_grad_sumsq
// (grad_clip.hip) and ovla_tensor_stats (tensor_stats.hip): the gradient element as AdamW sees it, squared in double, and THE TREE that
// pairs the lane sums of one workgroup.  Both files reduce a chunk and a run of partials with these functions, so a one-entry segment
// table gives ovla_grad_sumsq's bits by construction.  Include it under `#pragma clang fp contract(off)`.
#pragma once
#include "common.h"

namespace sumsq_order {

constexpr int kChunk = OVLA_GRAD_SUMSQ_CHUNK, kLanes = OVLA_GRAD_SUMSQ_LANES;
constexpr int kTrips = kChunk / (4 * kLanes);   // 16-byte loads per lane and full chunk
static_assert(kLanes == 256 && kChunk % (4 * kLanes) == 0, "the tree below pairs four waves of 64 lanes");

// r_i of the contract: one fp32 multiply, then the bf16 rounding of a bf16 parameter buffer
template <bool BF>
OVLA_DEV float seen(float g, float scale) {
  float r = g * scale;
  if (BF) r = bfround(r);
  return r;
}

template <bool BF>
OVLA_DEV double sq(float g, float scale) {
  const double d = (double)seen<BF>(g, scale);
  return d * d;   // exact: 24 x 24 significant bits
}

// THE TREE of the contract: within each wave h = 32 .. 1: s[t] += s[t + h] for t < h (lanes t >= h compute values nobody reads), then
// (w0 + w1) + (w2 + w3) over the four wave totals.  The result is valid in every lane.
OVLA_DEV double block_tree(double acc, double* wave_total /* LDS [4] */) {
#pragma unroll
  for (int h = 32; h > 0; h >>= 1) acc += __shfl_down(acc, h, 64);
  if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = acc;
  __syncthreads();
  return (wave_total[0] + wave_total[1]) + (wave_total[2] + wave_total[3]);
}

}  // namespace sumsq_order
