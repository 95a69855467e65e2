// tensor_stats.hip -- per-tensor gradient and parameter statistics of one flat trainable buffer (the reference reports such numbers through
// W&B; torch would need two tiny launches and a host synchronise per tensor).  The contract is in ovla.h "Per-tensor statistics"; the numpy
// restatement is tests/tensor_stats_reference.py.  A segmented form of ovla_grad_sumsq (grad_clip.hip), with which it shares the element and
// THE TREE (sumsq_order.h):
//   ovla_tensor_stats_plan   host only: checks the segment table and writes the prefix sums of the segments' chunk counts.
//   ovla_tensor_stats        two launches: one workgroup per chunk -> a 32-byte partial (both double sums, the finite absmax, the non-finite
//                            count), then one workgroup per segment over its partials -> out[t].  Reads 4 bytes of gradient and 2 or 4 of
//                            parameter per element.
// No atomics, no grid barrier, no spin-wait; nothing is read back.
#pragma clang fp contract(off)
#include <math.h>
#include <mutex>
#include <utility>
#include <vector>
#include "sumsq_order.h"

namespace {
using namespace sumsq_order;

static_assert(sizeof(ovla_tensor_stat) == OVLA_TENSOR_STATS_PARTIAL_BYTES && sizeof(ovla_tensor_seg) == 16, "the partials are ovla_tensor_stat records");

struct LaneStats {
  double g = 0.0, p = 0.0;
  float amax = 0.f;
  int bad = 0;   // per lane and chunk: at most kChunk / kLanes
};

template <bool BF>
OVLA_DEV void take_grad(float x, float scale, LaneStats& a) {
  const float r = seen<BF>(x, scale);
  const double d = (double)r;
  a.g += d * d;
  const float m = fabsf(r);
  if (m < INFINITY) a.amax = fmaxf(a.amax, m);   // NaN fails the comparison too
  else a.bad += 1;
}

OVLA_DEV void take_param(float w, LaneStats& a) {
  const double d = (double)w;
  a.p += d * d;
}

// four consecutive parameters: 8 bytes of bf16 (widened exactly) or 16 bytes of fp32
template <bool PBF> struct ParamGroup;
template <> struct ParamGroup<true> {
  typedef bf16x4_bits vec;
  typedef bf16_bits elem;
  static OVLA_DEV float at(const vec& v, int j) { return bf2f((bf16_bits)v[j]); }
  static OVLA_DEV float one(elem e) { return bf2f(e); }
};
template <> struct ParamGroup<false> {
  typedef f32x4 vec;
  typedef float elem;
  static OVLA_DEV float at(const vec& v, int j) { return v[j]; }
  static OVLA_DEV float one(elem e) { return e; }
};

template <bool BF, bool PBF>
__global__ __launch_bounds__(kLanes) void stats_chunk_kernel(const float* __restrict__ grad, const void* __restrict__ param, float scale,
                                                             const ovla_tensor_seg* __restrict__ segs, const int32_t* __restrict__ chunk_start, int n_segs,
                                                             ovla_tensor_stat* __restrict__ partials) {
  typedef ParamGroup<PBF> PG;
  __shared__ double wave_g[4], wave_p[4];
  __shared__ float wave_amax[4];
  __shared__ int wave_bad[4];
  const int t = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= chunk_start[n_segs]) return;                        // (the grid is the plan's total: uniform, never taken with the plan's table)
  int lo = 0, hi = n_segs;                                     // chunk_start[lo] <= b < chunk_start[hi]; an empty segment is never the answer
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (chunk_start[mid] <= b) lo = mid; else hi = mid;
  }
  const ovla_tensor_seg seg = segs[lo];
  const int64_t in_seg = (int64_t)(b - chunk_start[lo]) * kChunk;   // the chunks are counted from the segment's own start
  const int64_t c0 = seg.offset + in_seg, left = seg.n - in_seg;
  const int len = left < kChunk ? (int)left : kChunk;
  const f32x4* gv = reinterpret_cast<const f32x4*>(grad + c0);      // 16-byte aligned: grad is, offset % 8 == 0 and in_seg % 4 == 0
  const typename PG::elem* pe = reinterpret_cast<const typename PG::elem*>(param) + c0;
  const typename PG::vec* pv = reinterpret_cast<const typename PG::vec*>(pe);
  LaneStats a;
  if (len == kChunk) {                                         // every load of the chunk in flight before the first add
    f32x4 x[kTrips];
    typename PG::vec y[kTrips];
#pragma unroll
    for (int k = 0; k < kTrips; ++k) x[k] = gv[k * kLanes + t];
#pragma unroll
    for (int k = 0; k < kTrips; ++k) y[k] = pv[k * kLanes + t];
#pragma unroll
    for (int k = 0; k < kTrips; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) take_grad<BF>(x[k][j], scale, a);
    }
#pragma unroll
    for (int k = 0; k < kTrips; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) take_param(PG::at(y[k], j), a);
    }
  } else {                                                     // a segment's last chunk: the same lanes, the same order, bounds checked
    const int groups = len >> 2, rest = len & 3;
    for (int k = 0; k < kTrips; ++k) {
      const int gi = k * kLanes + t;
      if (gi < groups) {
        const f32x4 x = gv[gi];
        const typename PG::vec y = pv[gi];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          take_grad<BF>(x[j], scale, a);
          take_param(PG::at(y, j), a);
        }
      } else if (gi == groups) {                               // the scalar tail: n % 4 elements, read one by one by the lane that owns their group
        for (int j = 0; j < rest; ++j) {
          take_grad<BF>(grad[c0 + 4 * (int64_t)gi + j], scale, a);
          take_param(PG::one(pe[4 * (int64_t)gi + j]), a);
        }
      }
    }
  }
  // the maximum and the count are exact in any order; the two double sums go through THE TREE
#pragma unroll
  for (int h = 32; h > 0; h >>= 1) {
    a.amax = fmaxf(a.amax, __shfl_down(a.amax, h, 64));
    a.bad += __shfl_down(a.bad, h, 64);
  }
  if ((t & 63) == 0) {
    wave_amax[t >> 6] = a.amax;
    wave_bad[t >> 6] = a.bad;
  }
  const double g_total = block_tree(a.g, wave_g);              // (its barrier publishes wave_amax and wave_bad as well)
  const double p_total = block_tree(a.p, wave_p);
  if (t == 0) {
    ovla_tensor_stat s;
    s.grad_sumsq = g_total;
    s.param_sumsq = p_total;
    s.grad_absmax = fmaxf(fmaxf(wave_amax[0], wave_amax[1]), fmaxf(wave_amax[2], wave_amax[3]));
    s.n_bad_steps = 0;
    s.n_nonfinite = (int64_t)wave_bad[0] + wave_bad[1] + wave_bad[2] + wave_bad[3];
    partials[b] = s;
  }
}

__global__ __launch_bounds__(kLanes) void stats_final_kernel(const ovla_tensor_stat* __restrict__ partials, const int32_t* __restrict__ chunk_start,
                                                             ovla_tensor_stat* __restrict__ out) {
  __shared__ double wave_g[4], wave_p[4];
  __shared__ float wave_amax[4];
  __shared__ long long wave_bad[4];
  const int t = threadIdx.x;
  const int first = chunk_start[blockIdx.x], n_partials = chunk_start[blockIdx.x + 1] - first;
  const ovla_tensor_stat* part = partials + first;
  double g = 0.0, p = 0.0;
  float amax = 0.f;
  long long bad = 0;
  int j = t;
  for (; j + 3 * kLanes < n_partials; j += 4 * kLanes) {       // four records in flight, added in the same ascending order
    ovla_tensor_stat x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = part[j + u * kLanes];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      g += x[u].grad_sumsq;
      p += x[u].param_sumsq;
      amax = fmaxf(amax, x[u].grad_absmax);
      bad += x[u].n_nonfinite;
    }
  }
  for (; j < n_partials; j += kLanes) {
    const ovla_tensor_stat x = part[j];
    g += x.grad_sumsq;
    p += x.param_sumsq;
    amax = fmaxf(amax, x.grad_absmax);
    bad += x.n_nonfinite;
  }
#pragma unroll
  for (int h = 32; h > 0; h >>= 1) {
    amax = fmaxf(amax, __shfl_down(amax, h, 64));
    bad += __shfl_down(bad, h, 64);
  }
  if ((t & 63) == 0) {
    wave_amax[t >> 6] = amax;
    wave_bad[t >> 6] = bad;
  }
  const double g_total = block_tree(g, wave_g);
  const double p_total = block_tree(p, wave_p);
  if (t == 0) {                                                // n_t == 0: no partials, an all-zero entry
    ovla_tensor_stat* o = out + blockIdx.x;
    const long long n_bad = wave_bad[0] + wave_bad[1] + wave_bad[2] + wave_bad[3];
    o->grad_sumsq = g_total;
    o->param_sumsq = p_total;
    o->grad_absmax = fmaxf(fmaxf(wave_amax[0], wave_amax[1]), fmaxf(wave_amax[2], wave_amax[3]));
    o->n_nonfinite = n_bad;
    if (n_bad > 0) o->n_bad_steps += 1;                        // the latch: the only field that is read
  }
}

// the (n_segs, total_chunks) pairs of the plans made in this process: what the launch can check of a table that lives in device memory
std::mutex g_plans_mutex;
std::vector<std::pair<int32_t, int32_t>> g_plans;

void remember_plan(int32_t n_segs, int32_t total) {
  std::lock_guard<std::mutex> lock(g_plans_mutex);
  for (const auto& p : g_plans)
    if (p.first == n_segs && p.second == total) return;
  g_plans.emplace_back(n_segs, total);
}

bool plan_known(int32_t n_segs, int32_t total) {
  std::lock_guard<std::mutex> lock(g_plans_mutex);
  for (const auto& p : g_plans)
    if (p.first == n_segs && p.second == total) return true;
  return false;
}

inline bool aligned_to(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }
}  // namespace

extern "C" int ovla_tensor_stats_plan(const ovla_tensor_seg* segs, int32_t n_segs, int64_t buffer_n, int32_t* chunk_start) {
  OVLA_REQUIRE(segs && chunk_start, "ovla_tensor_stats_plan: null pointer");
  OVLA_REQUIRE(n_segs >= 1 && buffer_n >= 0, "ovla_tensor_stats_plan: n_segs = %d, buffer_n = %lld", n_segs, (long long)buffer_n);
  int64_t total = 0, end = 0;   // `end`: one past the previous segment
  for (int32_t t = 0; t < n_segs; ++t) {
    const int64_t off = segs[t].offset, n = segs[t].n;
    OVLA_REQUIRE(off >= 0 && n >= 0, "ovla_tensor_stats_plan: segment %d has offset %lld, n %lld", t, (long long)off, (long long)n);
    OVLA_REQUIRE(off % 8 == 0, "ovla_tensor_stats_plan: segment %d: offset %lld is not a multiple of 8", t, (long long)off);
    OVLA_REQUIRE(off >= end, "ovla_tensor_stats_plan: segment %d at %lld starts before the end %lld of the one before it (ascending, no overlap)", t,
                 (long long)off, (long long)end);
    OVLA_REQUIRE(n <= buffer_n - off, "ovla_tensor_stats_plan: segment %d [%lld, +%lld) ends past the buffer's %lld elements", t, (long long)off,
                 (long long)n, (long long)buffer_n);
    end = off + n;
    total += (n + kChunk - 1) / kChunk;
    OVLA_REQUIRE(total <= 0x7fffffffLL, "ovla_tensor_stats_plan: more chunks than a grid covers at segment %d", t);
  }
  total = 0;                    // nothing is written on a refusal
  for (int32_t t = 0; t < n_segs; ++t) {
    chunk_start[t] = (int32_t)total;
    total += (segs[t].n + kChunk - 1) / kChunk;
  }
  chunk_start[n_segs] = (int32_t)total;
  remember_plan(n_segs, (int32_t)total);
  return OVLA_OK;
}

extern "C" int ovla_tensor_stats(const ovla_tensor_stats_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->grad && a->param && a->segs && a->chunk_start && a->partials && a->out, "ovla_tensor_stats: null pointer");
  OVLA_REQUIRE(a->n_segs >= 1 && a->total_chunks >= 0, "ovla_tensor_stats: n_segs = %d, total_chunks = %d", a->n_segs, a->total_chunks);
  OVLA_REQUIRE(aligned16(a->grad) && aligned16(a->param), "ovla_tensor_stats: grad and param must be 16-byte aligned");
  OVLA_REQUIRE(aligned_to(a->out, 8) && aligned_to(a->partials, 8) && aligned_to(a->segs, 8) && aligned_to(a->chunk_start, 4),
               "ovla_tensor_stats: out, partials and segs must be 8-byte aligned, chunk_start 4-byte aligned");
  OVLA_REQUIRE(a->partials_bytes >= (int64_t)OVLA_TENSOR_STATS_PARTIAL_BYTES * a->total_chunks, "ovla_tensor_stats: partials of %lld bytes, %lld needed",
               (long long)a->partials_bytes, (long long)OVLA_TENSOR_STATS_PARTIAL_BYTES * a->total_chunks);
  OVLA_REQUIRE(plan_known(a->n_segs, a->total_chunks), "ovla_tensor_stats: no ovla_tensor_stats_plan of this process gave %d chunks for %d segments",
               a->total_chunks, a->n_segs);
  ovla_tensor_stat* partials = (ovla_tensor_stat*)a->partials;
  if (a->total_chunks > 0) {
    const dim3 grid((unsigned)a->total_chunks), block(kLanes);
#define OVLA_STATS_LAUNCH(BF, PBF) \
  hipLaunchKernelGGL((stats_chunk_kernel<BF, PBF>), grid, block, 0, stream, a->grad, a->param, a->grad_scale, a->segs, a->chunk_start, a->n_segs, partials)
    if (a->grad_round_bf16) {
      if (a->param_is_bf16) OVLA_STATS_LAUNCH(true, true); else OVLA_STATS_LAUNCH(true, false);
    } else {
      if (a->param_is_bf16) OVLA_STATS_LAUNCH(false, true); else OVLA_STATS_LAUNCH(false, false);
    }
#undef OVLA_STATS_LAUNCH
    OVLA_CHECK_LAUNCH("ovla_tensor_stats");
  }
  hipLaunchKernelGGL(stats_final_kernel, dim3((unsigned)a->n_segs), dim3(kLanes), 0, stream, (const ovla_tensor_stat*)partials, a->chunk_start, a->out);
  OVLA_CHECK_LAUNCH("ovla_tensor_stats");
  return OVLA_OK;
}
