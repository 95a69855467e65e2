// lora_route.hip -- device-side routing for multi-adapter serving: n LoRA adapters ("slots") ride in ONE K-extended GEMM launch, each row of the
// batch keeps the projection of its own observation's adapter and gets exact zeros for every other one (ovla_lora_route); the per-policy action
// head / proprio-projector outputs are picked per observation (ovla_select_by_slot).  The observation -> slot assignment is a device int32
// array, so a captured graph serves any assignment.  Both kernels clamp whatever they read from it: no index they form leaves the buffers.
#include "common.h"

namespace {

// One thread per 16-byte vector (8 bf16 columns) of the routed width G*n*r; r % 8 == 0, so a vector lies inside one slot's column block.
// Foreign vectors are OVERWRITTEN with +0 (never multiplied: a NaN / Inf of another adapter's projection must not reach the row); the row's
// own vectors and the columns >= G*n*r are not touched.
__global__ __launch_bounds__(256) void lora_route_kernel(bf16_bits* __restrict__ t, int64_t ld, const int32_t* __restrict__ obs_slot, int M, int nvec,
                                                         int n, int r, int rows_per_obs, int n_obs) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)M * nvec) return;
  const int m = (int)(idx / nvec), v = (int)(idx - (int64_t)m * nvec);
  int obs = m / rows_per_obs;
  obs = obs >= n_obs ? n_obs - 1 : obs;
  const int own = clamp_slot(obs_slot[obs], n);
  const int col = v * 8;
  if ((col / r) % n == own) return;
  *reinterpret_cast<uint4*>(t + (int64_t)m * ld + col) = make_uint4(0u, 0u, 0u, 0u);
}

// dst[m, :] = src[slot(m), m, :] in units of U bytes (the widest of 16 / 4 / 2 that the row size and the alignments allow).
template <typename U>
__global__ __launch_bounds__(256) void select_by_slot_kernel(const U* __restrict__ src, U* __restrict__ dst, const int32_t* __restrict__ obs_slot, int rows,
                                                             int units, int64_t slot_stride, int n, int rows_per_obs, int n_obs) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)rows * units) return;
  const int m = (int)(idx / units);
  int obs = m / rows_per_obs;
  obs = obs >= n_obs ? n_obs - 1 : obs;
  const int s = clamp_slot(obs_slot[obs], n);
  dst[idx] = src[(int64_t)s * slot_stride + idx];
}

}  // namespace

extern "C" int ovla_lora_route(const ovla_lora_route_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->t && a->obs_slot, "ovla_lora_route: null pointer");
  OVLA_REQUIRE(a->M > 0 && a->G > 0 && a->n > 0 && a->r > 0 && a->rows_per_obs > 0 && a->n_obs > 0, "ovla_lora_route: M=%d G=%d n=%d r=%d rows_per_obs=%d n_obs=%d",
               a->M, a->G, a->n, a->r, a->rows_per_obs, a->n_obs);
  const int64_t width = (int64_t)a->G * a->n * a->r;
  OVLA_REQUIRE(a->r % 8 == 0 && a->ld % 8 == 0 && a->ld >= width && aligned16(a->t), "ovla_lora_route: r=%d ld=%lld width=%lld (r %% 8, ld %% 8, ld >= G*n*r, 16-byte base)",
               a->r, (long long)a->ld, (long long)width);
  OVLA_REQUIRE((int64_t)a->n_obs * a->rows_per_obs >= a->M, "ovla_lora_route: %d rows but obs_slot covers %d observations of %d rows", a->M, a->n_obs, a->rows_per_obs);
  if (int rc = check_host_slots(a->obs_slot_host, a->n_obs, a->n, "ovla_lora_route")) return rc;
  if (a->n == 1) return OVLA_OK;   // one slot owns every column: nothing to zero
  const int nvec = (int)(width / 8);
  const int64_t total = (int64_t)a->M * nvec;
  OVLA_REQUIRE((total + 255) / 256 <= 0x7fffffffLL, "ovla_lora_route: %lld vectors need more than 2^31 - 1 workgroups", (long long)total);
  hipLaunchKernelGGL(lora_route_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, (bf16_bits*)a->t, a->ld, a->obs_slot, a->M, nvec, a->n, a->r,
                     a->rows_per_obs, a->n_obs);
  OVLA_CHECK_LAUNCH("ovla_lora_route");
  return OVLA_OK;
}

extern "C" int ovla_select_by_slot(const ovla_select_by_slot_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(a && a->src && a->dst && a->obs_slot, "ovla_select_by_slot: null pointer");
  OVLA_REQUIRE(a->n > 0 && a->rows > 0 && a->dim > 0 && a->rows_per_obs > 0 && a->n_obs > 0 && (a->elem_bytes == 2 || a->elem_bytes == 4),
               "ovla_select_by_slot: n=%d rows=%d dim=%d rows_per_obs=%d n_obs=%d elem_bytes=%d", a->n, a->rows, a->dim, a->rows_per_obs, a->n_obs, a->elem_bytes);
  const int64_t slot_stride = a->src_slot_stride ? a->src_slot_stride : (int64_t)a->rows * a->dim;   // elements
  OVLA_REQUIRE(slot_stride >= (int64_t)a->rows * a->dim, "ovla_select_by_slot: src_slot_stride %lld < rows * dim", (long long)slot_stride);
  OVLA_REQUIRE((int64_t)a->n_obs * a->rows_per_obs >= a->rows, "ovla_select_by_slot: %d rows but obs_slot covers %d observations of %d rows", a->rows, a->n_obs,
               a->rows_per_obs);
  OVLA_REQUIRE((((uintptr_t)a->src | (uintptr_t)a->dst) & (uintptr_t)(a->elem_bytes - 1)) == 0, "ovla_select_by_slot: misaligned pointers");
  if (int rc = check_host_slots(a->obs_slot_host, a->n_obs, a->n, "ovla_select_by_slot")) return rc;
  const int64_t row_bytes = (int64_t)a->dim * a->elem_bytes, stride_bytes = slot_stride * a->elem_bytes;
  const int unit = (row_bytes % 16 == 0 && stride_bytes % 16 == 0 && aligned16(a->src) && aligned16(a->dst)) ? 16 : a->elem_bytes;
  const int units = (int)(row_bytes / unit);
  const int64_t total = (int64_t)a->rows * units;
  const dim3 grid(cdiv(total, 256)), block(256);
  if (unit == 16)
    hipLaunchKernelGGL(select_by_slot_kernel<uint4>, grid, block, 0, stream, (const uint4*)a->src, (uint4*)a->dst, a->obs_slot, a->rows, units, stride_bytes / 16, a->n,
                       a->rows_per_obs, a->n_obs);
  else if (unit == 4)
    hipLaunchKernelGGL(select_by_slot_kernel<uint32_t>, grid, block, 0, stream, (const uint32_t*)a->src, (uint32_t*)a->dst, a->obs_slot, a->rows, units, slot_stride,
                       a->n, a->rows_per_obs, a->n_obs);
  else
    hipLaunchKernelGGL(select_by_slot_kernel<uint16_t>, grid, block, 0, stream, (const uint16_t*)a->src, (uint16_t*)a->dst, a->obs_slot, a->rows, units, slot_stride,
                       a->n, a->rows_per_obs, a->n_obs);
  OVLA_CHECK_LAUNCH("ovla_select_by_slot");
  return OVLA_OK;
}
