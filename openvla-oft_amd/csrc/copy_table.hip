// copy_table.hip -- grouped, strided 2-D device-to-device copy driven by a device table (ovla_copy_table): the policy pool's slot swap.  One
// launch moves every tensor of one policy: lora_A row groups into A_slots, lora_B [out, r] into the 64-byte column block of B_slots' 256-byte
// rows, the flat parameter buffers of the head and the proprio projector.  Shaped like ovla_transpose_batched: workgroup b finds its entry by
// binary search over the exclusive prefix sums of the entries' tile counts.
//
// A tile is at most TILE bytes of ONE entry: whole rows while a row fits (TILE / row_bytes of them), otherwise TILE-byte pieces of one row.
// Within a tile the units (16 bytes on the vector path, 2 on the element path) are numbered row-major and unit i goes to thread i % 256: a
// wave instruction covers 1 KiB of a long row, or -- rows of 64 bytes -- the whole segments of 16 consecutive rows (lane l: row l / 4, piece
// l % 4).  Every address a thread forms lies inside its tile's rectangle, and the tile's inside the entry's.
#include "common.h"

namespace {

constexpr int64_t TILE = 16384;   // bytes; a multiple of 16
constexpr int THREADS = 256;
constexpr int UNROLL = 4;         // loads in flight per thread before the first store

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
// the table's pointers are device-memory addresses: told so, the compiler emits global_load / global_store instead of flat accesses
#define OVLA_GLOBAL __attribute__((address_space(1)))

struct TileShape { int64_t rows_per_tile, pieces, tiles; };

// the one definition of the tiling, for the host plan and the kernel
__host__ __device__ inline TileShape tile_shape(int64_t rows, int64_t row_bytes) {
  TileShape t;
  if (rows <= 0 || row_bytes <= 0) { t.rows_per_tile = 1; t.pieces = 0; t.tiles = 0; return t; }
  if (row_bytes <= TILE) {
    t.rows_per_tile = TILE / row_bytes;
    t.pieces = 1;
    t.tiles = (rows + t.rows_per_tile - 1) / t.rows_per_tile;
  } else {
    t.rows_per_tile = 1;
    t.pieces = (row_bytes + TILE - 1) / TILE;
    t.tiles = rows * t.pieces;
  }
  return t;
}

// nrows rows of `upr` units of sizeof(T) bytes each; nrows * upr <= TILE / sizeof(T)
template <typename T>
OVLA_DEV void copy_tile(const OVLA_GLOBAL char* __restrict__ s, OVLA_GLOBAL char* __restrict__ d, int64_t sld, int64_t dld, uint32_t nrows, uint32_t upr) {
  const uint32_t total = nrows * upr;
  const uint32_t dq = THREADS / upr, dr = THREADS % upr;   // one step of THREADS units = dq rows and dr units
  uint32_t r = threadIdx.x / upr, c = threadIdx.x % upr;
  for (uint32_t i = threadIdx.x; i < total; i += UNROLL * THREADS) {
    T v[UNROLL];
    int64_t doff[UNROLL];
#pragma unroll
    for (int k = 0; k < UNROLL; ++k) {
      doff[k] = (int64_t)r * dld + (int64_t)c * (int64_t)sizeof(T);
      if (i + k * THREADS < total) v[k] = *(const OVLA_GLOBAL T*)(s + (int64_t)r * sld + (int64_t)c * (int64_t)sizeof(T));
      r += dq;
      c += dr;
      if (c >= upr) { c -= upr; ++r; }
    }
#pragma unroll
    for (int k = 0; k < UNROLL; ++k)
      if (i + k * THREADS < total) *(OVLA_GLOBAL T*)(d + doff[k]) = v[k];
  }
}

__global__ __launch_bounds__(THREADS) void copy_table_kernel(const ovla_copy_entry* __restrict__ table, const int32_t* __restrict__ tile_start, int n) {
  const int b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {   // the LAST entry whose first tile is <= b: entries without tiles (rows == 0) are never chosen
    const int mid = (lo + hi + 1) >> 1;
    if (tile_start[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const ovla_copy_entry e = table[lo];
  const int64_t t = b - tile_start[lo];
  const TileShape ts = tile_shape(e.rows, e.row_bytes);
  if (t < 0 || t >= ts.tiles) return;   // a table that does not match its prefix sums writes nothing
  int64_t row0, nrows, byte0, nbytes;
  if (ts.pieces == 1) {
    row0 = t * ts.rows_per_tile;
    nrows = e.rows - row0 < ts.rows_per_tile ? e.rows - row0 : ts.rows_per_tile;
    byte0 = 0;
    nbytes = e.row_bytes;
  } else {
    row0 = t / ts.pieces;
    nrows = 1;
    byte0 = (t - row0 * ts.pieces) * TILE;
    nbytes = e.row_bytes - byte0 < TILE ? e.row_bytes - byte0 : TILE;
  }
  const OVLA_GLOBAL char* s = (const OVLA_GLOBAL char*)e.src + row0 * e.src_ld_bytes + byte0;
  OVLA_GLOBAL char* d = (OVLA_GLOBAL char*)e.dst + row0 * e.dst_ld_bytes + byte0;
  const uint64_t all = (uint64_t)(uintptr_t)e.src | (uint64_t)(uintptr_t)e.dst | (uint64_t)e.src_ld_bytes | (uint64_t)e.dst_ld_bytes | (uint64_t)e.row_bytes;
  if ((all & 15) == 0)   // uniform over the entry (byte0 is a multiple of TILE)
    copy_tile<u32x4>(s, d, e.src_ld_bytes, e.dst_ld_bytes, (uint32_t)nrows, (uint32_t)(nbytes / 16));
  else
    copy_tile<unsigned short>(s, d, e.src_ld_bytes, e.dst_ld_bytes, (uint32_t)nrows, (uint32_t)(nbytes / 2));
}
}  // namespace

extern "C" int ovla_copy_table_plan(const ovla_copy_entry* entries, int32_t n, int32_t* tile_start) {
  OVLA_REQUIRE(entries && tile_start, "ovla_copy_table_plan: null pointer");
  OVLA_REQUIRE(n > 0, "ovla_copy_table_plan: n = %d entries", n);
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    const ovla_copy_entry& e = entries[i];
    tile_start[i] = (int32_t)total;
    OVLA_REQUIRE(e.rows >= 0, "ovla_copy_table_plan: entry %d has rows = %lld", i, (long long)e.rows);
    if (e.rows == 0) continue;
    OVLA_REQUIRE(e.src && e.dst, "ovla_copy_table_plan: entry %d has a null pointer", i);
    OVLA_REQUIRE(e.row_bytes > 0 && e.row_bytes % 2 == 0, "ovla_copy_table_plan: entry %d has row_bytes = %lld (positive multiples of 2 only)", i,
                 (long long)e.row_bytes);
    OVLA_REQUIRE(((((uintptr_t)e.src | (uintptr_t)e.dst) & 1) == 0) && e.src_ld_bytes % 2 == 0 && e.dst_ld_bytes % 2 == 0,
                 "ovla_copy_table_plan: entry %d: pointers and strides must be multiples of 2 bytes", i);
    OVLA_REQUIRE(e.rows == 1 || (e.src_ld_bytes >= e.row_bytes && e.dst_ld_bytes >= e.row_bytes),
                 "ovla_copy_table_plan: entry %d: strides %lld / %lld are below row_bytes = %lld", i, (long long)e.src_ld_bytes, (long long)e.dst_ld_bytes,
                 (long long)e.row_bytes);
    OVLA_REQUIRE(e.rows <= 0x7fffffffLL, "ovla_copy_table_plan: entry %d has %lld rows", i, (long long)e.rows);
    total += tile_shape(e.rows, e.row_bytes).tiles;
    OVLA_REQUIRE(total <= 0x7fffffffLL, "ovla_copy_table_plan: the table needs more than 2^31 - 1 tiles");
  }
  tile_start[n] = (int32_t)total;
  return OVLA_OK;
}

extern "C" int ovla_copy_table(const ovla_copy_entry* table, const int32_t* tile_start, int32_t n, int32_t total_tiles, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  OVLA_REQUIRE(table && tile_start, "ovla_copy_table: null pointer");
  OVLA_REQUIRE(n > 0 && total_tiles >= 0, "ovla_copy_table: n = %d entries, %d tiles", n, total_tiles);
  if (total_tiles == 0) return OVLA_OK;   // every entry has rows == 0
  hipLaunchKernelGGL(copy_table_kernel, dim3(total_tiles), dim3(THREADS), 0, stream, table, tile_start, n);
  OVLA_CHECK_LAUNCH("ovla_copy_table");
  return OVLA_OK;
}
