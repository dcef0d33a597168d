// fdoct_boxtile.h -- what the stages with a rectangular window over an image batch share (fdoct_doppler.hip, fdoct_angio.hip): the
// tile and its launch arithmetic as host functions, and on the device the tile's indices, the window pass and the bulk sum.  A
// stage's own file keeps its staging, its epilogue and its row decode.  Internal.  DESIGN 3.4m has the argument; in short:
//   tile    one workgroup of 256 threads takes 16 rows x 64 depth bins of output of one image at a time and loops over tiles (the
//           grid is capped, fdoct_grid.h).  It is staged in LDS with its halo, sr x sw = (16 + wa - 1) x (64 + wd - 1) floats a
//           plane, (wa - 1) / 2 rows and (wd - 1) / 2 depths of it in front; pixels outside the image are zeros, which change no sum.
//   window  depth sums in increasing depth, then row sums down the column in increasing row; a wave's 64 lanes lie along depth in
//           both, so every LDS access of a wave is 64 consecutive words: no padding, no swizzle.
//   bulk    one workgroup per row: a strided partial of X2 conj(X1) per thread, then a tree in LDS; no atomics.
// Every sum starts at 0.f and its order depends on the window and the indices only: a tile gives the same bits wherever it runs.
#pragma once
#include <hip/hip_runtime.h>

#include "fdoct_grid.h"

namespace fdoct {

constexpr int kBoxRows = 16;          // one workgroup's tile: 16 rows x 64 depth bins of output, 256 threads
constexpr int kBoxDepths = 64;        // (one wave's 64 lanes lie along depth in every pass)
constexpr int kBoxBlock = 256;
constexpr int kBoxOwn = kBoxRows * kBoxDepths / kBoxBlock;   // output pixels a thread owns: 4
constexpr int kBoxWavesPerCu = 16;    // the grids' cap: four workgroups a CU (Doppler's 4 x 8 tile is 31 KiB of LDS, angiography's 16 x 16 tile 35 KiB)
constexpr int kBoxBulkBlock = 256;    // the bulk sums: one workgroup per row

constexpr int box_staged_rows(int wa) { return kBoxRows + wa - 1; }
constexpr int box_staged_depths(int wd) { return kBoxDepths + wd - 1; }

// `planes` planes of floats of the staged halo tile, and as many of the depth-summed rows behind them.
inline unsigned box_lds_bytes(int planes, int wa, int wd) {
  const unsigned sr = box_staged_rows(wa), sw = box_staged_depths(wd);
  return (sr * sw + sr * kBoxDepths) * (unsigned)planes * (unsigned)sizeof(float);
}

// The launch fields of an argument block (DopplerArgs, AngioArgs) from its depths, wa, wd and use_bulk: the tiles of `images` images
// of `rows` rows, the LDS of `planes` planes, and both grids capped -- the bulk kernel's over `bulk_rows` rows.  Nothing is enqueued.
template <class Args>
void box_plan_launch(Args* a, int planes, int images, int rows, long long bulk_rows, int num_cu) {
  a->tiles_r = (rows + kBoxRows - 1) / kBoxRows;
  a->tiles_d = (a->depths + kBoxDepths - 1) / kBoxDepths;
  a->tiles = (long long)images * a->tiles_r * a->tiles_d;
  a->lds_bytes = box_lds_bytes(planes, a->wa, a->wd);
  const long long cap = resident_blocks(num_cu, kBoxWavesPerCu, kBoxBlock);
  a->blocks = (int)(a->tiles < cap ? a->tiles : cap);
  const long long bulk_cap = resident_blocks(num_cu, kBoxWavesPerCu, kBoxBulkBlock);
  a->bulk_blocks = a->use_bulk ? (int)(bulk_rows < bulk_cap ? bulk_rows : bulk_cap) : 0;
}

// Tile `tile` of the grid's loop: its image, its place among the image's tiles, and the staged tile's first row and depth.
struct BoxTile {
  int image, tr, td, row0, dep0;
};
__device__ __forceinline__ BoxTile box_tile(long long tile, int tiles_r, int tiles_d, int wa, int wd) {
  const long long per_image = (long long)tiles_r * tiles_d;
  BoxTile t;
  t.image = (int)(tile / per_image);
  const int i = (int)(tile - (long long)t.image * per_image);
  t.tr = i / tiles_d, t.td = i - t.tr * tiles_d;
  t.row0 = t.tr * kBoxRows - (wa - 1) / 2, t.dep0 = t.td * kBoxDepths - (wd - 1) / 2;
  return t;
}

// Staged pixel i of the tile (row-major, sw a row): its row and depth in the image; false outside the image.
__device__ __forceinline__ bool box_staged(const BoxTile& t, int i, int sw, int rows, int depths, int* r, int* b) {
  const int lr = i / sw, lc = i - lr * sw;
  *r = t.row0 + lr, *b = t.dep0 + lc;
  return *r >= 0 && *r < rows && *b >= 0 && *b < depths;
}

// Output pixel j (0..3) of the thread: its row and depth in the image; false beyond the image's edge.
__device__ __forceinline__ bool box_owned(const BoxTile& t, int j, int rows, int depths, int* r, int* b) {
  *r = t.tr * kBoxRows + ((int)threadIdx.x >> 6) + (kBoxBlock / 64) * j, *b = t.td * kBoxDepths + ((int)threadIdx.x & 63);
  return *r < rows && *b < depths;
}

// The pixels the window at (r, b) shares with the image, counted from the indices.
__device__ __forceinline__ int box_terms(int r, int b, int rows, int depths, int wa, int wd) {
  const int r_lo = max(r - (wa - 1) / 2, 0), r_hi = min(r + wa / 2, rows - 1);
  const int b_lo = max(b - (wd - 1) / 2, 0), b_hi = min(b + wd / 2, depths - 1);
  return (r_hi - r_lo + 1) * (b_hi - b_lo + 1);
}

// The box sums of the first `live` (1..P) of P staged planes at the thread's four output pixels: o[p][j]; planes past `live` give
// zeros.  s is the first staged plane, the others sr * sw floats apart; d the first plane of depth sums, sr * 64 apart.  Barriers
// in front (the planes are written), between the phases and behind (the planes are the next pass's).
template <int P>
__device__ __forceinline__ void box_window(const float* s, float* d, int sr, int sw, int wa, int wd, int live, float (&o)[P][kBoxOwn]) {
  const int ns = sr * sw, nd = sr * kBoxDepths;
  __syncthreads();
  for (int i = threadIdx.x; i < nd; i += kBoxBlock) {
    const int at = (i >> 6) * sw + (i & 63);
    float sum[P] = {};
    for (int j = 0; j < wd; j++) {
#pragma unroll
      for (int p = 0; p < P; p++)
        if (p == 0 || p < live) sum[p] += s[p * ns + at + j];
    }
#pragma unroll
    for (int p = 0; p < P; p++)
      if (p == 0 || p < live) d[p * nd + i] = sum[p];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kBoxOwn; j++) {
    const int at = (((int)threadIdx.x >> 6) + (kBoxBlock / 64) * j) * kBoxDepths + ((int)threadIdx.x & 63);
    float sum[P] = {};
    for (int w = 0; w < wa; w++) {
#pragma unroll
      for (int p = 0; p < P; p++)
        if (p == 0 || p < live) sum[p] += d[p * nd + at + w * kBoxDepths];
    }
#pragma unroll
    for (int p = 0; p < P; p++) o[p][j] = sum[p];
  }
  __syncthreads();
}

// The workgroup's sum B of x2[b] conj(x1[b]) over b < count, on every thread: a strided partial per thread, the tree in `part`, and
// the barrier behind it (part is the next row's).
__device__ __forceinline__ float2 box_bulk_sum(const float2* x1, const float2* x2, int count, float2 (&part)[kBoxBulkBlock]) {
  float2 s = make_float2(0.f, 0.f);
  for (int b = threadIdx.x; b < count; b += kBoxBulkBlock) {
    const float2 u = x1[b], v = x2[b];
    s.x += v.x * u.x + v.y * u.y, s.y += v.y * u.x - v.x * u.y;
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int half = kBoxBulkBlock / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) {
      const float2 o = part[threadIdx.x + half];
      part[threadIdx.x].x += o.x, part[threadIdx.x].y += o.y;
    }
    __syncthreads();
  }
  const float2 B = part[0];
  __syncthreads();
  return B;
}

// B / |B|, or with `conj` its conjugate; 1 where B is 0.
__device__ __forceinline__ float2 box_phasor(float2 B, bool conj) {
  const float m = hypotf(B.x, B.y);
  return m > 0.f ? make_float2(B.x / m, conj ? -(B.y / m) : B.y / m) : make_float2(1.f, 0.f);
}

}  // namespace fdoct
