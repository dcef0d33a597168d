// fdoct_bscanbin.hip -- spinjnt's output binning (include/fdoct_bscanbin.h), BscanFFTspinjnt.cpp:1856-1861:
//   resize(bscan, bscanbinned, Size(), 1.0 / bscanbinx, 1.0 / bscanbiny, INTER_AREA);
//   resize(multiplyfactor * bscanbinned, bscan, Size(), bscanbinx * binvaluey, bscanbiny, INTER_CUBIC);
// and the log that follows (1869-1874, or 1894-1903 behind the J0 lock-in's difference), as ONE kernel: a workgroup owns a
// tile of the output, sums the input blocks under the binned cells that tile's cubic taps touch (halo included, indices clamped
// to the binned image: the replicate border) into a tile of doubles in LDS, and evaluates the separable cubic from there.  No
// binned image exists in HBM and the dB is not a second pass.
// Everything is carried in double and every sum runs in an order the geometry alone fixes (a cell: depth rows outermost, A-scans
// left to right; the cubic: along A-scans first, then along depths, each left to right), so reruns, both layouts and both
// memory spaces give the same bits.  The layout is a template parameter: lanes run along the contiguous dimension either
// way, and what changes with it is which of the two loops of a sum is the outer one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "fdoct_bscanbin_kernels.h"

namespace fdoct {

namespace {

constexpr int BIN_BLOCK = 256;
constexpr int BIN_WAVES_PER_CU = 16;
constexpr int BIN_TILE_R = 32;   // output rows (memory) of a tile: >= 5, so the tile that owns depth rows 0-1 holds row 4 as well
constexpr int BIN_TILE_C = 128;  // ... and columns: 32 lanes x 16 bytes

// (1849-1852: positivediff = max(bscan - jscan, 0) + 0.001 on CV_64F data)
template <bool JS>
__device__ __forceinline__ double bin_input(float b, float j) {
  if (!JS) return (double)b;
  const double d = (double)b - (double)j;
  return (d > 0.0 ? d : 0.0) + 0.001;
}

// acc[cell] += x without an indexed register array: `cell` is the same for every lane
__device__ __forceinline__ void bin_add(double (&acc)[4], int cell, double x) {
#pragma unroll
  for (int k = 0; k < 4; k++) acc[k] = (cell == k) ? acc[k] + x : acc[k];
}

__device__ __forceinline__ float f4_at(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// The sums of `group` cells that lie side by side along the contiguous dimension, cell row cr, from column c0 on (span floats:
// whole cells, a multiple of 4 in the 16-byte form).  TR: a cell's picture rows are memory rows (outer loop), else its picture
// rows are memory columns.
template <bool TR, bool JS>
__device__ __forceinline__ void bin_reduce(const BscanBinArgs& a, const float* __restrict__ img, int cr, int c0, int span,
                                           double (&acc)[4]) {
  const float* p = img + (long long)cr * a.binr * a.C + c0;
  const float* pj = JS ? a.jscan + (long long)cr * a.binr * a.C + c0 : nullptr;
  acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
  if (a.vec_in) {
    if (TR) {
      for (int r = 0; r < a.binr; r++) {
        int cell = 0, k = 0;
        for (int q = 0; q < span; q += 4) {
          const float4 v = *reinterpret_cast<const float4*>(p + (long long)r * a.C + q);
          float4 j = make_float4(0.f, 0.f, 0.f, 0.f);
          if (JS) j = *reinterpret_cast<const float4*>(pj + (long long)r * a.C + q);
#pragma unroll
          for (int e = 0; e < 4; e++) {
            bin_add(acc, cell, bin_input<JS>(f4_at(v, e), f4_at(j, e)));
            if (++k == a.binc) k = 0, cell++;
          }
        }
      }
    } else {
      int cell = 0, k = 0;
      for (int q = 0; q < span; q += 4) {
        float4 v[kBinMaxFactor], j[JS ? kBinMaxFactor : 1];
#pragma unroll
        for (int r = 0; r < kBinMaxFactor; r++)
          if (r < a.binr) {
            v[r] = *reinterpret_cast<const float4*>(p + (long long)r * a.C + q);
            if (JS) j[JS ? r : 0] = *reinterpret_cast<const float4*>(pj + (long long)r * a.C + q);
          }
#pragma unroll
        for (int e = 0; e < 4; e++) {
#pragma unroll
          for (int r = 0; r < kBinMaxFactor; r++)
            if (r < a.binr) bin_add(acc, cell, bin_input<JS>(f4_at(v[r], e), JS ? f4_at(j[JS ? r : 0], e) : 0.f));
          if (++k == a.binc) k = 0, cell++;
        }
      }
    }
  } else {  // element-wise: one cell per thread (group == 1, span == binc)
    double s = 0.0;
    if (TR) {
      for (int r = 0; r < a.binr; r++)
        for (int c = 0; c < a.binc; c++) s += bin_input<JS>(p[(long long)r * a.C + c], JS ? pj[(long long)r * a.C + c] : 0.f);
    } else {
      for (int c = 0; c < a.binc; c++)
        for (int r = 0; r < a.binr; r++) s += bin_input<JS>(p[(long long)r * a.C + c], JS ? pj[(long long)r * a.C + c] : 0.f);
    }
    acc[0] = s;
  }
}

struct BinTile {
  int kr_lo, kc_lo;  // first cell row / column the LDS tile holds
};

// INTER_CUBIC at output (orow, ocol) from the LDS tile: along A-scans first, then along depths, each sum left to right.
template <bool TR>
__device__ __forceinline__ double bin_cubic(const BscanBinArgs& a, const double* __restrict__ tr, const double* __restrict__ tc,
                                            const double* __restrict__ cells, const BinTile& t, int orow, int ocol) {
  const int kr = orow / a.upr, kc = ocol / a.upc;
  const double* wr = tr + kBinTapStride * (orow - kr * a.upr);
  const double* wc = tc + kBinTapStride * (ocol - kc * a.upc);
  const int sr = kr + (int)wr[4], sc = kc + (int)wc[4];
  int ri[4], ci[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    ri[i] = (min(max(sr + i, 0), a.NR - 1) - t.kr_lo) * a.lds_stride;
    ci[i] = min(max(sc + i, 0), a.NC - 1) - t.kc_lo;
  }
  double h[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (TR)
      h[j] = ((wc[0] * cells[ri[j] + ci[0]] + wc[1] * cells[ri[j] + ci[1]]) + wc[2] * cells[ri[j] + ci[2]]) + wc[3] * cells[ri[j] + ci[3]];
    else
      h[j] = ((wr[0] * cells[ri[0] + ci[j]] + wr[1] * cells[ri[1] + ci[j]]) + wr[2] * cells[ri[2] + ci[j]]) + wr[3] * cells[ri[3] + ci[j]];
  }
  const double* wv = TR ? wr : wc;
  return ((wv[0] * h[0] + wv[1] * h[1]) + wv[2] * h[2]) + wv[3] * h[3];
}

template <bool TR, bool JS>
__global__ __launch_bounds__(BIN_BLOCK) void bscan_bin_kernel(BscanBinArgs a) {
  extern __shared__ double bin_lds[];
  double* tr = bin_lds;                          // the phases along memory rows ...
  double* tc = tr + kBinTapStride * a.upr;       // ... and along memory columns
  double* cells = tc + kBinTapStride * a.upc;
  {
    const double* gr = a.taps + (TR ? 1 : 0) * kBinMaxUp * kBinTapStride;
    const double* gc = a.taps + (TR ? 0 : 1) * kBinMaxUp * kBinTapStride;
    for (int i = threadIdx.x; i < kBinTapStride * a.upr; i += BIN_BLOCK) tr[i] = gr[i];
    for (int i = threadIdx.x; i < kBinTapStride * a.upc; i += BIN_BLOCK) tc[i] = gc[i];
  }
  const long long per_image = (long long)a.tiles_r * a.tiles_c, ntiles = per_image * a.nb;
  for (long long ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const long long g = ti / per_image;
    const int rem = (int)(ti - g * per_image);
    const int or0 = (rem / a.tiles_c) * BIN_TILE_R, oc0 = (rem % a.tiles_c) * BIN_TILE_C;
    const int or1 = min(or0 + BIN_TILE_R, a.OR), oc1 = min(oc0 + BIN_TILE_C, a.OC);
    // the cells this tile's taps touch: two before the first output's cell to two after the last one's, inside the binned image
    BinTile t;
    t.kr_lo = max(or0 / a.upr - 2, 0);
    t.kc_lo = max(oc0 / a.upc - 2, 0);
    const int kr_hi = min((or1 - 1) / a.upr + 2, a.NR - 1), kc_hi = min((oc1 - 1) / a.upc + 2, a.NC - 1);
    const int g_lo = t.kc_lo / a.group, ngroups = kc_hi / a.group - g_lo + 1;
    const int ncr = kr_hi - t.kr_lo + 1;
    const float* img = a.in + g * a.in_bs;
    __syncthreads();  // the last tile's readers are done with the LDS tile
    for (int it = threadIdx.x; it < ncr * ngroups; it += BIN_BLOCK) {
      const int ir = it / ngroups, cg = g_lo + (it - ir * ngroups);
      const int c0 = cg * a.group * a.binc;
      const int span = min(a.group * a.binc, a.C - c0);
      double acc[4];
      bin_reduce<TR, JS>(a, img, t.kr_lo + ir, c0, span, acc);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int cc = cg * a.group + k;
        if (k < a.group && cc >= t.kc_lo && cc <= kc_hi) cells[ir * a.lds_stride + cc - t.kc_lo] = acc[k] * a.inv_area * a.mf;
      }
    }
    __syncthreads();
    const int nquads = (oc1 - oc0 + 3) >> 2;
    for (int it = threadIdx.x; it < (or1 - or0) * nquads; it += BIN_BLOCK) {
      const int lr = it / nquads, orow = or0 + lr, ocol = oc0 + 4 * (it - lr * nquads);
      float lin[4], db[4];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        lin[e] = db[e] = 0.f;
        if (ocol + e >= a.OC) continue;
        const double v = bin_cubic<TR>(a, tr, tc, cells, t, orow, ocol + e);
        lin[e] = (float)v;
        if (a.out_db) {
          double vd = v;  // 1873-1874: depth row 4 over rows 0 and 1, recomputed here
          if (a.mask && (TR ? orow : ocol + e) < 2) vd = TR ? bin_cubic<TR>(a, tr, tc, cells, t, 4, ocol + e) : bin_cubic<TR>(a, tr, tc, cells, t, orow, 4);
          vd = vd > a.eps ? vd : a.eps;
          db[e] = (float)(__dmul_rn(20.0, log(vd)) / 2.303);
        }
      }
      const long long o = g * a.out_bs + (long long)orow * a.OC + ocol;
      if (a.vec_out) {
        if (a.out_lin) *reinterpret_cast<float4*>(a.out_lin + o) = make_float4(lin[0], lin[1], lin[2], lin[3]);
        if (a.out_db) *reinterpret_cast<float4*>(a.out_db + o) = make_float4(db[0], db[1], db[2], db[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
          if (ocol + e < a.OC) {
            if (a.out_lin) a.out_lin[o + e] = lin[e];
            if (a.out_db) a.out_db[o + e] = db[e];
          }
      }
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// cells along one dimension a tile of T outputs can touch at factor u: the outputs' own cells and two on either side
int tile_cells(int T, int u, int n) { return std::min(n, (T - 1) / u + 6); }

}  // namespace

void bscanbin_build_taps(int up, double* taps) {
  const double A = -0.75;
  const double scale = 1.0 / up;
  for (int p = 0; p < up; p++) {
    const double f = (p + 0.5) * scale - 0.5;
    const double s = std::floor(f);
    const double t = f - s, t1 = t + 1.0, u = 1.0 - t;
    double* c = taps + kBinTapStride * p;
    c[0] = ((A * t1 - 5.0 * A) * t1 + 8.0 * A) * t1 - 4.0 * A;
    c[1] = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0;
    c[2] = ((A + 2.0) * u - (A + 3.0)) * u * u + 1.0;
    c[3] = 1.0 - c[0] - c[1] - c[2];
    c[4] = s - 1.0;
  }
}

void bscanbin_plan(BscanBinArgs* a, int num_cu) {
  a->vec_in = a->C % 4 == 0 && aligned16(a->in) && (!a->jscan || aligned16(a->jscan));
  a->vec_out = a->OC % 4 == 0 && (!a->out_lin || aligned16(a->out_lin)) && (!a->out_db || aligned16(a->out_db));
  a->group = 1;
  if (a->vec_in) a->group = a->binc % 4 == 0 ? 1 : (a->binc % 2 == 0 ? 2 : 4);
  a->tiles_r = (a->OR + BIN_TILE_R - 1) / BIN_TILE_R;
  a->tiles_c = (a->OC + BIN_TILE_C - 1) / BIN_TILE_C;
  const int ncr = tile_cells(BIN_TILE_R, a->upr, a->NR), ncc = tile_cells(BIN_TILE_C, a->upc, a->NC);
  a->lds_stride = ncc | 1;  // odd: the rows of a column of cells start in different banks
  a->lds_bytes = ((size_t)kBinTapStride * (a->upr + a->upc) + (size_t)ncr * a->lds_stride) * sizeof(double);
  const long long ntiles = (long long)a->tiles_r * a->tiles_c * a->nb;
  // (more tiles than the cap: tests/test_gpu_stage_grids.py, test_binning_more_tiles_than_workgroups)
  const long long resident = resident_blocks(num_cu, BIN_WAVES_PER_CU, BIN_BLOCK);
  a->blocks = (int)std::min(ntiles, resident);
}

hipError_t launch_bscan_bin(const BscanBinArgs& a, hipStream_t st) {
  auto k = a.transposed ? (a.jscan ? bscan_bin_kernel<true, true> : bscan_bin_kernel<true, false>)
                        : (a.jscan ? bscan_bin_kernel<false, true> : bscan_bin_kernel<false, false>);
  hipLaunchKernelGGL(k, dim3(a.blocks), dim3(BIN_BLOCK), a.lds_bytes, st, a);
  return hipGetLastError();
}

}  // namespace fdoct
