// fdoct_bscanbin_kernels.h -- the output binning's kernel (fdoct_bscanbin.hip) behind include/fdoct_bscanbin.h: its argument
// block, the host-side sizing of a call and the cubic tap table.  Internal: fdoct_bscanbin.cpp is the only caller.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include "fdoct_grid.h"

namespace fdoct {

constexpr int kBinMaxFactor = 16;  // bscanbinx / bscanbiny: 1.0 / (1.0 / n) == n keeps the reference on INTER_AREA's integer path
constexpr int kBinMaxUp = 64;      // upx / upy
constexpr int kBinTapStride = 5;   // per phase: c0 c1 c2 c3 and the offset of the first tap's cell from d / u (as a double)
constexpr int kBinTapDoubles = 2 * kBinMaxUp * kBinTapStride;  // [0]: along A-scans (x, upx phases); [1]: along depths (y)

// One call as the kernel sees it.  R x C is a B-scan IN MEMORY (C the contiguous dimension): depths x ascans in the
// transposed layout, ascans x depths in the row-major one; every *r / *c member is along memory rows / columns.
struct BscanBinArgs {
  const float* in = nullptr;
  const float* jscan = nullptr;   // one R x C image shared by all B-scans, or null
  float* out_lin = nullptr;       // either may be null
  float* out_db = nullptr;
  const double* taps = nullptr;   // kBinTapDoubles doubles on the device (bscanbin_build_taps)
  long long in_bs = 0, out_bs = 0;  // floats per B-scan
  int nb = 0, R = 0, C = 0;
  int binr = 1, binc = 1, upr = 1, upc = 1;
  int NR = 0, NC = 0;             // binned cells
  int OR = 0, OC = 0;             // outputs
  int transposed = 0;             // memory rows are depths (the D x H layout)
  int mask = 0;                   // out_db: depth row 4 over depth rows 0 and 1
  double eps = 1e-5, inv_area = 1.0, mf = 1.0;
  // decided by bscanbin_plan
  int vec_in = 0, vec_out = 0, group = 1;  // 16-byte loads / stores; cells one thread reduces side by side (group * binc % 4 == 0)
  int lds_stride = 0;             // doubles between two cell rows of the LDS tile
  int tiles_r = 0, tiles_c = 0;
  size_t lds_bytes = 0;
  int blocks = 0;
};

// The `up` phases of INTER_CUBIC (A = -0.75) at scale 1 / up, in double: taps[5 p .. 5 p + 3] = c0 .. c3 and taps[5 p + 4] =
// floor(f) - 1 with f = (p + 0.5) * (1 / up) - 0.5: output d = k up + p reads cells k + offset .. k + offset + 3.
void bscanbin_build_taps(int up, double* taps);
// Fills the decided members from the others (pointers enter through their alignment).  Nothing is enqueued.
void bscanbin_plan(BscanBinArgs* a, int num_cu);
hipError_t launch_bscan_bin(const BscanBinArgs& a, hipStream_t st);

}  // namespace fdoct
