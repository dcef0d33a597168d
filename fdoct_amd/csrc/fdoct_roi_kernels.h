// fdoct_roi_kernels.h -- launchers of the B-scan readouts (fdoct_roi.hip) behind include/fdoct_roi.h.
// Internal: fdoct_roi.cpp is the only caller.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include "fdoct_grid.h"

namespace fdoct {

// One dB image batch as the readouts see it: nb B-scans of depths x ascans floats, in the chain's layout
// (FDOCT_LAYOUT_ROWMAJOR_HxD: [g][ascan][depth]; FDOCT_LAYOUT_TRANSPOSED_DxH: [g][depth][ascan]).
struct RoiImage {
  const float* db = nullptr;
  int nb = 0, depths = 0, ascans = 0;
  int transposed = 0;
};

// Holds are kept as order-preserving unsigned words of the f32 value (roi_encode), so that one atomicMax combines them.
__host__ __device__ inline uint32_t roi_encode(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float roi_decode(uint32_t u) {
  const uint32_t b = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  float f;
  __builtin_memcpy(&f, &b, 4);
  return f;
}
constexpr uint32_t kRoiHoldZero = 0x80000000u;  // roi_encode(0.0f): where every hold starts (BscanFFTpeak.cpp:175-179)

// Folds the image into the holds: cols[i] = max(cols[i], max over depths y..y+h-1 of A-scan x+i), i < w, and
// *scalar = max(*scalar, max over the same depths of A-scan ascanat).  One launch; num_cu sizes the grid.
hipError_t launch_roi_hold(const RoiImage& im, int x, int y, int w, int h, int ascanat, uint32_t* cols, uint32_t* scalar,
                           int num_cu, hipStream_t st);
// Per B-scan min / max of A-scan ascanat over depths 4..depths-1 (depths >= 5; rows 0-3 read as row 4, BscanFFT.cpp:154-157).
hipError_t launch_roi_ascan_minmax(const RoiImage& im, int ascanat, float* out_min, float* out_max, int num_cu, hipStream_t st);
// Per B-scan mean of depths vertpos..vertpos+2 x A-scans ascanat..ascanat+width-1, in double, fixed reduction order.
hipError_t launch_roi_mean(const RoiImage& im, int ascanat, int vertpos, int width, double* out, int num_cu, hipStream_t st);

}  // namespace fdoct
