// fdoct_complex_kernels.h -- the device side of include/fdoct_complex.h that is the add-on library's own (fdoct_complex.hip): the D x H
// layout of the complex A-scans.  The chain's kernels that write the pairs are the core library's (fdoct_wave_dev.h with
// FDOCT_WAVE_OPT_CXOUT, generic_kernel's CX form).
#pragma once
#include <hip/hip_runtime.h>

namespace fdoct {

constexpr int kCxTile = 32;  // the transpose moves tiles of 32 x 32 pairs through LDS, 256 threads each

// Tiles of one image of `rows` x `cols` pairs and of a batch of them; 0 where the batch has more tiles than a launch has workgroups
// (2^31 tiles are 16 TiB of pairs: no device holds them).
inline long long cx_transpose_tiles(int rows, int cols, long long images) {
  const long long per = (long long)((rows + kCxTile - 1) / kCxTile) * ((cols + kCxTile - 1) / kCxTile);
  return (images > 0 && per > 0 && per <= 0x7fffffffLL / images) ? per * images : 0;
}

// out[image][c][r] = in[image][r][c] for `images` images of rows x cols (re, im) pairs; in and out 8-byte aligned, not overlapping.
hipError_t launch_cx_transpose(const float2* in, float2* out, int rows, int cols, long long images, hipStream_t st);

}  // namespace fdoct
