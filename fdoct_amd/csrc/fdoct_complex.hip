// fdoct_complex.hip -- the D x H layout of the complex A-scans (include/fdoct_complex.h): a tiled transpose of 8-byte elements.
// One workgroup of 256 threads moves one 32 x 32 tile: 32 lanes read 32 consecutive pairs of an input row (256 bytes), four rows per
// step of eight; behind the barrier 32 lanes write 32 consecutive pairs of an output row.  The tile's LDS rows are 33 pairs long:
// the column read then strides 66 words, so the 32 lanes of an 8-byte LDS read start on 32 different even banks and no two of them
// meet (at 32 pairs a row they would all start on bank 0).  Partial tiles at both edges are masked, not padded.
#include "fdoct_complex_kernels.h"

namespace fdoct {

namespace {

__global__ __launch_bounds__(256) void cx_transpose_kernel(const float2* __restrict__ in, float2* __restrict__ out, int rows, int cols, int tiles_r,
                                                           int tiles_c) {
  __shared__ float2 tile[kCxTile][kCxTile + 1];
  const unsigned per = (unsigned)tiles_r * (unsigned)tiles_c;   // (< 2^31: the launch counts one workgroup per tile)
  const unsigned image = blockIdx.x / per, t = blockIdx.x - image * per;
  const int tr = (int)(t / (unsigned)tiles_c), tc = (int)(t - (unsigned)tr * (unsigned)tiles_c);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const size_t base = (size_t)image * rows * cols;
#pragma unroll
  for (int j = 0; j < kCxTile; j += 8) {
    const int r = tr * kCxTile + ty + j, c = tc * kCxTile + tx;
    if (r < rows && c < cols) tile[ty + j][tx] = in[base + (size_t)r * cols + c];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kCxTile; j += 8) {
    const int c = tc * kCxTile + ty + j, r = tr * kCxTile + tx;
    if (c < cols && r < rows) out[base + (size_t)c * rows + r] = tile[tx][ty + j];
  }
}

}  // namespace

hipError_t launch_cx_transpose(const float2* in, float2* out, int rows, int cols, long long images, hipStream_t st) {
  const long long tiles = cx_transpose_tiles(rows, cols, images);
  if (tiles < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cx_transpose_kernel, dim3((unsigned)tiles), dim3(256), 0, st, in, out, rows, cols, (rows + kCxTile - 1) / kCxTile,
                     (cols + kCxTile - 1) / kCxTile);
  return hipGetLastError();
}

}  // namespace fdoct
