// fdoct_colour.hip -- the kernels behind include/fdoct_colour.h: what BscanFFTwebcam.cpp:1015-1038 does to the camera's 8-bit
// interleaved B,G,R frame before the block every program has.
//   channelnum 0 / 1 / 2   mraw = that channel (CV_8U), then resize(INTER_AREA)      -> bytes
//   channelnum 3           mraw = (double(B) + double(G) + double(R)) * 0.00130718954, then resize(INTER_AREA) on doubles
//                                                                                     -> doubles
// The stage only streams: 3 bytes in per pixel, 1 / area or 8 / area out.  colour_vec_kernel reads whole 16-byte words: a
// thread owns 16 output pixels, i.e. BX runs of 16 input pixels = 3 x 16 bytes each per input row, takes its channel out of
// every 12 bytes with byte permutes (or adds the three channels as packed 16-bit pairs), carries the block sums in registers
// over the biny input rows and stores 16 bytes (select) or 8 x 16 bytes (sum).  The extracted full-resolution channel is
// never written.  colour_px_kernel is the same arithmetic pixel by pixel, for rows that are not 16-byte aligned, bin widths
// other than 1, 2, 4 and the columns a width leaves over after its last whole group of 16.
// Arithmetic.  Select: the integer block sum, then bin_kernel's rounding (fdoct_generic.hip) -- (s + 2) >> 2 for 2 x 2,
// rintf(s * (1.f / area)) otherwise, the sample itself for 1 x 1.  Sum: B + G + R exactly, one double multiply by the
// constant, the block's values added in double from 0.0 rows outermost and left to right, one multiply by
// (double)(1.f / area) (ResizeAreaFast as DESIGN.md 3.4c reads it).  __dmul_rn / __dadd_rn: never contracted.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fdoct_colour_kernels.h"

namespace fdoct {

namespace {

constexpr int COL_BLOCK = 256;
constexpr int COL_MAX_BLOCKS = 8192;

// byte `off` (0 .. 11) of the 12-byte string w0 w1 w2
template <int OFF>
__device__ __forceinline__ unsigned byte_of(unsigned w0, unsigned w1, unsigned w2) {
  const unsigned w = OFF < 4 ? w0 : OFF < 8 ? w1 : w2;
  return (w >> (8 * (OFF & 3))) & 0xffu;
}
// channel C of the four pixels in w0 w1 w2, as the four bytes of a word (two v_perm_b32)
template <int C>
__device__ __forceinline__ unsigned channel4(unsigned w0, unsigned w1, unsigned w2) {
  return byte_of<C>(w0, w1, w2) | (byte_of<C + 3>(w0, w1, w2) << 8) | (byte_of<C + 6>(w0, w1, w2) << 16) | (byte_of<C + 9>(w0, w1, w2) << 24);
}

// 16 pixels = 48 bytes at p (16-byte aligned) -> px[16]: the channel's samples (C < 3) or B + G + R (C == 3).
// words != null (C < 3): the channel's 16 bytes as they will be stored.
template <int C>
__device__ __forceinline__ void load16(const unsigned char* __restrict__ p, unsigned (&px)[16], unsigned* words) {
  const uint4* v = reinterpret_cast<const uint4*>(p);
  const uint4 a = v[0], b = v[1], c = v[2];
  const unsigned w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const unsigned w0 = w[3 * j], w1 = w[3 * j + 1], w2 = w[3 * j + 2];
    if constexpr (C < 3) {
      const unsigned ch = channel4<C>(w0, w1, w2);
      if (words) words[j] = ch;
      px[4 * j] = ch & 0xffu;
      px[4 * j + 1] = (ch >> 8) & 0xffu;
      px[4 * j + 2] = (ch >> 16) & 0xffu;
      px[4 * j + 3] = ch >> 24;
    } else {
      // pixels 0 and 2 in the 16-bit halves of `even`, 1 and 3 in those of `odd`: three bytes sum to at most 765
      const unsigned B = channel4<0>(w0, w1, w2), G = channel4<1>(w0, w1, w2), R = channel4<2>(w0, w1, w2);
      const unsigned m = 0x00ff00ffu;
      const unsigned even = (B & m) + (G & m) + (R & m);
      const unsigned odd = ((B >> 8) & m) + ((G >> 8) & m) + ((R >> 8) & m);
      px[4 * j] = even & 0xffffu;
      px[4 * j + 1] = odd & 0xffffu;
      px[4 * j + 2] = even >> 16;
      px[4 * j + 3] = odd >> 16;
    }
  }
}

__device__ __forceinline__ unsigned round_bin(unsigned s, bool two_by_two, float scale) {
  return two_by_two ? (s + 2u) >> 2 : (unsigned)rintf((float)s * scale);
}

// The whole groups of 16 output pixels of every output row.  a.bgr and a.pitch are multiples of 16.
template <int BX, int C>
__global__ __launch_bounds__(COL_BLOCK) void colour_vec_kernel(ColourArgs a) {
  const int groups = a.ow / 16;
  const long long total = a.out_rows * groups;
  const int area = BX * a.biny;
  const float scale = 1.f / (float)area;
  const bool two_by_two = BX == 2 && a.biny == 2;
  for (long long e = (long long)blockIdx.x * COL_BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * COL_BLOCK) {
    const long long oy = e / groups;
    const int g = (int)(e - oy * groups);
    const unsigned char* row = a.bgr + oy * a.biny * a.pitch + (long long)g * (48 * BX);
    if constexpr (C < 3) {
      unsigned char* dst = static_cast<unsigned char*>(a.out) + oy * a.out_pitch + (long long)g * 16;
      if (BX == 1 && a.biny == 1) {  // nothing to add: the permuted words are the result
        unsigned px[16], words[4];
        load16<C>(row, px, words);
        *reinterpret_cast<uint4*>(dst) = make_uint4(words[0], words[1], words[2], words[3]);
        continue;
      }
      unsigned acc[16];
#pragma unroll
      for (int i = 0; i < 16; i++) acc[i] = 0u;
      for (int dy = 0; dy < a.biny; dy++, row += a.pitch) {
#pragma unroll
        for (int q = 0; q < BX; q++) {
          unsigned px[16];
          load16<C>(row + 48 * q, px, nullptr);
#pragma unroll
          for (int i = 0; i < 16; i++) acc[(16 * q + i) / BX] += px[i];
        }
      }
      unsigned o[4];
#pragma unroll
      for (int j = 0; j < 4; j++)
        o[j] = round_bin(acc[4 * j], two_by_two, scale) | (round_bin(acc[4 * j + 1], two_by_two, scale) << 8) |
               (round_bin(acc[4 * j + 2], two_by_two, scale) << 16) | (round_bin(acc[4 * j + 3], two_by_two, scale) << 24);
      *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
      double acc[16];
#pragma unroll
      for (int i = 0; i < 16; i++) acc[i] = 0.0;
      for (int dy = 0; dy < a.biny; dy++, row += a.pitch) {
#pragma unroll
        for (int q = 0; q < BX; q++) {
          unsigned px[16];
          load16<3>(row + 48 * q, px, nullptr);
#pragma unroll
          for (int i = 0; i < 16; i++) acc[(16 * q + i) / BX] = __dadd_rn(acc[(16 * q + i) / BX], __dmul_rn((double)px[i], kColourSumScale));
        }
      }
      const double inv = (double)scale;
      double2* dst = reinterpret_cast<double2*>(static_cast<unsigned char*>(a.out) + oy * a.out_pitch + (long long)g * 128);
#pragma unroll
      for (int j = 0; j < 8; j++) dst[j] = make_double2(__dmul_rn(acc[2 * j], inv), __dmul_rn(acc[2 * j + 1], inv));
    }
  }
}

// Output columns x0 .. ow - 1 of every output row, one pixel per thread, any alignment and any bin factors.
__global__ __launch_bounds__(COL_BLOCK) void colour_px_kernel(ColourArgs a, int x0) {
  const int cols = a.ow - x0;
  const long long total = a.out_rows * cols;
  const float scale = 1.f / (float)(a.binx * a.biny);
  const bool two_by_two = a.binx == 2 && a.biny == 2;
  for (long long e = (long long)blockIdx.x * COL_BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * COL_BLOCK) {
    const long long oy = e / cols;
    const int x = x0 + (int)(e - oy * cols);
    const unsigned char* row = a.bgr + oy * a.biny * a.pitch + (long long)x * a.binx * 3;
    if (a.channelnum < 3) {
      unsigned s = 0u;
      for (int dy = 0; dy < a.biny; dy++, row += a.pitch)
        for (int dx = 0; dx < a.binx; dx++) s += row[3 * dx + a.channelnum];
      const unsigned o = (a.binx == 1 && a.biny == 1) ? s : round_bin(s, two_by_two, scale);
      (static_cast<unsigned char*>(a.out) + oy * a.out_pitch)[x] = (unsigned char)o;
    } else {
      double s = 0.0;
      for (int dy = 0; dy < a.biny; dy++, row += a.pitch)
        for (int dx = 0; dx < a.binx; dx++) {
          const unsigned bgr = (unsigned)row[3 * dx] + row[3 * dx + 1] + row[3 * dx + 2];
          s = __dadd_rn(s, __dmul_rn((double)bgr, kColourSumScale));
        }
      reinterpret_cast<double*>(static_cast<unsigned char*>(a.out) + oy * a.out_pitch)[x] = __dmul_rn(s, (double)scale);
    }
  }
}

int blocks_for(long long items) {
  const long long b = (items + COL_BLOCK - 1) / COL_BLOCK;
  return (int)(b < 1 ? 1 : b > COL_MAX_BLOCKS ? COL_MAX_BLOCKS : b);
}

template <int BX>
void launch_vec(const ColourArgs& a, long long items, hipStream_t st) {
  const dim3 g(blocks_for(items)), b(COL_BLOCK);
  switch (a.channelnum) {
    case 0: hipLaunchKernelGGL((colour_vec_kernel<BX, 0>), g, b, 0, st, a); break;
    case 1: hipLaunchKernelGGL((colour_vec_kernel<BX, 1>), g, b, 0, st, a); break;
    case 2: hipLaunchKernelGGL((colour_vec_kernel<BX, 2>), g, b, 0, st, a); break;
    default: hipLaunchKernelGGL((colour_vec_kernel<BX, 3>), g, b, 0, st, a); break;
  }
}

}  // namespace

bool colour_vectorised(const ColourArgs& a) {
  return (a.binx == 1 || a.binx == 2 || a.binx == 4) && a.ow >= 16 && reinterpret_cast<uintptr_t>(a.bgr) % 16 == 0 && a.pitch % 16 == 0;
}

hipError_t launch_colour(const ColourArgs& a, hipStream_t st) {
  if (!a.bgr || !a.out || a.ow < 1 || a.out_rows < 1 || a.binx < 1 || a.biny < 1 || a.channelnum < 0 || a.channelnum > 3 ||
      a.pitch < 3LL * a.ow * a.binx || reinterpret_cast<uintptr_t>(a.out) % 16 || a.out_pitch % 16 ||
      a.out_pitch < (long long)a.ow * (a.channelnum == 3 ? 8 : 1))
    return hipErrorInvalidValue;
  // (more items than 8192 workgroups take in one pass, either kernel: tests/test_gpu_stage_grids.py, test_colour_*_beyond_one_pass)
  int x0 = 0;
  if (colour_vectorised(a)) {
    const long long items = a.out_rows * (a.ow / 16);
    if (a.binx == 1) launch_vec<1>(a, items, st);
    else if (a.binx == 2) launch_vec<2>(a, items, st);
    else launch_vec<4>(a, items, st);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    x0 = a.ow / 16 * 16;
  }
  if (x0 < a.ow) hipLaunchKernelGGL(colour_px_kernel, dim3(blocks_for(a.out_rows * (a.ow - x0))), dim3(COL_BLOCK), 0, st, a, x0);
  return hipGetLastError();
}

}  // namespace fdoct
