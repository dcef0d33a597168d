// fdoct_doppler.hip -- the kernels of include/fdoct_doppler.h: the Kasai autocorrelation estimator with a rectangular window over
// complex A-scans (the header states the quantity; tests/doppler_model.py restates it in numpy).
//
// doppler_kernel.  One workgroup of 256 threads takes one tile of 16 pair rows x 64 depth bins of one pair image at a time and
// loops over tiles (the grid is capped, fdoct_grid.h).  Per tile:
//   stage   every pair of the tile and its halo -- (16 + wa - 1) x (64 + wd - 1) -- is formed once: X1 and X2 as 8-byte loads,
//           consecutive lanes on consecutive depths; T = X2 conj(X1), turned by the row's bulk phasor where that is asked for;
//           |X1|^2 + |X2|^2.  The three floats go to three planes of LDS.  Pairs outside the pair image are not loaded: their
//           terms are zeros, which change no sum.
//   depth   for every staged row and each of the tile's 64 bins, the wd terms along depth, in increasing depth.
//   rows    for every output, the wa depth sums down the column, in increasing row; then cnt (the window's overlap with the
//           pair image, counted from the indices), the angle, the mask, and the stores: 4 or 8 bytes a lane, consecutive lanes on
//           consecutive depths, lanes beyond the image's edge masked.
// LDS holds planes of floats, not pairs, and in all three phases a wave's 64 lanes lie along depth: every LDS access of a wave is
// 64 consecutive words, which no bank serves twice -- the column pass included, since it walks rows in time, not across lanes --
// so the layout needs neither padding nor a swizzle.  The sums are taken in a fixed order that depends on the window and the
// indices only, so a tile gives the same bits wherever the grid's loop puts it.
//
// doppler_bulk_kernel, in front of it where bulk is set: one workgroup per pair row (a capped grid looping over rows) sums T over
// the bulk range -- a strided partial per thread, then a tree in LDS; no atomics, a fixed order -- and leaves the row's phasor
// B / |B| (1 where B is 0) for the stage to turn T by.
#include "fdoct_doppler_kernels.h"
#include "fdoct_kernels.h"

namespace fdoct {

namespace {

struct DopPair {
  float re, im, pw;
};

// T = X2 conj(X1) and |X1|^2 + |X2|^2 of one pair.
__device__ __forceinline__ DopPair dop_pair(float2 x1, float2 x2) {
  DopPair t;
  t.re = x2.x * x1.x + x2.y * x1.y;
  t.im = x2.y * x1.x - x2.x * x1.y;
  t.pw = (x1.x * x1.x + x1.y * x1.y) + (x2.x * x2.x + x2.y * x2.y);
  return t;
}

// Where pair row `row` of pair image `image` starts in x: X1, and X2 lies a.partner pairs behind it.  On both axes pair image p
// starts at frame p and pair row r at that frame's A-scan r.
__device__ __forceinline__ long long dop_row_base(const DopplerArgs& a, int image, int row) {
  return ((long long)image * a.ascans + row) * (long long)a.depths;
}

__global__ __launch_bounds__(kDopBulkBlock) void doppler_bulk_kernel(const DopplerArgs a) {
  __shared__ float2 part[kDopBulkBlock];
  const long long rows = (long long)a.pair_images * a.pair_rows;
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const int image = (int)(row / a.pair_rows), r = (int)(row - (long long)image * a.pair_rows);
    const float2* x1 = a.x + dop_row_base(a, image, r) + a.bulk_first;
    const float2* x2 = x1 + a.partner;
    float2 s = make_float2(0.f, 0.f);
    for (int b = threadIdx.x; b < a.bulk_count; b += kDopBulkBlock) {
      const DopPair t = dop_pair(x1[b], x2[b]);
      s.x += t.re, s.y += t.im;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int half = kDopBulkBlock / 2; half > 0; half >>= 1) {
      if ((int)threadIdx.x < half) {
        const float2 o = part[threadIdx.x + half];
        part[threadIdx.x].x += o.x, part[threadIdx.x].y += o.y;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {  // what the stage multiplies by: conj(B) / |B| as (re, -im) of B / |B|, or 1 where B is 0
      const float2 B = part[0];
      const float m = hypotf(B.x, B.y);
      a.bulk[row] = m > 0.f ? make_float2(B.x / m, B.y / m) : make_float2(1.f, 0.f);
    }
    __syncthreads();  // part is the next row's
  }
}

__global__ __launch_bounds__(kDopBlock) void doppler_kernel(const DopplerArgs a) {
  extern __shared__ __align__(16) float dop_lds[];
  const int sr = kDopTileRows + a.wa - 1, sw = kDopTileDepths + a.wd - 1;
  float* const s_re = dop_lds;                 // the staged tile: sr x sw
  float* const s_im = s_re + sr * sw;
  float* const s_pw = s_im + sr * sw;
  float* const d_re = s_pw + sr * sw;          // its depth sums: sr x 64
  float* const d_im = d_re + sr * kDopTileDepths;
  float* const d_pw = d_im + sr * kDopTileDepths;
  const int back_r = (a.wa - 1) / 2, back_d = (a.wd - 1) / 2;
  const long long per_image = (long long)a.tiles_r * a.tiles_d;

  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int image = (int)(tile / per_image);
    const int t = (int)(tile - (long long)image * per_image);
    const int tr = t / a.tiles_d, td = t - tr * a.tiles_d;
    const int row0 = tr * kDopTileRows - back_r, dep0 = td * kDopTileDepths - back_d;   // the staged tile's first row and depth

    for (int i = threadIdx.x; i < sr * sw; i += kDopBlock) {
      const int lr = i / sw, lc = i - lr * sw;
      const int r = row0 + lr, b = dep0 + lc;
      DopPair p = {0.f, 0.f, 0.f};
      if (r >= 0 && r < a.pair_rows && b >= 0 && b < a.depths) {
        const float2* x1 = a.x + dop_row_base(a, image, r) + b;
        p = dop_pair(x1[0], x1[a.partner]);
        if (a.use_bulk) {
          const float2 u = a.bulk[(long long)image * a.pair_rows + r];   // B / |B|: T conj(u)
          const float re = p.re * u.x + p.im * u.y, im = p.im * u.x - p.re * u.y;
          p.re = re, p.im = im;
        }
      }
      s_re[i] = p.re, s_im[i] = p.im, s_pw[i] = p.pw;
    }
    __syncthreads();

    for (int i = threadIdx.x; i < sr * kDopTileDepths; i += kDopBlock) {
      const int lr = i / kDopTileDepths, c = i - lr * kDopTileDepths;
      const int at = lr * sw + c;
      float re = 0.f, im = 0.f, pw = 0.f;
      for (int j = 0; j < a.wd; j++) re += s_re[at + j], im += s_im[at + j], pw += s_pw[at + j];
      d_re[i] = re, d_im[i] = im, d_pw[i] = pw;
    }
    __syncthreads();

    for (int i = threadIdx.x; i < kDopTileRows * kDopTileDepths; i += kDopBlock) {
      const int lr = i / kDopTileDepths, c = i - lr * kDopTileDepths;
      const int r = tr * kDopTileRows + lr, b = td * kDopTileDepths + c;
      if (r >= a.pair_rows || b >= a.depths) continue;
      float re = 0.f, im = 0.f, pw = 0.f;
      for (int j = 0; j < a.wa; j++) {
        const int at = (lr + j) * kDopTileDepths + c;
        re += d_re[at], im += d_im[at], pw += d_pw[at];
      }
      const int r_lo = max(r - back_r, 0), r_hi = min(r + a.wa / 2, a.pair_rows - 1);
      const int b_lo = max(b - back_d, 0), b_hi = min(b + a.wd / 2, a.depths - 1);
      const float cnt = (float)((r_hi - r_lo + 1) * (b_hi - b_lo + 1));
      const float power = 0.5f * pw / cnt;
      const long long o = ((long long)image * a.pair_rows + r) * (long long)a.depths + b;
      if (a.out_corr) a.out_corr[o] = make_float2(re, im);
      if (a.out_power) a.out_power[o] = power;
      if (a.out_phase) a.out_phase[o] = (a.min_power > 0.f && power < a.min_power) ? 0.f : a.scale * atan2f(im, re);
    }
    __syncthreads();  // the planes are the next tile's
  }
}

LdsGrant g_doppler_lds;

}  // namespace

hipError_t launch_doppler(const DopplerArgs& a, hipStream_t st) {
  if (a.blocks < 1 || a.tiles < 1 || (a.use_bulk && (a.bulk_blocks < 1 || !a.bulk))) return hipErrorInvalidValue;
  if (hipError_t e = g_doppler_lds.ensure(doppler_kernel, a.lds_bytes); e != hipSuccess) return e;
  if (a.use_bulk) {
    hipLaunchKernelGGL(doppler_bulk_kernel, dim3((unsigned)a.bulk_blocks), dim3(kDopBulkBlock), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(doppler_kernel, dim3((unsigned)a.blocks), dim3(kDopBlock), a.lds_bytes, st, a);
  return hipGetLastError();
}

}  // namespace fdoct
