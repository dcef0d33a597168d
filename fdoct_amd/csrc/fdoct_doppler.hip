// fdoct_doppler.hip -- the kernels of include/fdoct_doppler.h: the Kasai autocorrelation estimator with a rectangular window over
// complex A-scans (the header states the quantity; tests/doppler_model.py restates it in numpy).  The tile, the window pass and the
// bulk sum are fdoct_boxtile.h's; what is this file's own:
//
// doppler_kernel.  Per tile of 16 pair rows x 64 depth bins of one pair image:
//   stage   every pair of the tile and its halo is formed once: X1 and X2 as 8-byte loads, consecutive lanes on consecutive
//           depths; T = X2 conj(X1), turned by the row's bulk phasor where that is asked for; |X1|^2 + |X2|^2.  The three floats
//           go to three planes of LDS.  Pairs outside the pair image are not loaded.
//   window  the shared pass over the three planes.
//   store   cnt, the angle, the mask, and the stores: 4 or 8 bytes a lane, consecutive lanes on consecutive depths, lanes beyond
//           the image's edge masked.
//
// doppler_bulk_kernel, in front of it where bulk is set: one workgroup per pair row (a capped grid looping over rows) leaves the
// row's phasor B / |B| (1 where B is 0), B the sum of T over the bulk range, for the stage to turn T by.
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

__global__ __launch_bounds__(kBoxBulkBlock) void doppler_bulk_kernel(const DopplerArgs a) {
  __shared__ float2 part[kBoxBulkBlock];
  const long long rows = (long long)a.pair_images * a.pair_rows;
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const int image = (int)(row / a.pair_rows), r = (int)(row - (long long)image * a.pair_rows);
    const float2* x1 = a.x + dop_row_base(a, image, r) + a.bulk_first;
    const float2 B = box_bulk_sum(x1, x1 + a.partner, a.bulk_count, part);
    if (threadIdx.x == 0) a.bulk[row] = box_phasor(B, false);   // the stage multiplies by its conjugate
  }
}

__global__ __launch_bounds__(kBoxBlock) void doppler_kernel(const DopplerArgs a) {
  extern __shared__ __align__(16) float dop_lds[];
  const int sr = box_staged_rows(a.wa), sw = box_staged_depths(a.wd), ns = sr * sw;
  float* const s_re = dop_lds;                 // the staged tile: sr x sw a plane
  float* const s_im = s_re + ns;
  float* const s_pw = s_im + ns;
  float* const sums = s_pw + ns;               // its depth sums: sr x 64 a plane

  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const BoxTile t = box_tile(tile, a.tiles_r, a.tiles_d, a.wa, a.wd);

    for (int i = threadIdx.x; i < ns; i += kBoxBlock) {
      int r, b;
      DopPair p = {0.f, 0.f, 0.f};
      if (box_staged(t, i, sw, a.pair_rows, a.depths, &r, &b)) {
        const float2* x1 = a.x + dop_row_base(a, t.image, r) + b;
        p = dop_pair(x1[0], x1[a.partner]);
        if (a.use_bulk) {
          const float2 u = a.bulk[(long long)t.image * a.pair_rows + r];   // B / |B|: T conj(u)
          const float re = p.re * u.x + p.im * u.y, im = p.im * u.x - p.re * u.y;
          p.re = re, p.im = im;
        }
      }
      s_re[i] = p.re, s_im[i] = p.im, s_pw[i] = p.pw;
    }

    float w[kDopPlanes][kBoxOwn];              // re, im, power
    box_window<kDopPlanes>(s_re, sums, sr, sw, a.wa, a.wd, kDopPlanes, w);

#pragma unroll
    for (int j = 0; j < kBoxOwn; j++) {
      int r, b;
      if (!box_owned(t, j, a.pair_rows, a.depths, &r, &b)) continue;
      const float cnt = (float)box_terms(r, b, a.pair_rows, a.depths, a.wa, a.wd);
      const float power = 0.5f * w[2][j] / cnt;
      const long long o = ((long long)t.image * a.pair_rows + r) * (long long)a.depths + b;
      if (a.out_corr) a.out_corr[o] = make_float2(w[0][j], w[1][j]);
      if (a.out_power) a.out_power[o] = power;
      if (a.out_phase) a.out_phase[o] = (a.min_power > 0.f && power < a.min_power) ? 0.f : a.scale * atan2f(w[1][j], w[0][j]);
    }
  }
}

LdsGrant g_doppler_lds;

}  // namespace

hipError_t launch_doppler(const DopplerArgs& a, hipStream_t st) {
  if (a.blocks < 1 || a.tiles < 1 || (a.use_bulk && (a.bulk_blocks < 1 || !a.bulk))) return hipErrorInvalidValue;
  if (hipError_t e = g_doppler_lds.ensure(doppler_kernel, a.lds_bytes); e != hipSuccess) return e;
  if (a.use_bulk) {
    hipLaunchKernelGGL(doppler_bulk_kernel, dim3((unsigned)a.bulk_blocks), dim3(kBoxBulkBlock), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(doppler_kernel, dim3((unsigned)a.blocks), dim3(kBoxBlock), a.lds_bytes, st, a);
  return hipGetLastError();
}

}  // namespace fdoct
