// fdoct_lowpass.hip -- BscanDark's lpfilter (BscanDark.cpp:119-167) behind include/fdoct_lowpass.h: a row-wise forward DFT
// scaled by 1 / W, the fftshifted spectrum blanked except for the columns [W/2 - f, W/2 + f), f = floor(W / 10), and the
// unscaled real-output inverse DFT.  The inverse reads bins 0 .. W/2 as a conjugate-symmetric spectrum, so of the kept bins
// -f .. f - 1 only 0 .. f - 1 are ever used and the filter is
//   y[m] = Re F[0] + 2 * sum_{k=1}^{f-1} Re( F[k] e^(+2 pi i k m / W) ),   F[k] = (1 / W) sum_n x[n] e^(-2 pi i k n / W),
// for even and odd W alike, all zeros for 1 < W < 10 and the sample itself for W = 1, where nothing is blanked (tests/lowpass_model.py keeps the literal steps; tests/test_lowpass_model.py
// confirms the closed form against them).  Only f bins are needed, so they are evaluated directly, in double.
//
// One workgroup of 256 owns a row.
//   analysis   a thread owns bin k and one of G slices of the samples (DftBinF64, fdoct_fft_reg.h: 8 samples per chunk against 8
//              phasors in registers, the chunk's base phasor advanced by recurrence and re-seeded from sincospi every 256
//              chunks); the G partial sums of a bin are added in slice order by one thread.  G and the slice length are
//              functions of W alone.
//   synthesis  a thread owns the output pair (j, W - j), whose phasors are conjugates: A = sum Re F[k] cos, B = sum Im F[k] sin,
//              y[j] = F0 + 2 (A - B), y[W - j] = F0 + 2 (A + B).  Its phasor e^(2 pi i k j / W) advances by recurrence over k and
//              is re-seeded every 256 bins; F[k] is one broadcast read per step.  y[0] and (even W) y[W/2] need no phasor and are
//              summed by one wave each, lane-strided and then a shuffle tree.
// A row is staged in LDS as doubles with its bins next to it while that fits in 64 KB (W <= ~5900); longer rows read their
// samples through the caches and keep their bins in a workspace in global memory.  Every sample is read before the first
// barrier and written after the last one, so a row may be filtered in place.  The order of every sum depends on W only -- not
// on the grid, the pitch or where the row lies -- so the same row gives the same bits wherever it is filtered.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "fdoct_capture_kernels.h"
#include "fdoct_fft_reg.h"

namespace fdoct {

namespace {

constexpr int LP_BLOCK = 256;
constexpr int LP_WAVES_PER_CU = 16;  // the grid's cap, as the other capture kernels cap theirs
constexpr int LP_T = 8;              // samples per chunk of a bin's sum
constexpr int LP_RESEED = 256;       // steps of a phasor recurrence between two exact values
constexpr int LP_MAX_SLICES = 8;
constexpr size_t LP_LDS_MAX = 64 * 1024;

struct LowpassArgs {
  const unsigned char* in;
  unsigned char* out;
  long long in_pitch, out_pitch;  // bytes per row
  int rows, W, f;
  int G, L;     // slices per bin and samples per slice (a multiple of LP_T; G * L >= W)
  double2* ws;  // rows longer than LDS: 2 * f bins per workgroup
};

// e^(sign * 2 pi i (q mod W) / W) with the product's index taken exactly
__device__ __forceinline__ void root_of_unity(long long q, int W, double sign, double* re, double* im) {
  sincospi(sign * (double)(2 * (q % W)) / (double)W, im, re);
}

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s = s + __shfl_xor(s, off, 64);
  return s;
}

template <bool STAGED>
__global__ __launch_bounds__(LP_BLOCK) void lowpass_rows_kernel(LowpassArgs a) {
  extern __shared__ __align__(16) double lp_lds[];
  const int tid = threadIdx.x, W = a.W, f = a.f;
  double* xs = lp_lds;  // STAGED: G * L samples, zeros past the row's end
  double2 *part, *Fs;   // part[g * f + k]: slice g of bin k; Fs[k] = F[k]
  if constexpr (STAGED) {
    part = reinterpret_cast<double2*>(lp_lds + (size_t)a.G * a.L);
    Fs = part + (size_t)a.G * f;
  } else {
    part = a.ws + (size_t)blockIdx.x * 2 * f;
    Fs = part + f;
  }
  for (int r = blockIdx.x; r < a.rows; r += gridDim.x) {
    const double* x = reinterpret_cast<const double*>(a.in + r * a.in_pitch);
    double* y = reinterpret_cast<double*>(a.out + r * a.out_pitch);
    if (f == 0) {  // W < 10: every column is blanked -- but for W = 1, whose ranges are empty: its one-point transforms copy
      for (int i = tid; i < W; i += LP_BLOCK) y[i] = W == 1 ? x[i] : 0.0;
      continue;
    }
    if constexpr (STAGED) {
      for (int i = tid; i < a.G * a.L; i += LP_BLOCK) xs[i] = i < W ? x[i] : 0.0;
      __syncthreads();
    }
    // ---- analysis
    for (int it = tid; it < f * a.G; it += LP_BLOCK) {
      const int g = it / f, k = it - g * f;
      const int m0 = g * a.L;
      DftBinF64<LP_T> bin;
      bin.init(k, 0, W);
      for (int c = 0; c < a.L / LP_T; c++) {
        const int m = m0 + c * LP_T;
        if (c % LP_RESEED == 0) root_of_unity((long long)k * m, W, -1.0, &bin.br, &bin.bi);
        double v[LP_T];
#pragma unroll
        for (int t = 0; t < LP_T; t++) {
          if constexpr (STAGED)
            v[t] = xs[m + t];
          else
            v[t] = m + t < W ? x[m + t] : 0.0;
        }
        bin.chunk(v);
      }
      part[it] = make_double2(bin.ar, bin.ai);
    }
    __syncthreads();
    for (int k = tid; k < f; k += LP_BLOCK) {
      double2 s = part[k];
      for (int g = 1; g < a.G; g++) {
        const double2 p = part[g * f + k];
        s.x = s.x + p.x, s.y = s.y + p.y;
      }
      Fs[k] = make_double2(s.x / (double)W, s.y / (double)W);  // DFT_SCALE
    }
    __syncthreads();
    // ---- synthesis
    const double f0 = Fs[0].x;
    const int half = (W - 1) / 2;  // the pairs (j, W - j), 1 <= j <= half
    for (int j = 1 + tid; j <= half; j += LP_BLOCK) {
      double sr, si;
      root_of_unity(j, W, 1.0, &sr, &si);
      double pr = sr, pi = si, A = 0.0, B = 0.0;
      for (int k = 1; k < f; k++) {
        if (k % LP_RESEED == 0) root_of_unity((long long)k * j, W, 1.0, &pr, &pi);
        const double2 F = Fs[k];
        A = fma(F.x, pr, A);
        B = fma(F.y, pi, B);
        const double nr = fma(pr, sr, -pi * si);
        pi = fma(pr, si, pi * sr);
        pr = nr;
      }
      y[j] = f0 + 2.0 * (A - B);
      y[W - j] = f0 + 2.0 * (A + B);
    }
    const int wave = tid >> 6, lane = tid & 63;
    if (wave == 0 || (wave == 1 && W % 2 == 0)) {  // y[0]: every phasor is 1; y[W/2]: (-1)^k
      double s = 0.0;
      for (int k = 1 + lane; k < f; k += 64) s = s + ((wave == 1 && (k & 1)) ? -Fs[k].x : Fs[k].x);
      s = wave_sum(s);
      if (lane == 0) y[wave == 0 ? 0 : W / 2] = f0 + 2.0 * s;
    }
    __syncthreads();  // (the next row overwrites xs / part / Fs)
  }
}

}  // namespace

LowpassShape lowpass_shape(int rows, int W, int num_cu) {
  LowpassShape s;
  s.f = W / 10;
  const int chunks = (W + LP_T - 1) / LP_T;
  const int f1 = std::max(1, s.f);
  s.G = std::max(1, std::min({LP_MAX_SLICES, LP_BLOCK / f1, chunks}));
  s.L = (chunks + s.G - 1) / s.G * LP_T;
  s.lds = sizeof(double) * (size_t)s.G * s.L + sizeof(double2) * (size_t)s.f * (s.G + 1);
  s.staged = s.lds <= LP_LDS_MAX;
  if (!s.staged) {
    s.G = 1, s.L = chunks * LP_T;
    s.lds = 0;
  }
  // (more rows than the cap, more than 256 staged bins, the last staged width 5849 and every slice count:
  // tests/test_gpu_stage_grids.py, test_lowpass_*; the formulas restated in tests/stage_grid_sizes.py)
  const int cap = resident_blocks(num_cu, LP_WAVES_PER_CU, LP_BLOCK);
  s.blocks = std::max(1, std::min(rows, cap));
  s.ws_doubles = s.staged ? 0 : (size_t)s.blocks * 4 * s.f;
  return s;
}

hipError_t launch_lowpass_rows(const double* in, size_t in_pitch, double* out, size_t out_pitch, int rows, int W, double* ws,
                               int num_cu, hipStream_t st) {
  if (!in || !out || rows < 1 || W < 1 || in_pitch < sizeof(double) * (size_t)W || out_pitch < sizeof(double) * (size_t)W ||
      in_pitch % sizeof(double) || out_pitch % sizeof(double))
    return hipErrorInvalidValue;
  const LowpassShape s = lowpass_shape(rows, W, num_cu);
  if (s.ws_doubles && !ws) return hipErrorInvalidValue;
  LowpassArgs a{};
  a.in = reinterpret_cast<const unsigned char*>(in);
  a.out = reinterpret_cast<unsigned char*>(out);
  a.in_pitch = (long long)in_pitch, a.out_pitch = (long long)out_pitch;
  a.rows = rows, a.W = W, a.f = s.f, a.G = s.G, a.L = s.L;
  a.ws = reinterpret_cast<double2*>(ws);
  if (s.staged)
    hipLaunchKernelGGL(lowpass_rows_kernel<true>, dim3(s.blocks), dim3(LP_BLOCK), s.lds, st, a);
  else
    hipLaunchKernelGGL(lowpass_rows_kernel<false>, dim3(s.blocks), dim3(LP_BLOCK), 0, st, a);
  return hipGetLastError();
}

}  // namespace fdoct
