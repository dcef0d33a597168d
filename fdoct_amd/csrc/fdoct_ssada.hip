// fdoct_ssada.hip -- the kernels of include/fdoct_ssada.h: split-spectrum amplitude decorrelation (the header states the quantity;
// tests/ssada_model.py restates it in numpy).  Between the split and the mean runs fdoct_angio.hip's own stage (launch_angio).
//
// ssada_table_kernel.  The transform's twiddles e^(+2 pi i m / n) and the bands' table G_m(q), every entry evaluated in double and
// rounded to float; grid-stride, one entry a thread.
//
// ssada_split_kernel.  One workgroup of 256 threads takes one A-scan and a chunk of bands at a time and loops over them (the grid
// is capped, fdoct_grid.h).  It loads the row into LDS, transforms it forward once and keeps z = F / n beside the transform's two
// ping-pong buffers.  Then, band by band: the work buffer gets z times G_m (4-byte loads of the table, consecutive lanes on
// consecutive q; two float multiplies), the inverse transform runs over the two buffers (fdoct_lds_fft.h), and the depth range
// goes out as 8-byte pairs, consecutive lanes on consecutive depths.  Nothing of a band's arithmetic depends on the chunk it lies
// in or on the workgroup that takes it, so a band gives the same bits in any grid.
//
// ssada_mean_kernel.  A thread owns one pixel at a time (grid-stride): the float sums of d and p over the bands in increasing m
// from 0.f, one division by (float)M each, the mask, the stores -- 4 bytes a lane, consecutive lanes on consecutive depths.
#include "fdoct_kernels.h"
#include "fdoct_ssada_kernels.h"

namespace fdoct {

namespace {

__global__ __launch_bounds__(kSsaBlock) void ssada_table_kernel(const SsadaArgs a) {
  const int n = a.fft.n;
  const size_t total = ((size_t)1 + (size_t)a.nbands) * (size_t)n;
  const double spacing = (double)a.k_count / (double)a.nbands;
  for (size_t e = (size_t)blockIdx.x * kSsaBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kSsaBlock) {
    const size_t t = e / (size_t)n;
    const int q = (int)(e - t * (size_t)n);
    if (t == 0) {
      double s, c;
      sincospi(2.0 * (double)q / (double)n, &s, &c);
      a.tw[q] = make_float2((float)c, (float)s);
    } else {
      const int m = (int)t - 1;
      float g = 0.f;
      if (q >= a.k_first && q < a.k_first + a.k_count) {
        const double centre = (double)a.k_first + ((double)m + 0.5) * spacing - 0.5;
        const double u = ((double)q - centre) / a.sigma;
        g = (float)exp(-0.5 * (u * u));
      }
      a.gauss[(size_t)m * (size_t)n + (size_t)q] = g;
    }
  }
}

__global__ __launch_bounds__(kSsaBlock) void ssada_split_kernel(const SsadaArgs a) {
  extern __shared__ __align__(16) unsigned char ssada_lds[];
  const int n = a.fft.n, tid = threadIdx.x;
  v2f* z = reinterpret_cast<v2f*>(ssada_lds);
  v2f* bufA = z + n;
  v2f* bufB = bufA + n;
  const v2f* tw = reinterpret_cast<const v2f*>(a.tw);
  const float inv_n = 1.0f / (float)n;
  const int b0 = a.depth_first, dc = a.depth_count;

  for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const long long row = item / a.chunks;                       // frame x A-scan
    const int ch = (int)(item - row * a.chunks);
    const long long f = row / a.ascans;
    const int r = (int)(row - f * a.ascans);
    const int g = (int)(f / a.repeats), rep = (int)(f - (long long)g * a.repeats);
    const int m0 = ch * a.per_wg, m1 = min(a.nbands, m0 + a.per_wg);
    const v2f* x = reinterpret_cast<const v2f*>(a.x) + (size_t)row * (size_t)n;

    for (int i = tid; i < n; i += kSsaBlock) bufA[i] = x[i];
    __syncthreads();
    const v2f* F = lds_fft<false, kSsaBlock>(bufA, bufB, a.fft, tw);
    for (int i = tid; i < n; i += kSsaBlock) z[i] = F[i] * inv_n;
    __syncthreads();

    for (int m = m0; m < m1; m++) {
      const float* G = a.gauss + (size_t)m * (size_t)n;
      for (int q = tid; q < n; q += kSsaBlock) bufA[q] = z[q] * G[q];
      __syncthreads();
      const v2f* A = lds_fft<true, kSsaBlock>(bufA, bufB, a.fft, tw);
      v2f* o = reinterpret_cast<v2f*>(a.bands) + ((((size_t)g * a.nbands + m) * a.repeats + rep) * (size_t)a.ascans + r) * (size_t)dc;
      for (int j = tid; j < dc; j += kSsaBlock) o[j] = A[b0 + j];
      __syncthreads();   // every read of A lies in front of it: the next band, or the next row, may write either buffer
    }
  }
}

__global__ __launch_bounds__(kSsaBlock) void ssada_mean_kernel(const SsadaArgs a) {
  const long long pixels = (long long)a.ascans * a.depth_count;
  const long long total = (long long)a.groups * pixels;
  const float fm = (float)a.nbands;
  for (long long i = (long long)blockIdx.x * kSsaBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kSsaBlock) {
    const long long g = i / pixels, px = i - g * pixels;
    const long long first = g * a.nbands * pixels + px;
    float power = 0.f;
    if (a.band_power) {
      float s = 0.f;
      for (int m = 0; m < a.nbands; m++) s += a.band_power[first + (long long)m * pixels];
      power = s / fm;
      if (a.out_power) a.out_power[i] = power;
    }
    if (a.out_decorr) {
      float s = 0.f;
      for (int m = 0; m < a.nbands; m++) s += a.band_decorr[first + (long long)m * pixels];
      const bool masked = a.min_power > 0.f && power < a.min_power;
      a.out_decorr[i] = masked ? 0.f : s / fm;
    }
  }
}

LdsGrant g_ssada_lds;

}  // namespace

hipError_t launch_ssada_table(const SsadaArgs& a, hipStream_t st) {
  if (!a.tw || !a.gauss || a.fft.n < kSsaMinN || a.fft.n > kSsaMaxN || a.nbands < 1 || a.nbands > kSsaMaxBands || a.k_count < 1 || a.k_first < 0 ||
      a.k_first + a.k_count > a.fft.n)
    return hipErrorInvalidValue;
  const size_t entries = ((size_t)1 + (size_t)a.nbands) * (size_t)a.fft.n;   // <= 17 x 4096
  hipLaunchKernelGGL(ssada_table_kernel, dim3((unsigned)((entries + kSsaBlock - 1) / kSsaBlock)), dim3(kSsaBlock), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_ssada_split(const SsadaArgs& a, hipStream_t st) {
  if (!a.x || !a.bands || !a.tw || !a.gauss || a.groups < 1 || a.repeats < 1 || a.ascans < 1 || a.nbands < 1 || a.per_wg < 1 || a.chunks < 1 ||
      a.chunks * a.per_wg < a.nbands || a.items != (long long)a.groups * a.repeats * a.ascans * a.chunks || a.blocks < 1 || a.fft.npass < 1 ||
      a.fft.n < kSsaMinN || a.fft.n > kSsaMaxN || a.lds_bytes != ssada_lds_bytes(a.fft.n) || a.depth_count < 1 || a.depth_first < 0 ||
      a.depth_first + a.depth_count > a.fft.n)
    return hipErrorInvalidValue;
  if (hipError_t e = g_ssada_lds.ensure(ssada_split_kernel, a.lds_bytes); e != hipSuccess) return e;
  hipLaunchKernelGGL(ssada_split_kernel, dim3((unsigned)a.blocks), dim3(kSsaBlock), a.lds_bytes, st, a);
  return hipGetLastError();
}

hipError_t launch_ssada_mean(const SsadaArgs& a, hipStream_t st) {
  if ((!a.out_decorr && !a.out_power) || (a.out_decorr && !a.band_decorr) || (a.out_power && !a.band_power) ||
      (a.out_decorr && a.min_power > 0.f && !a.band_power) || a.groups < 1 || a.ascans < 1 || a.depth_count < 1 || a.nbands < 1 || a.mean_blocks < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(ssada_mean_kernel, dim3((unsigned)a.mean_blocks), dim3(kSsaBlock), 0, st, a);
  return hipGetLastError();
}

}  // namespace fdoct
