// fdoct_dispersion.hip -- the kernels of include/fdoct_dispersion.h: a numerical dispersion search over a grid of (a2, a3) on
// complex A-scans of the full transform length (the header states the quantity; tests/dispersion_model.py restates it in numpy).
//
// disp_table_kernel.  The transform's twiddles e^(+2 pi i m / n) and the two phasor tables e^(i a2_i x^2), e^(i a3_j x^3), every
// entry evaluated in double and rounded to float; grid-stride, one entry a thread.
//
// disp_search_kernel.  One workgroup of 256 threads takes one A-scan and a chunk of candidates.  It loads the row into LDS,
// transforms it forward once and keeps z = F / n beside the transform's two ping-pong buffers.  Then, candidate by candidate: the
// work buffer gets z times the candidate's phasor (the float product of one entry of each table: 8-byte loads, consecutive lanes on
// consecutive q), the inverse transform runs over the two buffers, every thread sums I = |A|^2 and I^2 of its bins of the depth
// range in double (bins b0 + tid, b0 + tid + 256, ... in that order), the block reduces the two doubles -- a butterfly of
// shuffles inside each wave, then the waves' partials through LDS in wave order -- and thread 0 writes the (row, candidate) pair.
// Nothing of a candidate's arithmetic depends on the chunk it lies in, so a candidate gives the same bits in any grid.
//   The transform: mixed-radix Stockham passes over LDS, radices 16 / 8 / 4 / 2 / 5 / 3 with the butterflies in registers
// (fdoct_fft_reg.h), the passes of fdoct_generic.hip written again here from the same butterflies -- butterfly j of a pass reads
// src[j + r nb], so a wave's lanes read consecutive pairs; its stores are Ns apart per register and, in the first pass, R apart
// across lanes, which is why the radix plan puts an odd or small radix first (fdoct_plan.cpp).
//
// disp_rowsum_kernel.  One thread per candidate sums the rows' pairs in increasing row order; lanes on consecutive candidates.
//
// disp_best_kernel.  One workgroup: metric = S4 / S2^2 (0 where S2 = 0) of every candidate, the lowest index of the largest
// finite one (each thread over its strided candidates in increasing index, then thread 0 over the threads' winners), and the
// winner's (cos, sin) table in double, rounded to float.
#include "fdoct_dispersion_kernels.h"
#include "fdoct_fft_reg.h"
#include "fdoct_kernels.h"

namespace fdoct {

namespace {

__device__ __forceinline__ double disp_x(int q, int n) { return ((double)q - 0.5 * (double)n) / (0.5 * (double)n); }

__global__ __launch_bounds__(kDispBlock) void disp_table_kernel(const DispersionArgs a) {
  const size_t total = ((size_t)1 + (size_t)a.a2_count + (size_t)a.a3_count) * (size_t)a.n;
  for (size_t e = (size_t)blockIdx.x * kDispBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kDispBlock) {
    const size_t t = e / (size_t)a.n;
    const int q = (int)(e - t * (size_t)a.n);
    double s, c;
    if (t == 0) {
      sincospi(2.0 * (double)q / (double)a.n, &s, &c);
    } else {
      const double x = disp_x(q, a.n);
      double phi;
      if (t <= (size_t)a.a2_count)
        phi = (a.a2_first + (double)(t - 1) * a.a2_step) * (x * x);
      else
        phi = (a.a3_first + (double)(t - 1 - (size_t)a.a2_count) * a.a3_step) * (x * x * x);
      sincos(phi, &s, &c);
    }
    a.tab[e] = make_float2((float)c, (float)s);
  }
}

// One Stockham pass of radix R (fdoct_generic.hip: fft_pass): butterfly j takes src[j + r nb], multiplies by
// exp(+-2 pi i r k / (Ns R)) (k = j mod Ns; tw[m] = exp(+2 pi i m / n)), transforms in registers and writes
// dst[(j div Ns) Ns R + k + r Ns].  j div Ns by multiplication: magic = ceil(2^32 / Ns) is exact for j, Ns < 2^16.
template <int R, bool INV>
__device__ __forceinline__ void disp_pass(const v2f* src, v2f* dst, int n, int Ns, unsigned magic, const v2f* tw) {
  const int nb = n / R;
  const int twstep = nb / Ns;
  for (int j = threadIdx.x; j < nb; j += kDispBlock) {
    int q = j, k = 0;
    if (Ns > 1) {
      q = (int)__umulhi((unsigned)j, magic);
      k = j - q * Ns;
    }
    v2f v[R];
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = src[j + r * nb];
    if (Ns > 1) {
      v2f w[R];
      w[1] = tw[k * twstep];
      if (!INV) w[1].y = -w[1].y;
#pragma unroll
      for (int r = 2; r < R; r++) w[r] = (r & 1) ? cmul(w[r - 1], w[1]) : cmul(w[r / 2], w[r / 2]);
#pragma unroll
      for (int r = 1; r < R; r++) v[r] = cmul(v[r], w[r]);
    }
    if constexpr (R == 3)
      fft_reg3<INV>(v);
    else if constexpr (R == 5)
      fft_reg5<INV>(v);
    else
      fft_reg<R, INV>(v);
    v2f* d = dst + (q * Ns * R + k);
#pragma unroll
    for (int r = 0; r < R; r++) d[r * Ns] = v[r];
  }
}

// The transform of length n over the two buffers; returns the one that holds the result.  Ends behind a barrier.
template <bool INV>
__device__ v2f* disp_fft(v2f* src, v2f* dst, const DispersionArgs& a, const v2f* tw) {
  int Ns = 1;
  for (int p = 0; p < a.npass; p++) {
    const int R = a.rad[p];
    const unsigned magic = a.magic[p];
    switch (R) {
      case 16: disp_pass<16, INV>(src, dst, a.n, Ns, magic, tw); break;
      case 8: disp_pass<8, INV>(src, dst, a.n, Ns, magic, tw); break;
      case 4: disp_pass<4, INV>(src, dst, a.n, Ns, magic, tw); break;
      case 2: disp_pass<2, INV>(src, dst, a.n, Ns, magic, tw); break;
      case 5: disp_pass<5, INV>(src, dst, a.n, Ns, magic, tw); break;
      default: disp_pass<3, INV>(src, dst, a.n, Ns, magic, tw); break;
    }
    __syncthreads();
    v2f* t = src;
    src = dst;
    dst = t;
    Ns *= R;
  }
  return src;
}

__global__ __launch_bounds__(kDispBlock) void disp_search_kernel(const DispersionArgs a) {
  extern __shared__ __align__(16) unsigned char disp_lds[];
  const int n = a.n, tid = threadIdx.x;
  v2f* z = reinterpret_cast<v2f*>(disp_lds);
  v2f* bufA = z + n;
  v2f* bufB = bufA + n;
  double* red = reinterpret_cast<double*>(bufB + n);   // 2 x (waves) partials
  const v2f* tw = reinterpret_cast<const v2f*>(a.tab);
  const v2f* t2 = tw + n;
  const v2f* t3 = t2 + (size_t)a.a2_count * (size_t)n;

  const int r = (int)(blockIdx.x / (unsigned)a.chunks), ch = (int)(blockIdx.x - (unsigned)r * (unsigned)a.chunks);
  const int c0 = ch * a.per_wg, c1 = min(a.K, c0 + a.per_wg);
  const v2f* x = reinterpret_cast<const v2f*>(a.x) + (size_t)r * (size_t)n;

  for (int i = tid; i < n; i += kDispBlock) bufA[i] = x[i];
  __syncthreads();
  const v2f* F = disp_fft<false>(bufA, bufB, a, tw);
  const float inv_n = 1.0f / (float)n;
  for (int i = tid; i < n; i += kDispBlock) z[i] = F[i] * inv_n;
  __syncthreads();

  const int b0 = a.depth_first, b1 = a.depth_first + a.depth_count;
  for (int c = c0; c < c1; c++) {
    const int i2 = c / a.a3_count, i3 = c - i2 * a.a3_count;
    const v2f* p2 = t2 + (size_t)i2 * (size_t)n;
    const v2f* p3 = t3 + (size_t)i3 * (size_t)n;
    for (int q = tid; q < n; q += kDispBlock) bufA[q] = cmul(z[q], cmul(p2[q], p3[q]));
    __syncthreads();
    const v2f* A = disp_fft<true>(bufA, bufB, a, tw);
    double s2 = 0.0, s4 = 0.0;
    for (int b = b0 + tid; b < b1; b += kDispBlock) {
      const v2f v = A[b];
      const float I = v.x * v.x + v.y * v.y;
      const float I2 = I * I;
      s2 += (double)I;
      s4 += (double)I2;
    }
    for (int m = 32; m >= 1; m >>= 1) {
      s2 += __shfl_xor(s2, m, 64);
      s4 += __shfl_xor(s4, m, 64);
    }
    if ((tid & 63) == 0) red[2 * (tid >> 6)] = s2, red[2 * (tid >> 6) + 1] = s4;
    __syncthreads();   // (every read of A lies in front of it: the next candidate may write either buffer)
    if (tid == 0) {
      double t2s = red[0], t4s = red[1];
      for (int w = 1; w < kDispBlock / 64; w++) t2s += red[2 * w], t4s += red[2 * w + 1];
      a.row_sums[(size_t)r * (size_t)a.K + (size_t)c] = make_double2(t2s, t4s);
    }
    // red is next written behind the next candidate's barriers, which thread 0 reaches only after these reads
  }
}

__global__ __launch_bounds__(kDispBlock) void disp_rowsum_kernel(const DispersionArgs a) {
  const int c = (int)(blockIdx.x * kDispBlock + threadIdx.x);
  if (c >= a.K) return;
  double s2 = 0.0, s4 = 0.0;
  for (int r = 0; r < a.rows; r++) {
    const double2 v = a.row_sums[(size_t)r * (size_t)a.K + (size_t)c];
    s2 += v.x;
    s4 += v.y;
  }
  a.sums[c] = make_double2(s2, s4);
}

__global__ __launch_bounds__(kDispBlock) void disp_best_kernel(const DispersionArgs a) {
  __shared__ double s_m[kDispBlock];
  __shared__ int s_c[kDispBlock];
  const int tid = threadIdx.x;
  double bm = 0.0;
  int bc = -1;
  for (int c = tid; c < a.K; c += kDispBlock) {
    const double2 v = a.sums[c];
    const double m = v.x == 0.0 ? 0.0 : v.y / (v.x * v.x);
    if (isfinite(m) && (bc < 0 || m > bm)) bm = m, bc = c;
  }
  s_m[tid] = bm, s_c[tid] = bc;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < kDispBlock; t++) {
      const int c = s_c[t];
      if (c >= 0 && (bc < 0 || s_m[t] > bm || (s_m[t] == bm && c < bc))) bm = s_m[t], bc = c;
    }
    s_m[0] = bm, s_c[0] = bc;
    DispBest o;
    o.index = bc;
    o.i2 = bc < 0 ? -1 : bc / a.a3_count;
    o.i3 = bc < 0 ? -1 : bc - o.i2 * a.a3_count;
    o.a2 = bc < 0 ? 0.0 : a.a2_first + (double)o.i2 * a.a2_step;
    o.a3 = bc < 0 ? 0.0 : a.a3_first + (double)o.i3 * a.a3_step;
    o.metric = bc < 0 ? 0.0 : bm;
    *a.best = o;
  }
  __syncthreads();
  if (!a.cos_sin) return;
  bc = s_c[0];
  const int i2 = bc < 0 ? 0 : bc / a.a3_count, i3 = bc < 0 ? 0 : bc - i2 * a.a3_count;
  const double a2 = a.a2_first + (double)i2 * a.a2_step, a3 = a.a3_first + (double)i3 * a.a3_step;
  for (int q = tid; q < a.n; q += kDispBlock) {
    float2 o = make_float2(0.f, 0.f);
    if (bc >= 0) {
      const double x = disp_x(q, a.n);
      double s, c;
      sincos(a2 * (x * x) + a3 * (x * x * x), &s, &c);
      o = make_float2((float)c, (float)s);
    }
    a.cos_sin[q] = o;
  }
}

LdsGrant g_disp_lds;

}  // namespace

hipError_t launch_dispersion(const DispersionArgs& a, hipStream_t st) {
  if (a.rows < 1 || a.K < 1 || a.per_wg < 1 || a.chunks < 1 || a.workgroups < 1 || a.workgroups > 0x7fffffffLL || a.npass < 1 || a.depth_count < 1 ||
      a.depth_first < 0 || a.depth_first + a.depth_count > a.n || !a.x || !a.tab || !a.row_sums || !a.sums || !a.best)
    return hipErrorInvalidValue;
  if (hipError_t e = g_disp_lds.ensure(disp_search_kernel, a.lds_bytes); e != hipSuccess) return e;
  const size_t entries = dispersion_tab_entries(a.n, a.a2_count, a.a3_count);
  const size_t tab_blocks = (entries + kDispBlock - 1) / kDispBlock;
  hipLaunchKernelGGL(disp_table_kernel, dim3((unsigned)(tab_blocks < 4096 ? tab_blocks : 4096)), dim3(kDispBlock), 0, st, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(disp_search_kernel, dim3((unsigned)a.workgroups), dim3(kDispBlock), a.lds_bytes, st, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(disp_rowsum_kernel, dim3((unsigned)((a.K + kDispBlock - 1) / kDispBlock)), dim3(kDispBlock), 0, st, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(disp_best_kernel, dim3(1), dim3(kDispBlock), 0, st, a);
  return hipGetLastError();
}

}  // namespace fdoct
