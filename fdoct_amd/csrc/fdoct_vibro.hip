// fdoct_vibro.hip -- the kernels of include/fdoct_vibro.h: a pixel's phase followed through the frames (the header states the
// quantity; tests/vibro_model.py restates it in numpy).
//
// Time is cut into `chunks` of chunk_steps steps; chunk c owns the samples t in (c chunk_steps, min((c + 1) chunk_steps, T - 1)]
// and reads the frame before them too, so adjacent chunks share one frame.  Sample 0, where phi is 0, belongs to no chunk: it adds
// nothing to a sum of phi, and the sums of the table alone take it from `head`.
//
// vibro_setup_kernel (nfreq > 0).  One wave per (chunk, slot), slot = a frequency or, last, the window alone: the table entries
//   w[t] (cos, sin)(2 pi nu t) of the chunk's samples in double (sincospi, cospi), written to `tab`, and their sums E and F (F
//   weighted by t) -- a strided partial per lane, then a shuffle tree.  vibro_totals_kernel adds those over the chunks, in order.
// vibro_ref_kernel (ref).  One wave per (t, r): the float sum of the reference range -- a strided partial per lane, a shuffle
//   tree -- and the unit phasor conj(C) / |C|, or (1, 0) where |C| = 0, to `refph`.
// vibro_series_kernel.  One lane per pixel, a wave's lanes on 64 consecutive depths of one A-scan, so every time step is one
//   coalesced 512-byte read; the previous Y stays in registers.  Per step: Y = X u (the row's phasor), the lag product and atan2f
//   in float, the loads of four frames issued ahead of their use; phi and the sums S1 = sum phi, S2 = sum phi^2, St = sum t phi,
//   sum |X|^2, and sum w phi cos, sum w phi sin per
//   frequency in double, phi counted from the chunk's own start.  The table entry of (j, t) is the same for every lane: the wave's
//   index goes through readfirstlane and the table pointer is restrict, so the reads are uniform (DESIGN.md 3.4k says what the
//   compiler makes of them).  With one chunk the lane finishes its pixel; otherwise the sums go to `part`, [chunk][sum][pixel].
// vibro_combine_kernel (chunks > 1).  One lane per pixel, in chunk order: with off = the steps' total before chunk c,
//       sum phi     += S1_c + n_c off
//       sum phi^2   += S2_c + 2 off S1_c + n_c off^2
//       sum t phi   += St_c + off (sum of t over the chunk)
//       sum w phi e += Sc_c + off E_c
//   then the finish.
// The finish.  mean = S1 / T.  detrend 0: alpha = mean, beta = 0, RSS = S2 - S1 mean.  detrend 1, with t counted from its mean
//   tbar = (T - 1) / 2: Stc = St - tbar S1, beta = Stc / (T (T^2 - 1) / 12), alpha = mean - beta tbar, RSS = S2 - S1 mean - beta
//   Stc.  sum w phi' e = sum w phi e - alpha G0 - beta G1.  The mask, scale, the stores.
// Every order above is a function of (T, ascans, depths, chunk_steps): no atomics, no dependence on the grid.
#include "fdoct_vibro_kernels.h"

namespace fdoct {

namespace {

struct VibSums {
  double S1, S2, St, tot, P;
  double Sc[kVibMaxFreq], Ss[kVibMaxFreq];
};

// Chunk c reads frames t0 .. t1 and owns samples t0 + 1 .. t1.
__device__ __forceinline__ void vib_chunk(const VibroArgs& a, int c, int* t0, int* t1) {
  *t0 = c * a.chunk_steps;
  const int e = *t0 + a.chunk_steps;
  *t1 = e < a.T - 1 ? e : a.T - 1;
}

__device__ __forceinline__ double2 vib_entry(const VibroArgs& a, int slot, int t) {
  const double w = (a.window == 0 || a.T <= 2) ? 1.0 : 0.5 - 0.5 * cospi(2.0 * (double)t / (double)(a.T - 1));
  if (slot == a.nfreq) return make_double2(w, 0.0);
  double s, c;
  sincospi(2.0 * a.freq[slot] * (double)t, &s, &c);
  return make_double2(w * c, w * s);
}

__global__ __launch_bounds__(64) void vibro_setup_kernel(const VibroArgs a) {
  const int slots = a.nfreq + 1;
  const int c = (int)blockIdx.x / slots, slot = (int)blockIdx.x - c * slots;
  int t0, t1;
  vib_chunk(a, c, &t0, &t1);
  double2 E = make_double2(0.0, 0.0), F = make_double2(0.0, 0.0);
  for (int t = t0 + 1 + (int)threadIdx.x; t <= t1; t += 64) {
    const double2 v = vib_entry(a, slot, t);
    if (slot < a.nfreq) a.tab[(size_t)slot * a.T + t] = v;
    E.x += v.x, E.y += v.y;
    F.x += (double)t * v.x, F.y += (double)t * v.y;
  }
  for (int off = 32; off > 0; off >>= 1) {
    E.x += __shfl_down(E.x, off), E.y += __shfl_down(E.y, off);
    F.x += __shfl_down(F.x, off), F.y += __shfl_down(F.y, off);
  }
  if (threadIdx.x == 0) {
    a.cst[((size_t)c * slots + slot) * 2] = E;
    a.cst[((size_t)c * slots + slot) * 2 + 1] = F;
    if (c == 0) {
      const double2 v = vib_entry(a, slot, 0);
      a.head[slot] = v;
      if (slot < a.nfreq) a.tab[(size_t)slot * a.T] = v;
    }
  }
}

__global__ __launch_bounds__(64) void vibro_totals_kernel(const VibroArgs a) {
  const int slots = a.nfreq + 1, slot = (int)threadIdx.x;
  if (slot >= slots) return;
  double2 g0 = a.head[slot], g1 = make_double2(0.0, 0.0);
  for (int c = 0; c < a.chunks; c++) {
    const double2 E = a.cst[((size_t)c * slots + slot) * 2], F = a.cst[((size_t)c * slots + slot) * 2 + 1];
    g0.x += E.x, g0.y += E.y;
    g1.x += F.x, g1.y += F.y;
  }
  a.glob[2 * slot] = g0;
  a.glob[2 * slot + 1] = g1;
}

__global__ __launch_bounds__(kVibBlock) void vibro_ref_kernel(const VibroArgs a) {
  const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const long long rows = (long long)a.T * a.ascans;
  for (long long row = (long long)blockIdx.x * kVibWaves + wave; row < rows; row += (long long)gridDim.x * kVibWaves) {
    const float2* x = a.x + row * a.depths + a.ref_first;
    float2 s = make_float2(0.f, 0.f);
    for (int b = lane; b < a.ref_count; b += 64) {
      const float2 v = x[b];
      s.x += v.x, s.y += v.y;
    }
    for (int off = 32; off > 0; off >>= 1) s.x += __shfl_down(s.x, off), s.y += __shfl_down(s.y, off);
    if (lane == 0) {  // what the series pass multiplies by: conj(C) / |C|, or 1 where C is 0
      const float m = hypotf(s.x, s.y);
      a.refph[row] = m == 0.f ? make_float2(1.f, 0.f) : make_float2(s.x / m, -s.y / m);
    }
  }
}

__device__ __forceinline__ void vib_finish(const VibroArgs& a, int pix, const VibSums& s) {
  const double n = (double)a.T;
  const double power = s.P / n;
  const bool masked = a.min_power > 0.0 && power < a.min_power;
  const double mean = s.S1 / n;
  double alpha = mean, beta = 0.0, rss = s.S2 - s.S1 * mean;
  if (a.detrend) {
    const double tbar = 0.5 * (n - 1.0), stt = n * (n * n - 1.0) / 12.0;
    const double stc = s.St - tbar * s.S1;
    beta = stc / stt;
    alpha = mean - beta * tbar;
    rss -= beta * stc;
  }
  if (rss < 0.0) rss = 0.0;   // (a NaN stays one)
  if (a.out_power) a.out_power[pix] = (float)power;
  if (a.out_drift) a.out_drift[pix] = masked ? 0.f : (float)(a.scale * s.tot);
  if (a.out_rms) a.out_rms[pix] = masked ? 0.f : (float)(fabs(a.scale) * sqrt(rss / n));
  if (a.out_amp) {
    const double k = 2.0 * a.scale / a.glob[2 * a.nfreq].x;
#pragma unroll
    for (int j = 0; j < kVibMaxFreq; j++) {
      if (j < a.nfreq) {
        const double2 g0 = a.glob[2 * j], g1 = a.glob[2 * j + 1];
        const double re = s.Sc[j] - alpha * g0.x - beta * g1.x;
        const double im = s.Ss[j] - alpha * g0.y - beta * g1.y;   // e^(-i x) = cos x - i sin x: the sign goes on below
        a.out_amp[(size_t)j * a.pixels + pix] = masked ? make_float2(0.f, 0.f) : make_float2((float)(k * re), (float)(-(k * im)));
      }
    }
  }
}

__device__ __forceinline__ float2 vib_turn(float2 x, float2 u) { return make_float2(x.x * u.x - x.y * u.y, x.x * u.y + x.y * u.x); }

// One step of one pixel: frame t's pair x and its row's phasor u behind the previous Y.
__device__ __forceinline__ void vib_step(const VibroArgs& a, const double2* __restrict__ tab, int t, float2 x, float2 u, VibSums& s, double& phi, float2& yp) {
  s.P += (double)(x.x * x.x + x.y * x.y);
  const float2 y = a.use_ref ? vib_turn(x, u) : x;
  const float re = y.x * yp.x + y.y * yp.y, im = y.y * yp.x - y.x * yp.y;   // Y[t] conj(Y[t - 1])
  phi += (double)atan2f(im, re);
  s.S1 += phi;
  s.S2 += phi * phi;
  s.St += (double)t * phi;
#pragma unroll
  for (int j = 0; j < kVibMaxFreq; j++) {
    if (j < a.nfreq) {
      const double2 e = tab[(size_t)j * a.T + t];
      s.Sc[j] += e.x * phi, s.Ss[j] += e.y * phi;
    }
  }
  yp = y;
}

__global__ __launch_bounds__(kVibBlock) void vibro_series_kernel(const VibroArgs a) {
  const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const double2* __restrict__ tab = a.tab;
  const float2* __restrict__ refph = a.refph;
  const size_t stride = (size_t)a.pixels;
  const int nk = vibro_sums(a.nfreq);
  for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const int c = (int)(item / a.groups);
    const long long tile = (item - (long long)c * a.groups) * kVibWaves + wave;
    if (tile >= a.tiles) continue;
    const int r = (int)(tile / a.tiles_d), b = (int)(tile - (long long)r * a.tiles_d) * 64 + lane;
    if (b >= a.depths) continue;
    const int pix = r * a.depths + b;
    int t0, t1;
    vib_chunk(a, c, &t0, &t1);
    VibSums s = {};
    const float2* xp = a.x + (size_t)t0 * stride + pix;
    float2 x = *xp;
    if (c == 0) s.P += (double)(x.x * x.x + x.y * x.y);
    float2 yp = a.use_ref ? vib_turn(x, refph[(size_t)t0 * a.ascans + r]) : x;
    double phi = 0.0;
    int t = t0 + 1;
    for (; t + kVibAhead - 1 <= t1; t += kVibAhead) {   // kVibAhead frames' loads in flight before the first of them is used
      float2 xs[kVibAhead], us[kVibAhead];
#pragma unroll
      for (int k = 0; k < kVibAhead; k++) {
        xs[k] = xp[(size_t)(k + 1) * stride];
        us[k] = a.use_ref ? refph[(size_t)(t + k) * a.ascans + r] : make_float2(1.f, 0.f);
      }
#pragma unroll
      for (int k = 0; k < kVibAhead; k++) vib_step(a, tab, t + k, xs[k], us[k], s, phi, yp);
      xp += (size_t)kVibAhead * stride;
    }
    for (; t <= t1; t++) {
      xp += stride;
      vib_step(a, tab, t, *xp, a.use_ref ? refph[(size_t)t * a.ascans + r] : make_float2(1.f, 0.f), s, phi, yp);
    }
    s.tot = phi;
    if (a.chunks == 1) {
      vib_finish(a, pix, s);
    } else {
      double* p = a.part + (size_t)c * nk * stride + pix;
      p[0] = s.S1, p[stride] = s.S2, p[2 * stride] = s.St, p[3 * stride] = s.tot, p[4 * stride] = s.P;
#pragma unroll
      for (int j = 0; j < kVibMaxFreq; j++) {
        if (j < a.nfreq) p[(size_t)(kVibBaseSums + 2 * j) * stride] = s.Sc[j], p[(size_t)(kVibBaseSums + 2 * j + 1) * stride] = s.Ss[j];
      }
    }
  }
}

__global__ __launch_bounds__(kVibBlock) void vibro_combine_kernel(const VibroArgs a) {
  const int pix = (int)(blockIdx.x * kVibBlock + threadIdx.x);
  if (pix >= a.pixels) return;
  const size_t stride = (size_t)a.pixels;
  const int nk = vibro_sums(a.nfreq), slots = a.nfreq + 1;
  VibSums s = {};
  double off = 0.0;
  for (int c = 0; c < a.chunks; c++) {
    int t0, t1;
    vib_chunk(a, c, &t0, &t1);
    const double nc = (double)(t1 - t0);
    const double sum_t = (double)((long long)(t1 - t0) * (t0 + 1 + t1) / 2);   // t0 + 1 + ... + t1
    const double* p = a.part + (size_t)c * nk * stride + pix;
    const double S1 = p[0];
    s.S1 += S1 + nc * off;
    s.S2 += (p[stride] + (2.0 * off) * S1) + (nc * off) * off;
    s.St += p[2 * stride] + off * sum_t;
    s.P += p[4 * stride];
#pragma unroll
    for (int j = 0; j < kVibMaxFreq; j++) {
      if (j < a.nfreq) {
        const double2 E = a.cst[((size_t)c * slots + j) * 2];
        s.Sc[j] += p[(size_t)(kVibBaseSums + 2 * j) * stride] + off * E.x;
        s.Ss[j] += p[(size_t)(kVibBaseSums + 2 * j + 1) * stride] + off * E.y;
      }
    }
    off += p[3 * stride];
  }
  s.tot = off;
  vib_finish(a, pix, s);
}

}  // namespace

hipError_t launch_vibro(const VibroArgs& a, hipStream_t st) {
  if (!a.x || a.T < 2 || a.pixels < 1 || a.chunk_steps < 1 || a.chunks < 1 || a.series_blocks < 1 || a.nfreq < 0 || a.nfreq > kVibMaxFreq)
    return hipErrorInvalidValue;
  if ((a.use_ref && (!a.refph || a.ref_blocks < 1 || a.ref_count < 1)) || (a.chunks > 1 && (!a.part || a.combine_blocks < 1)) ||
      (a.nfreq > 0 && (!a.tab || !a.cst || !a.head || !a.glob)))
    return hipErrorInvalidValue;
  if (a.nfreq > 0) {
    hipLaunchKernelGGL(vibro_setup_kernel, dim3((unsigned)(a.chunks * (a.nfreq + 1))), dim3(64), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(vibro_totals_kernel, dim3(1), dim3(64), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (a.use_ref) {
    hipLaunchKernelGGL(vibro_ref_kernel, dim3((unsigned)a.ref_blocks), dim3(kVibBlock), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(vibro_series_kernel, dim3((unsigned)a.series_blocks), dim3(kVibBlock), 0, st, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (a.chunks > 1) {
    hipLaunchKernelGGL(vibro_combine_kernel, dim3((unsigned)a.combine_blocks), dim3(kVibBlock), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace fdoct
