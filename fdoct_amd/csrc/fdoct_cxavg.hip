// fdoct_cxavg.hip -- the kernels of include/fdoct_cxavg.h: the coherent average of repeated complex B-scans -- the complex mean after
// the repeats' common phase is taken out, its modulus, the mean of the moduli and their ratio (the header states the quantity;
// tests/cxavg_model.py restates it in numpy).
//
// One workgroup of 256 threads takes one (group, A-scan) at a time -- a capped grid looping over them: the N rows of depths pairs
// that are that A-scan's repeats, `ascans x depths` pairs apart.  Depth b of every row belongs to thread b mod 256 in every pass:
// 8-byte loads, consecutive lanes on consecutive depths (rows are only 8-byte aligned where depths is odd or the pointer is offset
// by a pair, so nothing wider is tried).
//   cxavg_reg_kernel<NR, CPT>  the register form: N <= NR repeats of depths <= 256 CPT, NR CPT = kCxaRegPairs.  The thread
//                   requests its CPT pairs of all N rows before it uses any -- one read of the pairs, all of it in flight at once --
//                   and keeps them: the alignment sums, the phasors and the outputs come from registers.  Every index into the
//                   pairs is a compile-time one; the ref's pair is picked by a chain of selects.
//   cxavg_stream_kernel        everything larger: the alignment sum reads the alignment range of the row and of the ref's; the
//                   average reads the rows again.
//   alignment       (align 1) per repeat a strided partial of X_n conj(X_ref) per thread, a butterfly over the wave's 64 lanes, the
//                   four waves' sums to LDS; after one barrier they are added in increasing wave and U[n] = conj(C) / |C| is
//                   formed.  (align 2) U[n] is read from the phasors the two kernels below left.  (align 0) U = 1.
//   average         per depth, Z += U_n X_n and M += |X_n| in increasing n, then the outputs asked for: 8 or 4 bytes a lane,
//                   consecutive lanes on consecutive depths.  What nothing reads is skipped by branches the whole grid takes alike.
//
// cxavg_rows_kernel and cxavg_phasors_kernel, in front with align 2: one workgroup per (group, repeat, A-scan) -- a capped grid
// looping over them -- leaves fdoct_boxtile.h's bulk sum of X_n conj(X_ref) over the alignment range; one thread per (group,
// repeat) then adds the A-scans' sums in increasing r and leaves conj(C) / |C| (1 where C is 0, and for the ref).
#include "fdoct_cxavg_kernels.h"

namespace fdoct {

namespace {

constexpr int kCxaWaves = kCxaBlock / 64;

// The sum of s over the wave's 64 lanes, on every lane: partners add the same two values, so every lane holds the same bits.
__device__ __forceinline__ float2 cxa_wave_sum(float2 s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s.x += __shfl_xor(s.x, off, 64), s.y += __shfl_xor(s.y, off, 64);
  return s;
}

// The four waves' sums of one repeat, in increasing wave.
__device__ __forceinline__ float2 cxa_waves_sum(const float2 (&w)[kCxaWaves]) {
  float2 c = make_float2(0.f, 0.f);
#pragma unroll
  for (int i = 0; i < kCxaWaves; i++) c.x += w[i].x, c.y += w[i].y;
  return c;
}

// One depth's outputs from S = sum_n U_n X_n (zr, zi) and M = sum_n |X_n|.
__device__ __forceinline__ void cxa_store(const CxavgArgs& a, long long o, float zr, float zi, float m, float fn) {
  const float mr = zr / fn, mi = zi / fn;
  if (a.out_mean) a.out_mean[o] = make_float2(mr, mi);
  if (a.out_mag) a.out_mag[o] = hypotf(mr, mi);
  if (a.out_incoh) a.out_incoh[o] = m / fn;
  if (a.out_coh) a.out_coh[o] = m == 0.f ? 0.f : hypotf(zr, zi) / m;
}

__global__ __launch_bounds__(kBoxBulkBlock) void cxavg_rows_kernel(const CxavgArgs a) {
  __shared__ float2 part[kBoxBulkBlock];
  const int N = a.repeats;
  const long long rows = (long long)a.groups * N * a.ascans;
  const long long pixels = (long long)a.ascans * a.depths;
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const long long gn = row / a.ascans;
    const int r = (int)(row - gn * a.ascans);
    const int g = (int)(gn / N), n = (int)(gn - (long long)g * N);
    if (n == a.ref) continue;                  // the whole workgroup alike
    const float2* const x0 = a.x + (long long)g * a.stride * pixels + (long long)r * a.depths + a.first;
    const float2 C = box_bulk_sum(x0 + (long long)a.ref * pixels, x0 + (long long)n * pixels, a.count, part);   // X_n conj(X_ref)
    if (threadIdx.x == 0) a.rows[row] = C;
  }
}

__global__ __launch_bounds__(kCxaBlock) void cxavg_phasors_kernel(const CxavgArgs a) {
  const long long i = (long long)blockIdx.x * kCxaBlock + threadIdx.x;
  if (i >= (long long)a.groups * a.repeats) return;
  const int n = (int)(i % a.repeats);
  float2 u = make_float2(1.f, 0.f);
  if (n != a.ref) {
    const float2* const c = a.rows + i * a.ascans;
    float2 s = make_float2(0.f, 0.f);
    for (int r = 0; r < a.ascans; r++) s.x += c[r].x, s.y += c[r].y;
    u = box_phasor(s, true);
  }
  a.phasors[i] = u;
}

template <int NR, int CPT>
__global__ __launch_bounds__(kCxaBlock) void cxavg_reg_kernel(const CxavgArgs a) {
  static_assert(NR * CPT == kCxaRegPairs, "the register budget");
  __shared__ float2 wpart[NR][kCxaWaves];
  const int N = a.repeats, D = a.depths, tid = (int)threadIdx.x;
  const long long pixels = (long long)a.ascans * D;
  const long long items = (long long)a.groups * a.ascans;
  const bool need_z = a.out_mean || a.out_mag || a.out_coh, need_m = a.out_incoh || a.out_coh;
  const bool corr = a.align == kCxaAlignRow;
  const int last = a.first + a.count;
  const float fn = (float)N;

  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const int g = (int)(item / a.ascans), r = (int)(item - (long long)g * a.ascans);
    const float2* const x0 = a.x + (long long)g * a.stride * pixels + (long long)r * D;   // repeat n's row: x0 + n pixels
    float2 v[NR][CPT];
#pragma unroll
    for (int n = 0; n < NR; n++) {
#pragma unroll
      for (int c = 0; c < CPT; c++) {
        const int b = tid + c * kCxaBlock;
        v[n][c] = n < N && b < D ? x0[(long long)n * pixels + b] : make_float2(0.f, 0.f);
      }
    }
    float2 un[NR];
#pragma unroll
    for (int n = 0; n < NR; n++) un[n] = make_float2(1.f, 0.f);
    if (corr) {
      float2 s[NR];
#pragma unroll
      for (int n = 0; n < NR; n++) s[n] = make_float2(0.f, 0.f);
#pragma unroll
      for (int c = 0; c < CPT; c++) {
        const int b = tid + c * kCxaBlock;
        float2 w = v[0][c];                    // the ref's pair
#pragma unroll
        for (int k = 1; k < NR; k++) w = k == a.ref ? v[k][c] : w;
        if (b >= a.first && b < last) {
#pragma unroll
          for (int n = 0; n < NR; n++) s[n].x += v[n][c].x * w.x + v[n][c].y * w.y, s[n].y += v[n][c].y * w.x - v[n][c].x * w.y;
        }
      }
#pragma unroll
      for (int n = 0; n < NR; n++) {
        if (n < N) {
          s[n] = cxa_wave_sum(s[n]);
          if ((tid & 63) == 0) wpart[n][tid >> 6] = s[n];
        }
      }
      __syncthreads();
#pragma unroll
      for (int n = 0; n < NR; n++)
        if (n < N && n != a.ref) un[n] = box_phasor(cxa_waves_sum(wpart[n]), true);
      __syncthreads();                         // wpart is the next item's
    } else if (a.align == kCxaAlignFrame) {
#pragma unroll
      for (int n = 0; n < NR; n++)
        if (n < N && n != a.ref) un[n] = a.phasors[(long long)g * N + n];
    }

    const long long o0 = ((long long)g * a.ascans + r) * (long long)D;
#pragma unroll
    for (int c = 0; c < CPT; c++) {
      const int b = tid + c * kCxaBlock;
      if (b >= D) continue;
      float zr = 0.f, zi = 0.f, m = 0.f;
#pragma unroll
      for (int n = 0; n < NR; n++) {
        if (n < N) {
          const float2 x = v[n][c];
          if (need_z) zr += x.x * un[n].x - x.y * un[n].y, zi += x.x * un[n].y + x.y * un[n].x;
          if (need_m) m += sqrtf(x.x * x.x + x.y * x.y);
        }
      }
      cxa_store(a, o0 + b, zr, zi, m, fn);
    }
  }
}

__global__ __launch_bounds__(kCxaBlock) void cxavg_stream_kernel(const CxavgArgs a) {
  __shared__ float2 u[kCxaMaxRepeats];
  __shared__ float2 wpart[kCxaMaxRepeats][kCxaWaves];
  const int N = a.repeats, D = a.depths, tid = (int)threadIdx.x;
  const long long pixels = (long long)a.ascans * D;
  const long long items = (long long)a.groups * a.ascans;
  const bool need_z = a.out_mean || a.out_mag || a.out_coh, need_m = a.out_incoh || a.out_coh;
  const bool corr = a.align == kCxaAlignRow;
  const int last = a.first + a.count;
  const float fn = (float)N;

  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const int g = (int)(item / a.ascans), r = (int)(item - (long long)g * a.ascans);
    const float2* const x0 = a.x + (long long)g * a.stride * pixels + (long long)r * D;   // repeat n's row: x0 + n pixels
    const float2* const xr = x0 + (long long)a.ref * pixels;

    if (corr) {
      for (int n = 0; n < N; n++) {
        if (n == a.ref) continue;
        const float2* const xn = x0 + (long long)n * pixels;
        float2 s = make_float2(0.f, 0.f);
#pragma unroll 4
        for (int b = a.first + tid; b < last; b += kCxaBlock) {
          const float2 v = xn[b], w = xr[b];
          s.x += v.x * w.x + v.y * w.y, s.y += v.y * w.x - v.x * w.y;
        }
        s = cxa_wave_sum(s);
        if ((tid & 63) == 0) wpart[n][tid >> 6] = s;
      }
      __syncthreads();
    }
    if (tid < N) {
      float2 un = make_float2(1.f, 0.f);
      if (tid != a.ref && corr) un = box_phasor(cxa_waves_sum(wpart[tid]), true);
      if (tid != a.ref && a.align == kCxaAlignFrame) un = a.phasors[(long long)g * N + tid];
      u[tid] = un;
    }
    __syncthreads();

    const long long o0 = ((long long)g * a.ascans + r) * (long long)D;
    for (int b = tid; b < D; b += kCxaBlock) {
      float zr = 0.f, zi = 0.f, m = 0.f;
#pragma unroll 4
      for (int n = 0; n < N; n++) {
        const float2 v = x0[(long long)n * pixels + b];
        if (need_z) {
          const float2 un = u[n];
          zr += v.x * un.x - v.y * un.y, zi += v.x * un.y + v.y * un.x;
        }
        if (need_m) m += sqrtf(v.x * v.x + v.y * v.y);
      }
      cxa_store(a, o0 + b, zr, zi, m, fn);
    }
    __syncthreads();                            // u and wpart are the next item's
  }
}

template <int NR>
hipError_t launch_reg(const CxavgArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((cxavg_reg_kernel<NR, kCxaRegPairs / NR>), dim3((unsigned)a.blocks), dim3(kCxaBlock), 0, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_cxavg(const CxavgArgs& a, hipStream_t st) {
  if (!a.x || a.blocks < 1 || a.groups < 1 || a.ascans < 1 || a.depths < 1) return hipErrorInvalidValue;
  if (a.repeats < kCxaMinRepeats || a.repeats > kCxaMaxRepeats || a.stride < 1 || a.stride > a.repeats || a.ref < 0 || a.ref >= a.repeats)
    return hipErrorInvalidValue;
  if (!a.out_mean && !a.out_mag && !a.out_incoh && !a.out_coh) return hipErrorInvalidValue;
  if (a.align != kCxaAlignNone && a.align != kCxaAlignRow && a.align != kCxaAlignFrame) return hipErrorInvalidValue;
  if (a.align != kCxaAlignNone && (a.first < 0 || a.count < 1 || a.count > a.depths - a.first)) return hipErrorInvalidValue;
  if (a.align == kCxaAlignFrame && (!a.rows || !a.phasors || a.row_blocks < 1 || a.phasor_blocks < 1)) return hipErrorInvalidValue;
  const bool reg = a.form == kCxaFormRegister;
  if (!reg && a.form != kCxaFormStreaming) return hipErrorInvalidValue;
  if (reg && (a.slots < 2 || a.slots != cxavg_register_slots(a.repeats, a.depths))) return hipErrorInvalidValue;   // every pair has its register
  if (a.align == kCxaAlignFrame) {
    hipLaunchKernelGGL(cxavg_rows_kernel, dim3((unsigned)a.row_blocks), dim3(kBoxBulkBlock), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(cxavg_phasors_kernel, dim3((unsigned)a.phasor_blocks), dim3(kCxaBlock), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (reg) return a.slots == 2 ? launch_reg<2>(a, st) : a.slots == 4 ? launch_reg<4>(a, st) : a.slots == 8 ? launch_reg<8>(a, st) : launch_reg<16>(a, st);
  hipLaunchKernelGGL(cxavg_stream_kernel, dim3((unsigned)a.blocks), dim3(kCxaBlock), 0, st, a);
  return hipGetLastError();
}

}  // namespace fdoct
