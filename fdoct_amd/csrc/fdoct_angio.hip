// fdoct_angio.hip -- the kernels of include/fdoct_angio.h: motion contrast of repeated B-scans -- speckle variance, amplitude
// decorrelation, complex decorrelation with bulk-motion correction, and the mean power (the header states the quantity;
// tests/angio_model.py restates it in numpy).
//
// The tile, the window pass and the bulk sum are fdoct_boxtile.h's; what is this file's own:
//
// angio_kernel.  Per tile of 16 A-scans x 64 depth bins of one group, staged pixel i of the halo tile belongs to thread i mod 256
// for the whole tile: at most K = 10 of them a thread (K = 4 or 6 where the halo tile holds no more than 1024 or 1536 pixels; the
// three instantiations do the same arithmetic).  Per staged pixel the thread keeps in registers
//     the previous frame's pair, sum_n T'[n] (re, im), sum_n (I_n + I_{n+1}) / 2, sum_n I_n, and Welford's (mean, M2) of I,
// so every frame of the tile is loaded once -- 8-byte loads, consecutive lanes on consecutive depths of the staged row -- and frame
// n + 2 is requested before pair n's window passes.  Pixels of the halo outside the image are not loaded.
//   per pair n   (out_decorr only) A_n A_{n+1} and (I_n + I_{n+1}) / 2 go to two planes of LDS; the window pass gives their box
//                sums at the thread's four output pixels, whose ratio Q_n is added into a register of the output pixel.
//   at the end   the running sums go through the same two planes -- (T' re, T' im), then (the half sums, sum I), then M2 / N --
//                one window pass each, then cnt, the mask, the stores: 4 bytes a lane, consecutive lanes on consecutive depths.
//   1 x 1        the staged tile is the output tile and a thread's staged pixels are its output pixels: no plane, no barrier.
// Two staged planes and two planes of depth sums are all of the LDS: 35 KiB at the 16 x 16 window.  What nothing reads is skipped by
// branches the whole grid takes alike, and a group's tiles read that group's frames only.
//
// angio_bulk_kernel, in front of it where bulk is set and out_cdecorr is asked for: one workgroup per (group, pair, A-scan) -- a
// capped grid looping over them -- leaves conj(B) / |B| (1 where B is 0), B the sum of X[n + 1] conj(X[n]) over the bulk range, for
// the stage to turn T by.
#include "fdoct_angio_kernels.h"
#include "fdoct_kernels.h"

namespace fdoct {

namespace {

__device__ __forceinline__ float ang_power(float2 x) { return x.x * x.x + x.y * x.y; }

__global__ __launch_bounds__(kBoxBulkBlock) void angio_bulk_kernel(const AngioArgs a) {
  __shared__ float2 part[kBoxBulkBlock];
  const int pairs = a.repeats - 1;
  const long long rows = (long long)a.groups * pairs * a.ascans;
  const long long pixels = (long long)a.ascans * a.depths;
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const long long gn = row / a.ascans;
    const int r = (int)(row - gn * a.ascans);
    const int g = (int)(gn / pairs), n = (int)(gn - (long long)g * pairs);
    const float2* x1 = a.x + ((long long)g * a.repeats + n) * pixels + (long long)r * a.depths + a.bulk_first;
    const float2 B = box_bulk_sum(x1, x1 + pixels, a.bulk_count, part);
    if (threadIdx.x == 0) a.bulk[row] = box_phasor(B, true);   // what the stage multiplies by
  }
}

// The box sums of a thread's staged values v0 (and, with `two`, v1) at its four output pixels: o[0], o[1].  Through the planes and
// the window pass -- or, with the 1 x 1 window (`unit`), where the staged tile is the output tile and staged pixel k of a thread
// is its output pixel k, without them: the same two additions from 0 a one-term depth sum and a one-term row sum make.
template <int K>
__device__ __forceinline__ void ang_box(bool unit, const float (&v0)[K], const float (&v1)[K], float* planes, float* sums, int sr, int sw, int wa, int wd,
                                        bool two, float (&o)[kAngPlanes][kBoxOwn]) {
  static_assert(K >= kBoxOwn, "the 1 x 1 window's four output pixels are the first four staged ones");
  if (unit) {
#pragma unroll
    for (int j = 0; j < kBoxOwn; j++) o[0][j] = 0.f + (0.f + v0[j]), o[1][j] = two ? 0.f + (0.f + v1[j]) : 0.f;
    return;
  }
  const int ns = sr * sw;
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int i = (int)threadIdx.x + k * kBoxBlock;
    if (i < ns) {
      planes[i] = v0[k];
      if (two) planes[ns + i] = v1[k];
    }
  }
  box_window<kAngPlanes>(planes, sums, sr, sw, wa, wd, two ? 2 : 1, o);
}

template <int K>
__global__ __launch_bounds__(kBoxBlock) void angio_kernel(const AngioArgs a) {
  extern __shared__ __align__(16) float ang_lds[];
  const int sr = box_staged_rows(a.wa), sw = box_staged_depths(a.wd), ns = sr * sw;
  float* const planes = ang_lds;                  // two planes of the staged tile: sr x sw each
  float* const sums = planes + kAngPlanes * ns;   // their depth sums: sr x 64 each
  const int N = a.repeats, tid = (int)threadIdx.x;
  const long long pixels = (long long)a.ascans * a.depths;
  const bool need_var = a.out_var != nullptr, need_dec = a.out_decorr != nullptr, need_cd = a.out_cdecorr != nullptr;
  const bool need_pow = a.out_power != nullptr || a.min_power > 0.f;
  const bool turn = need_cd && a.use_bulk;
  const bool unit = a.wa == 1 && a.wd == 1;    // the staged tile is the output tile: 16 x 64, staged pixel tid + 256 k is output pixel k

  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const BoxTile t = box_tile(tile, a.tiles_r, a.tiles_d, a.wa, a.wd);
    const int g = t.image;
    const float2* const xg = a.x + (long long)g * N * pixels;                            // the group's first frame
    const long long ug = (long long)g * (N - 1) * a.ascans;                              // ... and its first phasor

    int off[K], brow[K];                       // the staged pixel in its frame, or -1 outside the image; its A-scan
    float2 prev[K], cur[K];
    float t_re[K], t_im[K], half[K], sum_i[K], mean[K], m2[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int i = tid + k * kBoxBlock;
      int r, b;
      off[k] = -1, brow[k] = 0;
      if (i < ns && box_staged(t, i, sw, a.ascans, a.depths, &r, &b)) off[k] = r * a.depths + b, brow[k] = r;
      prev[k] = cur[k] = make_float2(0.f, 0.f);
      t_re[k] = t_im[k] = half[k] = sum_i[k] = mean[k] = m2[k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < K; k++)
      if (off[k] >= 0) prev[k] = xg[off[k]], cur[k] = xg[pixels + off[k]];
#pragma unroll
    for (int k = 0; k < K; k++) {
      if (off[k] >= 0) {                       // frame 0: Welford's first step, from (0, 0)
        const float i0 = ang_power(prev[k]);
        if (need_pow) sum_i[k] += i0;
        if (need_var) {
          const float delta = i0 - mean[k];
          mean[k] += delta / 1.f;
          m2[k] += delta * (i0 - mean[k]);
        }
      }
    }
    float q[kBoxOwn] = {0.f, 0.f, 0.f, 0.f};

    for (int n = 0; n + 1 < N; n++) {
      float aa_v[K], hh_v[K];
#pragma unroll
      for (int k = 0; k < K; k++) {
        float aa = 0.f, hh = 0.f;
        if (off[k] >= 0) {
          const float2 x1 = prev[k], x2 = cur[k];
          const float i1 = ang_power(x1), i2 = ang_power(x2);
          hh = 0.5f * (i1 + i2);
          if (need_cd) {
            float re = x2.x * x1.x + x2.y * x1.y, im = x2.y * x1.x - x2.x * x1.y;   // X[n + 1] conj(X[n])
            if (turn) {
              const float2 u = a.bulk[ug + (long long)n * a.ascans + brow[k]];
              const float tre = re * u.x - im * u.y, tim = re * u.y + im * u.x;
              re = tre, im = tim;
            }
            t_re[k] += re, t_im[k] += im, half[k] += hh;
          }
          if (need_dec) aa = sqrtf(i1) * sqrtf(i2);
          if (need_pow) sum_i[k] += i2;
          if (need_var) {
            const float delta = i2 - mean[k];
            mean[k] += delta / (float)(n + 2);
            m2[k] += delta * (i2 - mean[k]);
          }
          prev[k] = x2;
        }
        aa_v[k] = aa, hh_v[k] = hh;
      }
      if (n + 2 < N) {                         // the next frame, ahead of this pair's window passes
        const float2* const xn = xg + (long long)(n + 2) * pixels;
#pragma unroll
        for (int k = 0; k < K; k++)
          if (off[k] >= 0) cur[k] = xn[off[k]];
      }
      if (need_dec) {
        float nd[kAngPlanes][kBoxOwn];           // numerator, denominator
        ang_box<K>(unit, aa_v, hh_v, planes, sums, sr, sw, a.wa, a.wd, true, nd);
#pragma unroll
        for (int j = 0; j < kBoxOwn; j++) q[j] += nd[1][j] == 0.f ? 1.f : nd[0][j] / nd[1][j];
      }
    }

    float w_t[kAngPlanes][kBoxOwn] = {}, w_hi[kAngPlanes][kBoxOwn] = {}, w_var[kAngPlanes][kBoxOwn] = {};   // (T' re, T' im), (half sums, sum I), (V, -)
    if (need_cd) ang_box<K>(unit, t_re, t_im, planes, sums, sr, sw, a.wa, a.wd, true, w_t);
    if (need_cd || need_pow) ang_box<K>(unit, half, sum_i, planes, sums, sr, sw, a.wa, a.wd, true, w_hi);
    if (need_var) {
#pragma unroll
      for (int k = 0; k < K; k++) m2[k] = m2[k] / (float)N;   // V
      ang_box<K>(unit, m2, m2, planes, sums, sr, sw, a.wa, a.wd, false, w_var);
    }

#pragma unroll
    for (int j = 0; j < kBoxOwn; j++) {
      int r, b;
      if (!box_owned(t, j, a.ascans, a.depths, &r, &b)) continue;
      const int terms = box_terms(r, b, a.ascans, a.depths, a.wa, a.wd);
      const float cnt = (float)terms;
      const float power = w_hi[1][j] / (float)(N * terms);
      const bool masked = a.min_power > 0.f && power < a.min_power;
      const long long o = ((long long)g * a.ascans + r) * (long long)a.depths + b;
      if (a.out_power) a.out_power[o] = power;
      if (a.out_var) a.out_var[o] = masked ? 0.f : w_var[0][j] / cnt;
      if (a.out_decorr) a.out_decorr[o] = masked ? 0.f : 1.f - q[j] / (float)(N - 1);
      if (a.out_cdecorr) a.out_cdecorr[o] = (masked || w_hi[0][j] == 0.f) ? 0.f : 1.f - hypotf(w_t[0][j], w_t[1][j]) / w_hi[0][j];
    }
  }
}

template <int K>
hipError_t launch_stage(const AngioArgs& a, hipStream_t st) {
  static LdsGrant grant;   // one per instantiation
  if (hipError_t e = grant.ensure(angio_kernel<K>, a.lds_bytes); e != hipSuccess) return e;
  hipLaunchKernelGGL(angio_kernel<K>, dim3((unsigned)a.blocks), dim3(kBoxBlock), a.lds_bytes, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_angio(const AngioArgs& a, hipStream_t st) {
  if (!a.x || a.blocks < 1 || a.tiles < 1 || a.repeats < kAngMinRepeats || a.groups < 1) return hipErrorInvalidValue;
  if (a.wa < 1 || a.wa > kAngMaxWin || a.wd < 1 || a.wd > kAngMaxWin || a.lds_bytes != box_lds_bytes(kAngPlanes, a.wa, a.wd)) return hipErrorInvalidValue;
  if (!a.out_var && !a.out_decorr && !a.out_cdecorr && !a.out_power) return hipErrorInvalidValue;
  if (a.use_bulk && (a.bulk_blocks < 1 || !a.bulk || a.bulk_count < 1)) return hipErrorInvalidValue;
  if (a.keep != kAngKeepSmall && a.keep != kAngKeepMid && a.keep != kAngKeepLarge) return hipErrorInvalidValue;
  if (box_staged_rows(a.wa) * box_staged_depths(a.wd) > a.keep * kBoxBlock) return hipErrorInvalidValue;   // every staged pixel has its thread
  if (a.use_bulk) {
    hipLaunchKernelGGL(angio_bulk_kernel, dim3((unsigned)a.bulk_blocks), dim3(kBoxBulkBlock), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return a.keep == kAngKeepSmall ? launch_stage<kAngKeepSmall>(a, st) : a.keep == kAngKeepMid ? launch_stage<kAngKeepMid>(a, st) : launch_stage<kAngKeepLarge>(a, st);
}

}  // namespace fdoct
