// fdoct_calibrate.hip -- the kernels behind include/fdoct_calibrate.h:
//   BscanDark.cpp:82-90, 1056-1063   normalizerows and cv::normalize(.., 0.0001, 1, NORM_MINMAX) on the accumulated doubles
//                                    -> cal_minmax_kernel, cal_fold_kernel, cal_apply_kernel<CAL_SCALE>
//   BscanDark.cpp:1063               baccum / averagestoggle                                -> cal_apply_kernel<CAL_DIVIDE>
//   BscanDark.cpp:996                data_yb = (data_yr - data_yd) + (data_ys - data_yd)     -> cal_compose_kernel
// All of them stream rows of doubles: a lane owns a run of 2 doubles (16 bytes) of one row, read and written with one 16-byte
// access where pointer and pitch allow it and sample by sample otherwise (an odd width's last run, rows that are only 8-byte
// aligned).  Min and max are selections, so their reduction order does not matter; everything that rounds is written one
// operation at a time and must stay that way: the results are compared with the host's arithmetic (fdoct_host.cpp) bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "fdoct_calibrate_kernels.h"

// y * scale + shift and (yr - yd) + (ys - yd) round after every operation, as the host's do (its file is built with
// -ffp-contract=off): no fused multiply-add may be formed from them, whatever flags this file is compiled with.  (HIP's __dmul_rn
// / __dadd_rn are the plain operators, so they would not keep the compiler from contracting.)
#pragma clang fp contract(off)

namespace fdoct {

namespace {

constexpr int CAL_BLOCK = 256;
constexpr int CAL_WAVES_PER_CU = 16;  // the grid's cap, as the capture caps its grids (fdoct_capture.hip)
constexpr int CAL_RUN = 2;            // doubles a lane loads at once
constexpr int CAL_MIN_RUNS = 4;       // a segment is not made shorter than this many runs a lane
constexpr int CAL_MAX_SEGMENTS = 4096;

__device__ __forceinline__ double sel_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double sel_max(double a, double b) { return b > a ? b : a; }
// over the T lanes of a team (T a power of two; teams are aligned, so the partners of a lane are its own team's lanes)
__device__ __forceinline__ void team_minmax(double& lo, double& hi, int T) {
  for (int off = T >> 1; off > 0; off >>= 1) {
    lo = sel_min(lo, __shfl_xor(lo, off, 64));
    hi = sel_max(hi, __shfl_xor(hi, off, 64));
  }
}

struct MinMaxArgs {
  const double* in;
  long long pitch;          // doubles per row
  long long groups, items;  // items: runs per group
  int gh, cpr, W;           // rows per group, runs per row
  int T, S, vec;
  double* partials;         // [group][segment] (min, max)
};

// Team t of the grid folds units t, t + teams, ...; unit u is segment u % S of group u / S.
__global__ __launch_bounds__(CAL_BLOCK) void cal_minmax_kernel(MinMaxArgs a) {
  const int lane = threadIdx.x & (a.T - 1);
  const long long team = ((long long)blockIdx.x * CAL_BLOCK + threadIdx.x) / a.T;
  const long long teams = (long long)gridDim.x * CAL_BLOCK / a.T;
  const long long units = a.groups * a.S;
  const long long step = (long long)a.S * a.T;
  for (long long u = team; u < units; u += teams) {
    const long long g = u / a.S;
    const int seg = (int)(u - g * a.S);
    const double* base = a.in + g * a.gh * a.pitch;
    double lo = INFINITY, hi = -INFINITY;
    for (long long i = (long long)seg * a.T + lane; i < a.items; i += step) {
      const long long r = a.gh == 1 ? 0 : i / a.cpr;
      const int c = (int)(i - r * a.cpr) * CAL_RUN;
      const double* p = base + r * a.pitch + c;
      if (c + 1 < a.W) {
        double v0, v1;
        if (a.vec) {
          const double2 v = *reinterpret_cast<const double2*>(p);
          v0 = v.x, v1 = v.y;
        } else {
          v0 = p[0], v1 = p[1];
        }
        lo = sel_min(sel_min(lo, v0), v1), hi = sel_max(sel_max(hi, v0), v1);
      } else {
        const double v0 = p[0];
        lo = sel_min(lo, v0), hi = sel_max(hi, v0);
      }
    }
    team_minmax(lo, hi, a.T);
    if (lane == 0) a.partials[2 * u] = lo, a.partials[2 * u + 1] = hi;
  }
}

struct FoldArgs {
  const double* partials;
  double* coef;  // [group] (scale, shift)
  long long groups;
  int S, T2;
  double lo, hi;  // the caller's limits, in either order
};

// A team of T2 lanes folds a group's S partials; its first lane forms scale and shift in fdoct_host.cpp::normalize_minmax's
// operations.
__global__ __launch_bounds__(CAL_BLOCK) void cal_fold_kernel(FoldArgs a) {
  const int lane = threadIdx.x & (a.T2 - 1);
  const long long team = ((long long)blockIdx.x * CAL_BLOCK + threadIdx.x) / a.T2;
  const long long teams = (long long)gridDim.x * CAL_BLOCK / a.T2;
  for (long long g = team; g < a.groups; g += teams) {
    const double* p = a.partials + 2 * g * a.S;
    double smin = INFINITY, smax = -INFINITY;
#pragma unroll 4
    for (int s = lane; s < a.S; s += a.T2) smin = sel_min(smin, p[2 * s]), smax = sel_max(smax, p[2 * s + 1]);
    team_minmax(smin, smax, a.T2);
    if (lane == 0) {
      const double dmin = a.lo < a.hi ? a.lo : a.hi, dmax = a.lo < a.hi ? a.hi : a.lo;
      const double range = smax - smin;
      const double inv = range > DBL_EPSILON ? 1. / range : 0;
      const double scale = (dmax - dmin) * inv;
      const double prod = smin * scale;
      a.coef[2 * g] = scale;
      a.coef[2 * g + 1] = dmin - prod;
    }
  }
}

enum { CAL_SCALE = 0, CAL_DIVIDE = 1 };

struct ApplyArgs {
  const double* in;
  double* out;
  long long in_pitch, out_pitch;  // doubles per row
  long long items;                // runs in all
  int cpr, W, vec, per_row;
  const double* coef;             // CAL_SCALE: (scale, shift) per row, or one pair
  double divisor;                 // CAL_DIVIDE
};

template <int MODE>
__device__ __forceinline__ double cal_apply(double y, double k0, double k1) {
  if (MODE == CAL_DIVIDE) return y / k0;
  const double prod = y * k0;
  return prod + k1;
}

template <int MODE>
__global__ __launch_bounds__(CAL_BLOCK) void cal_apply_kernel(ApplyArgs a) {
  double k0 = a.divisor, k1 = 0.0;
  if (MODE == CAL_SCALE && !a.per_row) k0 = a.coef[0], k1 = a.coef[1];
  for (long long i = (long long)blockIdx.x * CAL_BLOCK + threadIdx.x; i < a.items; i += (long long)gridDim.x * CAL_BLOCK) {
    const long long r = i / a.cpr;
    const int c = (int)(i - r * a.cpr) * CAL_RUN;
    if (MODE == CAL_SCALE && a.per_row) k0 = a.coef[2 * r], k1 = a.coef[2 * r + 1];
    const double* p = a.in + r * a.in_pitch + c;
    double* o = a.out + r * a.out_pitch + c;
    if (c + 1 < a.W) {
      if (a.vec) {
        const double2 v = *reinterpret_cast<const double2*>(p);
        *reinterpret_cast<double2*>(o) = make_double2(cal_apply<MODE>(v.x, k0, k1), cal_apply<MODE>(v.y, k0, k1));
      } else {
        const double v0 = p[0], v1 = p[1];
        o[0] = cal_apply<MODE>(v0, k0, k1);
        o[1] = cal_apply<MODE>(v1, k0, k1);
      }
    } else {
      o[0] = cal_apply<MODE>(p[0], k0, k1);
    }
  }
}

__global__ __launch_bounds__(CAL_BLOCK) void cal_compose_kernel(const double* __restrict__ yr, const double* __restrict__ ys,
                                                                const double* __restrict__ yd, double* __restrict__ out, long long n) {
  const long long pairs = n / 2;
  for (long long i = (long long)blockIdx.x * CAL_BLOCK + threadIdx.x; i < pairs; i += (long long)gridDim.x * CAL_BLOCK) {
    const double2 r = reinterpret_cast<const double2*>(yr)[i], s = reinterpret_cast<const double2*>(ys)[i],
                  d = reinterpret_cast<const double2*>(yd)[i];
    const double rx = r.x - d.x, sx = s.x - d.x, ry = r.y - d.y, sy = s.y - d.y;
    reinterpret_cast<double2*>(out)[i] = make_double2(rx + sx, ry + sy);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double rd = yr[n - 1] - yd[n - 1], sd = ys[n - 1] - yd[n - 1];
    out[n - 1] = rd + sd;
  }
}

int pow2_up_to_wave(long long n) {
  int t = 1;
  while (t < 64 && t < n) t <<= 1;
  return t;
}
bool aligned16(const void* p, size_t pitch) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && pitch % 16 == 0; }
int capped_blocks(long long threads, int num_cu) {
  const long long want = (threads + CAL_BLOCK - 1) / CAL_BLOCK;
  return (int)std::max<long long>(1, std::min<long long>(want, resident_blocks(num_cu, CAL_WAVES_PER_CU, CAL_BLOCK)));
}

}  // namespace

MinMaxShape minmax_shape(int rows, int W, bool per_row, int num_cu) {
  MinMaxShape s;
  s.cpr = (W + CAL_RUN - 1) / CAL_RUN;
  s.groups = per_row ? rows : 1;
  s.rows_per_group = per_row ? 1 : rows;
  s.items = (long long)s.rows_per_group * s.cpr;
  s.T = pow2_up_to_wave(s.items);
  const long long teams = (long long)resident_blocks(num_cu, CAL_WAVES_PER_CU, CAL_BLOCK) * CAL_BLOCK / s.T;
  const long long worth = (s.items + (long long)CAL_MIN_RUNS * s.T - 1) / ((long long)CAL_MIN_RUNS * s.T);
  s.S = (int)std::max<long long>(1, std::min<long long>({teams / s.groups, worth, (long long)CAL_MAX_SEGMENTS}));
  s.T2 = pow2_up_to_wave(s.S);
  const long long units = s.groups * s.S;
  s.blocks = capped_blocks(units * s.T, num_cu);
  s.blocks2 = capped_blocks(s.groups * s.T2, num_cu);
  s.coef_offset = 2 * (size_t)units;
  s.ws_doubles = s.coef_offset + 2 * (size_t)s.groups;
  return s;
}

hipError_t launch_normalize_minmax(const RowsF64& r, bool per_row, double lo, double hi, double* ws, int num_cu, hipStream_t st) {
  if (r.rows < 1 || r.W < 1 || r.in_pitch % sizeof(double) || r.out_pitch % sizeof(double)) return hipErrorInvalidValue;
  const MinMaxShape s = minmax_shape(r.rows, r.W, per_row, num_cu);
  MinMaxArgs m{};
  m.in = r.in, m.pitch = (long long)(r.in_pitch / sizeof(double));
  m.groups = s.groups, m.items = s.items, m.gh = s.rows_per_group, m.cpr = s.cpr, m.W = r.W;
  m.T = s.T, m.S = s.S, m.vec = aligned16(r.in, r.in_pitch);
  m.partials = ws;
  hipLaunchKernelGGL(cal_minmax_kernel, dim3(s.blocks), dim3(CAL_BLOCK), 0, st, m);
  if (hipError_t e = hipGetLastError()) return e;
  FoldArgs f{};
  f.partials = ws, f.coef = ws + s.coef_offset, f.groups = s.groups, f.S = s.S, f.T2 = s.T2, f.lo = lo, f.hi = hi;
  hipLaunchKernelGGL(cal_fold_kernel, dim3(s.blocks2), dim3(CAL_BLOCK), 0, st, f);
  if (hipError_t e = hipGetLastError()) return e;
  ApplyArgs a{};
  a.in = r.in, a.out = r.out, a.in_pitch = m.pitch, a.out_pitch = (long long)(r.out_pitch / sizeof(double));
  a.items = (long long)r.rows * s.cpr, a.cpr = s.cpr, a.W = r.W;
  a.vec = m.vec && aligned16(r.out, r.out_pitch);
  a.per_row = per_row, a.coef = f.coef;
  hipLaunchKernelGGL(cal_apply_kernel<CAL_SCALE>, dim3(capped_blocks(a.items, num_cu)), dim3(CAL_BLOCK), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_divide_rows(const RowsF64& r, double divisor, int num_cu, hipStream_t st) {
  if (r.rows < 1 || r.W < 1 || r.in_pitch % sizeof(double) || r.out_pitch % sizeof(double)) return hipErrorInvalidValue;
  ApplyArgs a{};
  a.cpr = (r.W + CAL_RUN - 1) / CAL_RUN, a.W = r.W;
  a.in = r.in, a.out = r.out, a.in_pitch = (long long)(r.in_pitch / sizeof(double)), a.out_pitch = (long long)(r.out_pitch / sizeof(double));
  a.items = (long long)r.rows * a.cpr;
  a.vec = aligned16(r.in, r.in_pitch) && aligned16(r.out, r.out_pitch);
  a.divisor = divisor;
  hipLaunchKernelGGL(cal_apply_kernel<CAL_DIVIDE>, dim3(capped_blocks(a.items, num_cu)), dim3(CAL_BLOCK), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_compose(const double* yr, const double* ys, const double* yd, double* out, size_t n, int num_cu, hipStream_t st) {
  if (!n || !aligned16(yr, 0) || !aligned16(ys, 0) || !aligned16(yd, 0) || !aligned16(out, 0)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cal_compose_kernel, dim3(capped_blocks((long long)((n + 1) / 2), num_cu)), dim3(CAL_BLOCK), 0, st, yr, ys, yd, out,
                     (long long)n);
  return hipGetLastError();
}

}  // namespace fdoct
