// fdoct_capture.hip -- the kernels behind include/fdoct_capture.h:
//   BscanFFT.cpp:1041-1044   accumulate(data_y, baccum) over averagestoggle frames (and BscanDark.cpp's three captures),
//   BscanFFT.cpp:276-294     with smoothmovavg in front of it when movavgn > 0            -> capture_accumulate_kernel
//   BscanFFT.cpp:1105-1108   minMaxLoc over the binned frame ("Max intensity")             -> frame_minmax_kernel
// Both only stream.  A thread owns a run of 16 bytes of consecutive samples of one row (8 x u16, 16 x u8, 4 x f32, 2 x f64)
// and walks the frames in order with its sums in double registers.  Integer samples sum exactly (below 2^53); float samples
// sum in the order cv::accumulate adds them, one frame after the other, so the doubles are the reference's either way.
// Rows that are not 16-byte aligned, a row's tail and the moving average's taps are read sample by sample (the taps come from
// the caches: a thread's neighbours have just read them).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/fdoct.h"
#include "fdoct_capture_kernels.h"

namespace fdoct {

namespace {

constexpr int CAP_BLOCK = 256;
constexpr int CAP_WAVES_PER_CU = 16;  // the grid's cap, as the readouts cap theirs (fdoct_roi.hip)
constexpr int CAP_INFLIGHT = 4;       // frames whose loads are issued before the first of them is added

template <typename T> constexpr int kRun = 16 / (int)sizeof(T);

template <typename T>
__device__ __forceinline__ void widen(const uint4& raw, double (&d)[kRun<T>]) {
  T s[kRun<T>];
  __builtin_memcpy(s, &raw, 16);
#pragma unroll
  for (int j = 0; j < kRun<T>; j++) d[j] = (double)s[j];
}

// smoothmovavg of sample x of one row, BscanFFT.cpp:276-294, in double: taps -n..n in order, a tap outside the row replaced
// by the centre sample, the centre once more, then / 2 / (n + 1).
template <typename T>
__device__ __forceinline__ double movavg_at(const T* __restrict__ s, int x, int W, int n) {
  const double c = (double)s[x];
  double ssum = 0.0;
  for (int sk = -n; sk <= n; sk++) {
    const int ii = x + sk;
    ssum = ssum + ((ii > -1 && ii < W) ? (double)s[ii] : c);
  }
  ssum = ssum + c;
  return ssum / 2 / (n + 1);
}

struct AccArgs {
  const unsigned char* frames;
  long long pitch, fstride;  // bytes per row, per frame
  int nframes, H, W, n;
  int vec;         // frames, pitch and fstride are multiples of 16: a whole run is one 16-byte load
  int zero_start;  // the sum starts from 0.0 (cv::accumulate into zeros), else from the first frame's value
  double* out;     // H x W, packed
};

template <typename T>
__global__ __launch_bounds__(CAP_BLOCK) void capture_accumulate_kernel(AccArgs a) {
  constexpr int V = kRun<T>;
  const int cpr = (a.W + V - 1) / V;  // runs per row
  const long long items = (long long)a.H * cpr;
  for (long long t = (long long)blockIdx.x * CAP_BLOCK + threadIdx.x; t < items; t += (long long)gridDim.x * CAP_BLOCK) {
    const int r = (int)(t / cpr), x0 = (int)(t % cpr) * V;
    const unsigned char* row = a.frames + r * a.pitch;
    double acc[V];
    if (a.vec && a.n == 0 && x0 + V <= a.W) {
      const unsigned char* p = row + (long long)x0 * (int)sizeof(T);
      int f = 0;
      if (a.zero_start) {
#pragma unroll
        for (int j = 0; j < V; j++) acc[j] = 0.0;
      } else {
        widen<T>(*reinterpret_cast<const uint4*>(p), acc);
        f = 1;
      }
      for (; f + CAP_INFLIGHT <= a.nframes; f += CAP_INFLIGHT) {
        uint4 raw[CAP_INFLIGHT];
#pragma unroll
        for (int k = 0; k < CAP_INFLIGHT; k++) raw[k] = *reinterpret_cast<const uint4*>(p + (f + k) * a.fstride);
#pragma unroll
        for (int k = 0; k < CAP_INFLIGHT; k++) {
          double d[V];
          widen<T>(raw[k], d);
#pragma unroll
          for (int j = 0; j < V; j++) acc[j] = acc[j] + d[j];
        }
      }
      for (; f < a.nframes; f++) {
        double d[V];
        widen<T>(*reinterpret_cast<const uint4*>(p + f * a.fstride), d);
#pragma unroll
        for (int j = 0; j < V; j++) acc[j] = acc[j] + d[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; j++) acc[j] = 0.0;
      for (int f = 0; f < a.nframes; f++) {
        const T* s = reinterpret_cast<const T*>(row + f * a.fstride);
        const bool copy = f == 0 && !a.zero_start;
#pragma unroll
        for (int j = 0; j < V; j++) {
          const int x = x0 + j;
          if (x < a.W) {
            const double v = a.n > 0 ? movavg_at<T>(s, x, a.W, a.n) : (double)s[x];
            acc[j] = copy ? v : acc[j] + v;
          }
        }
      }
    }
    const long long o = (long long)r * a.W + x0;
#pragma unroll
    for (int j = 0; j < V; j += 2) {
      if (x0 + j + 1 < a.W && ((o + j) & 1) == 0) {
        *reinterpret_cast<double2*>(a.out + o + j) = make_double2(acc[j], acc[j + 1]);
      } else {
        if (x0 + j < a.W) a.out[o + j] = acc[j];
        if (x0 + j + 1 < a.W) a.out[o + j + 1] = acc[j + 1];
      }
    }
  }
}

// ---- min / max per frame ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double sel_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double sel_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double wave_min(double m) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = sel_min(m, __shfl_xor(m, off, 64));
  return m;
}
__device__ __forceinline__ double wave_max(double m) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = sel_max(m, __shfl_xor(m, off, 64));
  return m;
}

struct MinMaxArgs {
  const unsigned char* frames;
  long long pitch, fstride;
  int nframes, H, W, vec;
  double* partials;  // [frame][block] (min, max)
};

// Block (b, f) folds runs b * 256 + thread, + gridDim.x * 256, ... of frame f.
template <typename T>
__global__ __launch_bounds__(CAP_BLOCK) void frame_minmax_kernel(MinMaxArgs a) {
  constexpr int V = kRun<T>;
  __shared__ double part[2 * (CAP_BLOCK / 64)];
  const int cpr = (a.W + V - 1) / V;
  const long long items = (long long)a.H * cpr;
  const unsigned char* frame = a.frames + blockIdx.y * a.fstride;
  double lo = INFINITY, hi = -INFINITY;
  for (long long t = (long long)blockIdx.x * CAP_BLOCK + threadIdx.x; t < items; t += (long long)gridDim.x * CAP_BLOCK) {
    const int r = (int)(t / cpr), x0 = (int)(t % cpr) * V;
    const unsigned char* row = frame + r * a.pitch;
    if (a.vec && x0 + V <= a.W) {
      double d[V];
      widen<T>(*reinterpret_cast<const uint4*>(row + (long long)x0 * (int)sizeof(T)), d);
#pragma unroll
      for (int j = 0; j < V; j++) lo = sel_min(lo, d[j]), hi = sel_max(hi, d[j]);
    } else {
      const T* s = reinterpret_cast<const T*>(row);
#pragma unroll
      for (int j = 0; j < V; j++)
        if (x0 + j < a.W) {
          const double v = (double)s[x0 + j];
          lo = sel_min(lo, v), hi = sel_max(hi, v);
        }
    }
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) part[2 * wave] = lo, part[2 * wave + 1] = hi;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < CAP_BLOCK / 64; w++) lo = sel_min(lo, part[2 * w]), hi = sel_max(hi, part[2 * w + 1]);
    double* o = a.partials + 2 * ((long long)blockIdx.y * gridDim.x + blockIdx.x);
    o[0] = lo;
    o[1] = hi;
  }
}

// One wave per frame folds its nblk partials.
__global__ __launch_bounds__(CAP_BLOCK) void frame_minmax_fold_kernel(const double* __restrict__ partials, int nblk, int nframes,
                                                                      double* __restrict__ out_min, double* __restrict__ out_max) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * (CAP_BLOCK / 64) + (threadIdx.x >> 6);
  if (f >= nframes) return;
  double lo = INFINITY, hi = -INFINITY;
  for (int b = lane; b < nblk; b += 64) {
    const double* p = partials + 2 * ((long long)f * nblk + b);
    lo = sel_min(lo, p[0]), hi = sel_max(hi, p[1]);
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if (lane == 0) {
    if (out_min) out_min[f] = lo;
    if (out_max) out_max[f] = hi;
  }
}

bool vec_ok(const CaptureFrames& in) {
  return (reinterpret_cast<uintptr_t>(in.frames) % 16 == 0) && (in.pitch % 16 == 0);  // (a frame is H rows: its stride follows)
}
long long runs_of(const CaptureFrames& in, int es) { return (long long)in.H * ((in.W + 16 / es - 1) / (16 / es)); }
int sample_bytes(int dt) { return dt == FDOCT_U8 ? 1 : dt == FDOCT_U16 ? 2 : dt == FDOCT_F32 ? 4 : 8; }

}  // namespace

hipError_t launch_capture_accumulate(const CaptureFrames& in, int movavgn, bool zero_start, double* out, int num_cu, hipStream_t st) {
  AccArgs a{};
  a.frames = static_cast<const unsigned char*>(in.frames);
  a.pitch = (long long)in.pitch;
  a.fstride = (long long)in.pitch * in.H;
  a.nframes = in.nframes, a.H = in.H, a.W = in.W, a.n = movavgn;
  a.vec = vec_ok(in);
  a.zero_start = zero_start;
  a.out = out;
  const long long items = runs_of(in, sample_bytes(in.dt));
  // (more runs than the capped grid has threads: tests/test_gpu_stage_grids.py, test_capture_beyond_one_pass_of_the_grid)
  const int blocks = (int)std::min<long long>((items + CAP_BLOCK - 1) / CAP_BLOCK, resident_blocks(num_cu, CAP_WAVES_PER_CU, CAP_BLOCK));
  switch (in.dt) {
    case FDOCT_U8: hipLaunchKernelGGL(capture_accumulate_kernel<uint8_t>, dim3(blocks), dim3(CAP_BLOCK), 0, st, a); break;
    case FDOCT_U16: hipLaunchKernelGGL(capture_accumulate_kernel<uint16_t>, dim3(blocks), dim3(CAP_BLOCK), 0, st, a); break;
    case FDOCT_F32: hipLaunchKernelGGL(capture_accumulate_kernel<float>, dim3(blocks), dim3(CAP_BLOCK), 0, st, a); break;
    case FDOCT_F64: hipLaunchKernelGGL(capture_accumulate_kernel<double>, dim3(blocks), dim3(CAP_BLOCK), 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

int frame_minmax_blocks(const CaptureFrames& in, int num_cu) {
  const long long items = runs_of(in, sample_bytes(in.dt));
  const long long want = (items + CAP_BLOCK - 1) / CAP_BLOCK;
  const long long share = std::max(1, resident_blocks(num_cu, CAP_WAVES_PER_CU, CAP_BLOCK) / std::max(1, in.nframes));
  return (int)std::max<long long>(1, std::min(want, share));
}

hipError_t launch_frame_minmax(const CaptureFrames& in, double* partials, double* out_min, double* out_max, int num_cu, hipStream_t st) {
  if (in.nframes > 65535) return hipErrorInvalidValue;  // (frames ride in gridDim.y)
  MinMaxArgs a{};
  a.frames = static_cast<const unsigned char*>(in.frames);
  a.pitch = (long long)in.pitch;
  a.fstride = (long long)in.pitch * in.H;
  a.nframes = in.nframes, a.H = in.H, a.W = in.W;
  a.vec = vec_ok(in);
  a.partials = partials;
  // (more than 64 partials a frame, and more frames than workgroups: tests/test_gpu_stage_grids.py,
  // test_one_large_frame_takes_the_folds_second_stride, test_more_frames_than_workgroups)
  const int nblk = frame_minmax_blocks(in, num_cu);
  const dim3 grid(nblk, in.nframes);
  switch (in.dt) {
    case FDOCT_U8: hipLaunchKernelGGL(frame_minmax_kernel<uint8_t>, grid, dim3(CAP_BLOCK), 0, st, a); break;
    case FDOCT_U16: hipLaunchKernelGGL(frame_minmax_kernel<uint16_t>, grid, dim3(CAP_BLOCK), 0, st, a); break;
    case FDOCT_F32: hipLaunchKernelGGL(frame_minmax_kernel<float>, grid, dim3(CAP_BLOCK), 0, st, a); break;
    case FDOCT_F64: hipLaunchKernelGGL(frame_minmax_kernel<double>, grid, dim3(CAP_BLOCK), 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(frame_minmax_fold_kernel, dim3((in.nframes + CAP_BLOCK / 64 - 1) / (CAP_BLOCK / 64)), dim3(CAP_BLOCK), 0, st,
                     partials, nblk, in.nframes, out_min, out_max);
  return hipGetLastError();
}

}  // namespace fdoct
