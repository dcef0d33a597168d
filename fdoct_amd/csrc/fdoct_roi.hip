// fdoct_roi.hip -- readouts of the dB B-scans the chain wrote (include/fdoct_roi.h):
//   BscanFFTpeak.cpp:466-739  printPeakHoldAscan: per A-scan column of an ROI the max over its depth rows, and the same max
//                             for one A-scan, held across B-scans                                  -> roi_hold_kernel
//   BscanFFT.cpp:146-171      printMinMaxAscan: min / max of one A-scan, depth rows 0-3 read as row 4 -> roi_minmax_kernel
//   BscanFFT.cpp:99-144       printAvgROI: mean of a 3-depth x width box                         -> roi_mean_kernel
// All three only read the image.  Max and min are selections, so the holds and the A-scan extremes are the input's own f32
// values whatever the grid; the mean sums in double in a fixed order, so reruns agree bit for bit.  Grids are capped at what is
// resident: a wave walks a contiguous piece of its item's (B-scan, position) space, so an ROI of one pixel and the whole image
// of every B-scan of the call take one launch of the same shape.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "fdoct_roi_kernels.h"

namespace fdoct {

namespace {

constexpr int ROI_BLOCK = 256;  // 4 waves; every wave of the hold / min-max kernels is an independent worker
constexpr int ROI_WAVES_PER_CU = 16;
constexpr int kMinLaneLoads = 16;  // loads per lane below which another slice of an item does not pay

__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  return m;
}
__device__ __forceinline__ float wave_min(float m) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fminf(m, __shfl_xor(m, off, 64));
  return m;
}
// Holds only grow within a launch, so a word already at or above the value needs no atomic: once a hold has settled, most
// waves only read it, and an ROI folded by thousands of waves does not queue thousands of atomics on each word.
__device__ __forceinline__ void hold_max(uint32_t* word, float m) {
  if (m == -INFINITY) return;
  const uint32_t e = roi_encode(m);
  if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < e) atomicMax(word, e);
}

// Walks positions t0 + first, t0 + first + step, ... < t1 of a space of npos positions per B-scan as (g, p) without a
// division per step.
struct Walk {
  long long g;
  int p, dg, dp, npos;
  __device__ Walk(long long t, int step, int npos_) : g(t / npos_), p((int)(t % npos_)), dg(step / npos_), dp(step % npos_), npos(npos_) {}
  __device__ void next() {
    g += dg;
    p += dp;
    if (p >= npos) p -= npos, g++;
  }
};

struct HoldArgs {
  const float* db;
  long long bs;  // floats per B-scan
  int nb, D, H, tr;
  int x, y, w, h, ascanat;
  uint32_t* cols;
  uint32_t* scalar;
  int vec;      // 16-byte loads along the contiguous dimension (its length a multiple of 4, the image 16-byte aligned)
  int nchunks;  // transposed: items of up to 64 lanes across the ROI's A-scans (0 in row-major)
  int nruns;    // items that reduce one contiguous or strided run: row-major w + 1 (the ROI's A-scans, then ascanat); transposed 1
  int slices;   // each item's (B-scan, position) space in this many contiguous pieces
};

// Row-major runs (depth-contiguous): lanes across the run's positions and B-scans, a wave reduction, one atomic per wave.
// The transposed layout's A-scan ascanat is a run too, strided by H.
__device__ void hold_run(const HoldArgs& a, int k, int s, int lane) {
  const bool strided = a.tr;
  const int c = strided ? a.ascanat : (k < a.w ? a.x + k : a.ascanat);
  uint32_t* word = (!strided && k < a.w) ? a.cols + k : a.scalar;
  const bool vec = a.vec && !strided;
  const int q0 = a.y >> 2, q1 = (a.y + a.h + 3) >> 2;
  const int npos = vec ? q1 - q0 : a.h;
  const long long n = (long long)a.nb * npos, t0 = n * s / a.slices, t1 = n * (s + 1) / a.slices;
  float m = -INFINITY;
  if (t0 + lane < t1) {
    Walk wk(t0 + lane, 64, npos);
    if (vec) {
      const float* base = a.db + (long long)c * a.D;
#pragma unroll 8
      for (long long t = t0 + lane; t < t1; t += 64, wk.next()) {
        const int q = q0 + wk.p;
        const float4 v = *reinterpret_cast<const float4*>(base + wk.g * a.bs + 4 * q);
        const int r = 4 * q;
        if (r >= a.y && r < a.y + a.h) m = fmaxf(m, v.x);
        if (r + 1 >= a.y && r + 1 < a.y + a.h) m = fmaxf(m, v.y);
        if (r + 2 >= a.y && r + 2 < a.y + a.h) m = fmaxf(m, v.z);
        if (r + 3 >= a.y && r + 3 < a.y + a.h) m = fmaxf(m, v.w);
      }
    } else {
      const long long es = strided ? a.H : 1;  // element stride along the run
      const float* base = a.db + (strided ? (long long)a.y * a.H + c : (long long)c * a.D + a.y);
#pragma unroll 8
      for (long long t = t0 + lane; t < t1; t += 64, wk.next()) m = fmaxf(m, base[wk.g * a.bs + wk.p * es]);
    }
  }
  m = wave_max(m);
  if (lane == 0) hold_max(word, m);
}

// Transposed (A-scan-contiguous): each lane owns one quad (or one A-scan) of the ROI and folds the rows in registers; lanes
// beyond the chunk's width take further rows of the same quads, so a narrow ROI still keeps the wave busy.
__device__ void hold_chunk(const HoldArgs& a, int u, int s, int lane) {
  const int qa = a.vec ? (a.x >> 2) + 64 * u : a.x + 64 * u;
  const int qend = a.vec ? (a.x + a.w + 3) >> 2 : a.x + a.w;
  const int nq = min(64, qend - qa);
  const int groups = 64 / nq;
  if (lane >= groups * nq) return;
  const int pq = lane % nq, rg = lane / nq;
  const long long n = (long long)a.nb * a.h, t0 = n * s / a.slices, t1 = n * (s + 1) / a.slices;
  if (t0 + rg >= t1) return;
  Walk wk(t0 + rg, groups, a.h);
  if (a.vec) {
    const float* base = a.db + (long long)a.y * a.H + 4 * (qa + pq);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll 8
    for (long long t = t0 + rg; t < t1; t += groups, wk.next()) {
      const float4 v = *reinterpret_cast<const float4*>(base + wk.g * a.bs + (long long)wk.p * a.H);
      m.x = fmaxf(m.x, v.x), m.y = fmaxf(m.y, v.y), m.z = fmaxf(m.z, v.z), m.w = fmaxf(m.w, v.w);
    }
    const int c = 4 * (qa + pq);
    const float mv[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (c + j >= a.x && c + j < a.x + a.w) hold_max(a.cols + (c + j - a.x), mv[j]);
  } else {
    const float* base = a.db + (long long)a.y * a.H + qa + pq;
    float m = -INFINITY;
#pragma unroll 8
    for (long long t = t0 + rg; t < t1; t += groups, wk.next()) m = fmaxf(m, base[wk.g * a.bs + (long long)wk.p * a.H]);
    hold_max(a.cols + (qa + pq - a.x), m);
  }
}

__global__ __launch_bounds__(ROI_BLOCK) void roi_hold_kernel(HoldArgs a) {
  const int lane = threadIdx.x & 63;
  const int per_slice = a.nchunks + a.nruns;
  const long long items = (long long)per_slice * a.slices;
  const long long waves = (long long)gridDim.x * (ROI_BLOCK / 64);
  for (long long i = (long long)blockIdx.x * (ROI_BLOCK / 64) + (threadIdx.x >> 6); i < items; i += waves) {
    const int u = (int)(i % per_slice), s = (int)(i / per_slice);
    if (u < a.nchunks)
      hold_chunk(a, u, s, lane);
    else
      hold_run(a, u - a.nchunks, s, lane);
  }
}

// One wave per B-scan: A-scan ascanat over depths 4..D-1 (depths 0-3 are copies of depth 4: they cannot change either extreme).
__global__ __launch_bounds__(ROI_BLOCK) void roi_minmax_kernel(const float* __restrict__ db, long long bs, int nb, int D, int H,
                                                               int tr, int ascanat, int vec, float* __restrict__ out_min,
                                                               float* __restrict__ out_max) {
  const int lane = threadIdx.x & 63;
  const int waves = gridDim.x * (ROI_BLOCK / 64);
  for (int g = blockIdx.x * (ROI_BLOCK / 64) + (threadIdx.x >> 6); g < nb; g += waves) {
    float lo = INFINITY, hi = -INFINITY;
    const float* col = db + g * bs + (tr ? ascanat : (long long)ascanat * D);
    if (vec) {  // row-major, D % 4 == 0: quads 1 .. D/4 - 1 are exactly depths 4 .. D-1
      for (int q = 1 + lane; q < D / 4; q += 64) {
        const float4 v = *reinterpret_cast<const float4*>(col + 4 * q);
        lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
        hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
      }
    } else {
      const long long es = tr ? H : 1;
      for (int r = 4 + lane; r < D; r += 64) {
        const float v = col[r * es];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
      }
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    if (lane == 0) {
      out_min[g] = lo;
      out_max[g] = hi;
    }
  }
}

// One workgroup per B-scan: thread t sums A-scans ascanat + t, + t + 256, ... (three depths each, in depth order) in double;
// the block then adds the partial sums in a fixed tree, so the result does not depend on the grid or on timing.
__global__ __launch_bounds__(ROI_BLOCK) void roi_mean_kernel(const float* __restrict__ db, long long bs, int nb, int D, int H,
                                                             int tr, int ascanat, int vertpos, int width, double* __restrict__ out) {
  __shared__ double part[ROI_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long rs = tr ? H : 1, cs = tr ? 1 : D;  // strides of a depth step and an A-scan step
  for (int g = blockIdx.x; g < nb; g += gridDim.x) {
    const float* box = db + g * bs + (long long)vertpos * rs + (long long)ascanat * cs;
    double acc = 0.0;
    for (int c = threadIdx.x; c < width; c += ROI_BLOCK) {
      const float* p = box + c * cs;
      acc += (double)p[0];
      acc += (double)p[rs];
      acc += (double)p[2 * rs];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double sum = part[0];
      for (int w = 1; w < ROI_BLOCK / 64; w++) sum += part[w];
      out[g] = sum / (3.0 * width);
    }
    __syncthreads();
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

hipError_t launch_roi_hold(const RoiImage& im, int x, int y, int w, int h, int ascanat, uint32_t* cols, uint32_t* scalar,
                           int num_cu, hipStream_t st) {
  HoldArgs a{};
  a.db = im.db;
  a.bs = (long long)im.depths * im.ascans;
  a.nb = im.nb, a.D = im.depths, a.H = im.ascans, a.tr = im.transposed;
  a.x = x, a.y = y, a.w = w, a.h = h, a.ascanat = ascanat;
  a.cols = cols, a.scalar = scalar;
  a.vec = aligned16(im.db) && ((im.transposed ? im.ascans : im.depths) % 4 == 0);
  long long lane_work;  // loads per lane of one item over all B-scans: slices stop where each would get fewer than 16
  if (im.transposed) {
    const int span = a.vec ? ((x + w + 3) >> 2) - (x >> 2) : w;
    a.nchunks = (span + 63) / 64;
    a.nruns = 1;
    lane_work = (long long)im.nb * h / (64 / std::min(64, span));
  } else {
    a.nchunks = 0;
    a.nruns = w + 1;
    lane_work = (long long)im.nb * (a.vec ? ((y + h + 3) >> 2) - (y >> 2) : h) / 64;
  }
  const int per_slice = a.nchunks + a.nruns;
  const long long waves = (long long)resident_blocks(num_cu, ROI_WAVES_PER_CU, ROI_BLOCK) * (ROI_BLOCK / 64);
  long long slices = std::max(1LL, waves / per_slice);
  slices = std::min(slices, std::max(1LL, lane_work / kMinLaneLoads));
  a.slices = (int)slices;
  const long long items = (long long)per_slice * slices;
  // (more runs than waves, and the quad masks against poisoned surroundings: tests/test_gpu_stage_grids.py, test_hold_*)
  const int blocks = (int)std::min<long long>((items + 3) / 4, resident_blocks(num_cu, ROI_WAVES_PER_CU, ROI_BLOCK));
  hipLaunchKernelGGL(roi_hold_kernel, dim3(blocks), dim3(ROI_BLOCK), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_roi_ascan_minmax(const RoiImage& im, int ascanat, float* out_min, float* out_max, int num_cu, hipStream_t st) {
  const long long bs = (long long)im.depths * im.ascans;
  const int vec = !im.transposed && im.depths % 4 == 0 && aligned16(im.db);
  // (more B-scans than waves: tests/test_gpu_stage_grids.py, test_ascan_minmax_of_more_bscans_than_waves)
  const int blocks = std::min((im.nb + 3) / 4, resident_blocks(num_cu, ROI_WAVES_PER_CU, ROI_BLOCK));
  hipLaunchKernelGGL(roi_minmax_kernel, dim3(blocks), dim3(ROI_BLOCK), 0, st, im.db, bs, im.nb, im.depths, im.ascans,
                     im.transposed, ascanat, vec, out_min, out_max);
  return hipGetLastError();
}

hipError_t launch_roi_mean(const RoiImage& im, int ascanat, int vertpos, int width, double* out, int num_cu, hipStream_t st) {
  const long long bs = (long long)im.depths * im.ascans;
  // (more B-scans than workgroups: tests/test_gpu_stage_grids.py, test_roi_mean_of_more_bscans_than_workgroups)
  const int blocks = std::min(im.nb, resident_blocks(num_cu, ROI_WAVES_PER_CU, ROI_BLOCK));
  hipLaunchKernelGGL(roi_mean_kernel, dim3(blocks), dim3(ROI_BLOCK), 0, st, im.db, bs, im.nb, im.depths, im.ascans,
                     im.transposed, ascanat, vertpos, width, out);
  return hipGetLastError();
}

}  // namespace fdoct
