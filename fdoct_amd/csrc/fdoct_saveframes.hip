// fdoct_saveframes.hip -- per-frame B-scan saves while averaging (include/fdoct_saveframes.h), BscanFFT.cpp:1197-1240 and 1360-1377:
//   accumulate(bscantemp, bscantransposed); bscantemp.copyTo(bscansave0/1[indextemp]);                       (every frame)
//   transpose(bscantransposed, bscan); bscan = bscan / averagestoggle; bscan += 0.00001; log; 20.0 * . / 2.303; DC mask   (a group)
//   transpose(bscansave[ii], t); t += 0.000001; log(t, t); t = 20.0 * t / 2.303; normalize(0, 1, NORM_MINMAX); convertTo(CV_8UC1, 255.0)
// in two passes over per-frame magnitudes that lie in device memory.  Byte work: 4 bytes in and 1 byte out per pixel, plus the
// fold's output, so by their bytes both passes are bandwidth-bound (measured, they are not there yet: DESIGN.md 3.4f); every
// product, sum and quotient is separately rounded (no FMA), which makes the results pure functions of the float input.
//   scan   reads every image once, coalesced in the input's own order.  A lane owns SF_PER_LANE elements of a chunk of an
//          image, walks the frames of a fold group with their sums in registers as doubles (as fdoct_manualavg.hip does),
//          and writes bscan / bscandb once per group in the output's layout.  On the way it takes min and max of
//          d = 20 ln(x + 1e-6) / 2.303 per image -- on d itself, not on x: nothing guarantees that the device's double ln is
//          monotone to its last bit -- and leaves one (min, max) pair per image and workgroup column in `part`.
//   map    folds an image's partial extrema, normalises and writes the bytes.  For H x D input this is a transpose: a tile is
//          loaded along depths, turned into bytes, laid into a padded LDS tile and stored along A-scans, four bytes per
//          store where the address allows it and byte by byte where it does not (the picture's edges, a pointer or an `ascans`
//          that is no multiple of four).  D x H input is mapped in place, four pixels per lane.
// Both grids are capped and swept by loops; neither H nor D need be a multiple of anything.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "fdoct_saveframes_kernels.h"

namespace fdoct {

namespace {

constexpr int SF_BLOCK = 256;
constexpr int SF_PER_LANE = 16;                       // elements of a chunk per lane: 16 double sums in registers
constexpr int SF_CHUNK = SF_BLOCK * SF_PER_LANE;      // elements of an image a workgroup takes at a time
constexpr int SF_MAX_PARTS = 256;                     // partial (min, max) pairs per image; one per thread in the map pass
constexpr int SF_WAVES_PER_CU = 16;
constexpr int SF_TILE = 64, SF_TILE_PITCH = SF_TILE + 4;  // bytes: rows 17 dwords apart, so a wave's byte writes down a column spread over the banks

__device__ __forceinline__ double sf_db(float x) {
  double v = __dadd_rn((double)x, 0.000001);          // main:1369
  v = v < 0.000001 ? 0.000001 : v;                    // (a negative input only: include/fdoct_saveframes.h)
  return __dmul_rn(20.0, log(v)) / 2.303;             // main:1370-1371
}

__device__ __forceinline__ void block_minmax(double& lo, double& hi, double* sm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double l2 = __shfl_xor(lo, off, 64), h2 = __shfl_xor(hi, off, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if (lane == 0) {
    sm[2 * wave] = lo;
    sm[2 * wave + 1] = hi;
  }
  __syncthreads();
  lo = sm[0];
  hi = sm[1];
#pragma unroll
  for (int w = 1; w < SF_BLOCK / 64; w++) {
    lo = sm[2 * w] < lo ? sm[2 * w] : lo;
    hi = sm[2 * w + 1] > hi ? sm[2 * w + 1] : hi;
  }
  __syncthreads();
}

// Slot j of a lane within a chunk: with 16-byte loads four neighbours at a time, else strided by the workgroup.
template <bool VEC>
__device__ __forceinline__ long long sf_slot(int j, int t) {
  return VEC ? ((long long)((j >> 2) * SF_BLOCK + t) << 2) + (j & 3) : (long long)j * SF_BLOCK + t;
}

// grid = (parts, groups in flight).  A workgroup column p takes chunks p, p + parts, .. of every image of its groups, and keeps
// the running extrema of (image, p) in part[] itself: one thread of one workgroup owns each pair.
template <bool VEC>
__global__ __launch_bounds__(SF_BLOCK) void saveframes_scan_kernel(SaveFramesArgs a) {
  __shared__ double sm[2 * (SF_BLOCK / 64)];
  const int t = threadIdx.x, A = a.group, D = a.depths, H = a.ascans;
  const long long count = a.count, nchunks = (count + SF_CHUNK - 1) / SF_CHUNK;
  const int ngroups = a.nframes / A;
  const bool fold = a.out_bscan || a.out_db, mask = a.dc_mask && D > 4;
  const double dA = (double)A;
  for (int g = blockIdx.y; g < ngroups; g += gridDim.y) {
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
      const long long base = c * SF_CHUNK;
      double acc[SF_PER_LANE];
#pragma unroll
      for (int j = 0; j < SF_PER_LANE; j++) acc[j] = 0.0;
      for (int f = 0; f < A; f++) {
        const long long frame = (long long)g * A + f;
        const float* __restrict__ src = a.in + frame * count + base;
        float x[SF_PER_LANE];
        if (VEC) {
#pragma unroll
          for (int k = 0; k < SF_PER_LANE / 4; k++) {
            const long long off = sf_slot<true>(4 * k, t);
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (base + off < count) q = *reinterpret_cast<const float4*>(src + off);  // count % 4 == 0: a whole quad or none
            x[4 * k] = q.x, x[4 * k + 1] = q.y, x[4 * k + 2] = q.z, x[4 * k + 3] = q.w;
          }
        } else {
#pragma unroll
          for (int j = 0; j < SF_PER_LANE; j++) {
            const long long off = sf_slot<false>(j, t);
            x[j] = base + off < count ? src[off] : 0.f;
          }
        }
        double lo = __builtin_huge_val(), hi = -__builtin_huge_val();
#pragma unroll
        for (int j = 0; j < SF_PER_LANE; j++) {
          if (base + sf_slot<VEC>(j, t) >= count) continue;
          acc[j] = __dadd_rn(acc[j], (double)x[j]);  // main:1197
          if (a.part) {
            const double d = sf_db(x[j]);
            lo = d < lo ? d : lo;
            hi = d > hi ? d : hi;
          }
        }
        if (a.part) {  // (uniform: the barriers inside are met by every thread)
          block_minmax(lo, hi, sm);
          if (t == 0) {
            double* p = a.part + ((size_t)frame * gridDim.x + blockIdx.x) * 2;
            if (c != (long long)blockIdx.x) {  // not this column's first chunk of the image
              lo = p[0] < lo ? p[0] : lo;
              hi = p[1] > hi ? p[1] : hi;
            }
            p[0] = lo;
            p[1] = hi;
          }
        }
      }
      if (!fold) continue;
#pragma unroll
      for (int j = 0; j < SF_PER_LANE; j++) {
        const long long e = base + sf_slot<VEC>(j, t);
        if (e >= count) continue;
        const double b = __dadd_rn(acc[j] / dA, a.eps);  // main:1221-1222
        const long long asc = a.in_transposed ? e % H : e / D;
        const int dep = (int)(a.in_transposed ? e / H : e % D);
        const long long image = (long long)g * count;
        const long long o = image + (a.out_transposed ? (long long)dep * H + asc : asc * D + dep);
        if (a.out_bscan) a.out_bscan[o] = (float)b;
        if (a.out_db) {
          const float v = (float)(__dmul_rn(20.0, log(b)) / 2.303);  // main:1235-1237
          if (!(mask && dep < 2)) a.out_db[o] = v;
          if (mask && dep == 4) {  // main:1239-1240: the owner of depth row 4 writes rows 1 and 0 as well
            a.out_db[image + (a.out_transposed ? (long long)1 * H + asc : asc * D + 1)] = v;
            a.out_db[image + (a.out_transposed ? asc : asc * D)] = v;
          }
        }
      }
    }
  }
}

// The extrema of image `frame` from its partial pairs, as cv::normalize(NORM_MINMAX, 0, 1) uses them: scale = 1 / (max - min)
// (0 when the range is below DBL_EPSILON), shift = -min * scale.  Every thread of the workgroup calls it.
__device__ __forceinline__ void sf_scale_shift(const SaveFramesArgs& a, long long frame, double* sm, double* scale, double* shift) {
  double lo = __builtin_huge_val(), hi = -__builtin_huge_val();
  if ((int)threadIdx.x < a.parts) {
    lo = a.part[((size_t)frame * a.parts + threadIdx.x) * 2];
    hi = a.part[((size_t)frame * a.parts + threadIdx.x) * 2 + 1];
  }
  block_minmax(lo, hi, sm);
  const double range = hi - lo;
  *scale = range > 2.220446049250313e-16 ? 1.0 / range : 0.0;
  *shift = __dsub_rn(0.0, __dmul_rn(lo, *scale));
}

__device__ __forceinline__ unsigned sf_u8(float x, double scale, double shift) {
  // normalize: dst = src * scale + shift in double; convertTo(CV_8U, 255.0): saturate(rint(dst * 255.0))
  const double nrm = __dadd_rn(__dmul_rn(sf_db(x), scale), shift);
  double r = rint(__dmul_rn(nrm, 255.0));
  r = r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r);
  return (unsigned)(int)r;
}

// D x H input: the picture has the input's order.  Work item = (image, chunk); a lane takes four quads of neighbours.
__global__ __launch_bounds__(SF_BLOCK) void saveframes_map_kernel(SaveFramesArgs a) {
  __shared__ double sm[2 * (SF_BLOCK / 64)];
  const long long count = a.count, nchunks = (count + SF_CHUNK - 1) / SF_CHUNK, total = nchunks * a.nframes;
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const long long frame = w / nchunks, base = (w % nchunks) * SF_CHUNK;
    double scale, shift;
    sf_scale_shift(a, frame, sm, &scale, &shift);
    const float* __restrict__ src = a.in + frame * count;
    unsigned char* __restrict__ dst = a.gray + frame * count;
#pragma unroll
    for (int k = 0; k < SF_PER_LANE / 4; k++) {
      const long long e = base + ((long long)(k * SF_BLOCK + threadIdx.x) << 2);
      if (e >= count) continue;
      const bool whole = e + 3 < count;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (whole && (reinterpret_cast<uintptr_t>(src + e) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(src + e);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      } else {
        for (int i = 0; i < 4; i++)
          if (e + i < count) v[i] = src[e + i];
      }
      unsigned u[4];
#pragma unroll
      for (int i = 0; i < 4; i++) u[i] = sf_u8(v[i], scale, shift);
      if (whole && (reinterpret_cast<uintptr_t>(dst + e) & 3) == 0) {
        *reinterpret_cast<unsigned*>(dst + e) = u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24);
      } else {
        for (int i = 0; i < 4; i++)
          if (e + i < count) dst[e + i] = (unsigned char)u[i];
      }
    }
  }
}

// H x D input: work item = (image, tile of SF_TILE A-scans x SF_TILE depths).  Loads run along depths, stores along A-scans.
__global__ __launch_bounds__(SF_BLOCK) void saveframes_map_transpose_kernel(SaveFramesArgs a) {
  __shared__ double sm[2 * (SF_BLOCK / 64)];
  __shared__ __attribute__((aligned(4))) unsigned char tile[SF_TILE][SF_TILE_PITCH];  // [depth][A-scan]
  const int D = a.depths, H = a.ascans;
  const long long th = (H + SF_TILE - 1) / SF_TILE, td = (D + SF_TILE - 1) / SF_TILE, per_image = th * td, total = per_image * a.nframes;
  const int tx = threadIdx.x & (SF_TILE - 1), ty = threadIdx.x / SF_TILE;
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const long long frame = w / per_image, tl = w % per_image;
    const int h0 = (int)(tl / td) * SF_TILE, d0 = (int)(tl % td) * SF_TILE;
    double scale, shift;
    sf_scale_shift(a, frame, sm, &scale, &shift);
    const float* __restrict__ src = a.in + frame * a.count;
    unsigned char* __restrict__ dst = a.gray + frame * a.count;
    const int d = d0 + tx;
#pragma unroll 4
    for (int r = ty; r < SF_TILE; r += SF_BLOCK / SF_TILE) {
      const int h = h0 + r;
      if (h < H && d < D) tile[tx][r] = (unsigned char)sf_u8(src[(long long)h * D + d], scale, shift);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < SF_TILE * SF_TILE / 4 / SF_BLOCK; it++) {
      const int idx = it * SF_BLOCK + threadIdx.x, dd = idx / (SF_TILE / 4), hq = (idx % (SF_TILE / 4)) * 4;
      const int od = d0 + dd, oh = h0 + hq;
      if (od >= D || oh >= H) continue;
      unsigned char* p = dst + (long long)od * H + oh;
      if (oh + 3 < H && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        *reinterpret_cast<unsigned*>(p) = *reinterpret_cast<const unsigned*>(&tile[dd][hq]);
      } else {
        for (int i = 0; i < 4; i++)
          if (oh + i < H) p[i] = tile[dd][hq + i];
      }
    }
    __syncthreads();  // the tile is free for the next work item
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

void saveframes_plan_launch(SaveFramesArgs* a, int num_cu) {
  // images are `count` floats apart: beyond the first, groups of four stay aligned only if count % 4 == 0
  a->vec = a->count >= 4 && a->count % 4 == 0 && aligned16(a->in);
  const long long nchunks = (a->count + SF_CHUNK - 1) / SF_CHUNK;
  const long long resident = resident_blocks(num_cu, SF_WAVES_PER_CU, SF_BLOCK);
  a->parts = (int)std::min<long long>(nchunks, SF_MAX_PARTS);
  const long long ngroups = a->nframes / a->group;
  a->scan_groups = (int)std::max(1LL, std::min({ngroups, (2 * resident + a->parts - 1) / a->parts, 65535LL}));
  const long long th = (a->ascans + SF_TILE - 1) / SF_TILE, td = (a->depths + SF_TILE - 1) / SF_TILE;
  const long long items = (a->in_transposed ? nchunks : th * td) * a->nframes;
  a->map_blocks = (int)std::max(1LL, std::min(items, 2 * resident));
}

hipError_t launch_saveframes(const SaveFramesArgs& a, hipStream_t st) {
  auto scan = a.vec ? saveframes_scan_kernel<true> : saveframes_scan_kernel<false>;
  hipLaunchKernelGGL(scan, dim3(a.parts, a.scan_groups), dim3(SF_BLOCK), 0, st, a);
  if (a.gray) {
    auto map = a.in_transposed ? saveframes_map_kernel : saveframes_map_transpose_kernel;
    hipLaunchKernelGGL(map, dim3(a.map_blocks), dim3(SF_BLOCK), 0, st, a);
  }
  return hipGetLastError();
}

}  // namespace fdoct
