// fdoct_enface.hip -- the kernels of include/fdoct_enface.h: the en-face projection of a volume over depth slabs that are fixed or
// follow the surface (the header states the quantity and the order of every sum; tests/enface_model.py restates both in numpy).
//
// Both kernels give one wavefront an A-scan -- 256-thread workgroups, a capped grid striding over the A-scans -- and use no LDS.
//
// enface_surface_kernel, in front where a surface is asked for: lane l takes candidates s0 + l + 64 i.  A candidate's box sum is
// `smooth` 4-byte loads from scratch, consecutive lanes on consecutive depths; the re-reads of neighbouring candidates hit the
// cache (EXPERIMENTS.md: the LDS form with a halo was not built).  Mode 2 makes a pass for the maximum first.  The crossing is
// searched 64 candidates at a time, in increasing depth, and the search ends at the first block with one: the ballot's lowest lane.
//
// enface_project_kernel<NS>, NS = 1, 4 or 8 the slabs it keeps registers for (the call's count rounded up; the same arithmetic in
// each).  With a surface the wave first takes the lower median of up to 15 raw surfaces, one a lane, by rank.  It then walks the
// blocks of 256 depths between the first and the last depth of the A-scan's clipped slabs and skips those no slab meets; the next
// block's loads are issued before this block's depths are added.  Of a block lane l holds depths 4 l .. 4 l + 3: one 16-byte load
// where the A-scan's first depth lies on a 16-byte address and the four depths exist, else 4-byte loads of those that exist -- the
// same depths in the same lanes either way, so the volume's address never enters a result.  Per slab a lane keeps (sum, max,
// argmax) in registers and adds a block's depths in increasing depth; across lanes the six shuffle steps of the header's butterfly
// follow.  What nothing reads is skipped by branches the whole wave takes alike.  __launch_bounds__(256, 8): eight waves a SIMD, so
// that the capped grid (eight workgroups a compute unit) is resident at once.
#include "fdoct_enface_kernels.h"

#include <cmath>

namespace fdoct {

namespace {

constexpr int kEnfWaves = kEnfBlock / 64;

// The lower median of the valid raw surfaces of A-scans [r - half, r + half] of the position whose first A-scan is z0: lane j holds
// A-scan r - half + j.  Among the valid lanes the ranks by (value, lane) are a permutation of 0 .. k - 1, so one lane has the asked one.
__device__ __forceinline__ int enf_median(const int32_t* z0, int ascans, int r, int median, int lane) {
  const int rr = r - (median - 1) / 2 + lane;
  int x = -1;
  if (lane < median && rr >= 0 && rr < ascans) x = z0[rr];
  const bool valid = x >= 0;
  int rank = 0;
#pragma unroll
  for (int j = 0; j < kEnfMaxMedian; j++) {
    const int xj = __builtin_amdgcn_readlane(x, j);
    rank += (xj >= 0 && (xj < x || (xj == x && j < lane))) ? 1 : 0;
  }
  const int k = __popcll(__ballot(valid));
  if (k == 0) return -1;
  const unsigned long long hit = __ballot(valid && rank == (k - 1) / 2);
  return __shfl(x, __ffsll((long long)hit) - 1);
}

__device__ __forceinline__ float enf_box(const float* s, int smooth) {
  float B = s[0];
  for (int j = 1; j < smooth; j++) B += s[j];
  return B;
}

__global__ __launch_bounds__(kEnfBlock) void enface_surface_kernel(const EnfaceArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int ncand = a.s1 - a.smooth - a.s0 + 1;   // >= 1: the search range holds `smooth` depths
  const long long stride = (long long)gridDim.x * kEnfWaves;
  for (long long row = (long long)blockIdx.x * kEnfWaves + wave; row < a.rows; row += stride) {
    const float* const s = a.structure + row * a.depths + a.s0;
    float thr = a.threshold * (float)a.smooth;
    if (a.surface == 2) {
      float m = -INFINITY;
      for (int i = lane; i < ncand; i += 64) {
        const float B = enf_box(s + i, a.smooth);
        if (B > m) m = B;
      }
#pragma unroll
      for (int k = 32; k >= 1; k >>= 1) {
        const float o = __shfl_xor(m, k);
        if (o > m) m = o;
      }
      thr = a.threshold * m;
    }
    int z = -1;
    for (int c = 0; c < ncand; c += 64) {
      const int i = c + lane;
      bool hit = false;
      if (i < ncand) hit = enf_box(s + i, a.smooth) >= thr;
      const unsigned long long mask = __ballot(hit);
      if (mask) {
        z = a.s0 + c + __ffsll((long long)mask) - 1;
        break;
      }
    }
    if (lane == 0) a.z0[row] = z;
  }
}

// NS: the slabs the instantiation keeps registers for (1, 4 or 8): the same arithmetic in each
template <int NS>
__global__ __launch_bounds__(kEnfBlock, 8) void enface_project_kernel(const EnfaceArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const bool need_sum = a.out_mean != nullptr, need_max = a.out_max != nullptr || a.out_argmax != nullptr;
  const long long stride = (long long)gridDim.x * kEnfWaves;
  for (long long row = (long long)blockIdx.x * kEnfWaves + wave; row < a.rows; row += stride) {
    int z = 0;
    if (a.surface) {
      const long long p = row / a.ascans;
      z = __builtin_amdgcn_readfirstlane(enf_median(a.z0 + p * a.ascans, a.ascans, (int)(row - p * a.ascans), a.median, lane));
    }
    if (a.out_surface && lane == 0) a.out_surface[row] = z;
    if (!need_sum && !need_max) continue;

    int lo[NS], hi[NS];   // the clipped slabs: hi <= lo where nothing remains
    int u0 = a.depths, u1 = 0;                // from their first depth to their last
#pragma unroll
    for (int s = 0; s < NS; s++) {
      lo[s] = hi[s] = 0;
      if (s < a.nslabs && z >= 0) {
        const int f = z + a.first[s];
        lo[s] = max(f, 0), hi[s] = min(f + a.count[s], a.depths);
        if (hi[s] > lo[s]) u0 = min(u0, lo[s]), u1 = max(u1, hi[s]);
      }
    }

    float sum[NS], mx[NS];
    int am[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) sum[s] = 0.f, mx[s] = 0.f, am[s] = -1;

    const float* const v = a.vol + row * a.depths;
    const bool wide = (reinterpret_cast<uintptr_t>(v) & 15) == 0;
    // does a slab meet the block of 256 depths at c?
    auto meets = [&](int c) {
      bool m = false;
#pragma unroll
      for (int s = 0; s < NS; s++) m = m || (lo[s] < c + kEnfChunk && hi[s] > c && hi[s] > lo[s]);
      return m;
    };
    // the lane's four depths of that block
    auto load = [&](int c, float (&x)[4]) {
      const int b0 = c + 4 * lane;
      x[0] = x[1] = x[2] = x[3] = 0.f;
      if (wide && b0 + 3 < a.depths) {
        const float4 t = *reinterpret_cast<const float4*>(v + b0);
        x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (b0 + j < a.depths) x[j] = v[b0 + j];
      }
    };
    // the next block's loads are issued before this block's depths are added
    int c = u0 / kEnfChunk * kEnfChunk;
    float x[4], nx[4] = {0.f, 0.f, 0.f, 0.f};
    bool mc = c < u1 && meets(c);
    if (mc) load(c, x);
    while (c < u1) {
      const int cn = c + kEnfChunk;
      const bool mn = cn < u1 && meets(cn);
      if (mn) load(cn, nx);
      if (mc) {
        const int b0 = c + 4 * lane;
#pragma unroll
        for (int s = 0; s < NS; s++) {
          if (!(lo[s] < c + kEnfChunk && hi[s] > c && hi[s] > lo[s])) continue;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int b = b0 + j;
            const bool in = b >= lo[s] && b < hi[s];
            if (need_sum && in) sum[s] += x[j];
            if (need_max && in && (am[s] < 0 || x[j] > mx[s])) mx[s] = x[j], am[s] = b;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; j++) x[j] = nx[j];
      mc = mn, c = cn;
    }

#pragma unroll
    for (int s = 0; s < NS; s++) {
      if (s >= a.nslabs) continue;
      const int n = hi[s] - lo[s];
      float S = sum[s], M = mx[s];
      int A = am[s];
      if (n > 0) {
        if (need_sum) {
#pragma unroll
          for (int k = 32; k >= 1; k >>= 1) S += __shfl_down(S, k);
        }
        if (need_max) {
#pragma unroll
          for (int k = 32; k >= 1; k >>= 1) {
            const float Mo = __shfl_down(M, k);
            const int Ao = __shfl_down(A, k);
            const bool take = Ao >= 0 && (A < 0 || Mo > M || (Mo == M && Ao < A));
            M = take ? Mo : M, A = take ? Ao : A;
          }
        }
      }
      if (lane == 0) {
        const long long o = (long long)s * a.rows + row;
        if (a.out_mean) a.out_mean[o] = n > 0 ? S / (float)n : 0.f;
        if (a.out_max) a.out_max[o] = n > 0 ? M : 0.f;
        if (a.out_argmax) a.out_argmax[o] = n > 0 ? A : -1;
      }
    }
  }
}

}  // namespace

hipError_t launch_enface(const EnfaceArgs& a, hipStream_t st) {
  if (!a.vol || a.blocks < 1 || a.rows < 1 || a.rows != (long long)a.positions * a.ascans || a.depths < 1) return hipErrorInvalidValue;
  if (a.nslabs < 1 || a.nslabs > kEnfMaxSlabs || a.median < 1 || a.median > kEnfMaxMedian || !(a.median & 1)) return hipErrorInvalidValue;
  if (!a.out_mean && !a.out_max && !a.out_argmax && !a.out_surface) return hipErrorInvalidValue;
  for (int s = 0; s < a.nslabs; s++)   // z + first + count stays an int
    if (a.first[s] <= -a.depths || a.first[s] >= a.depths || a.count[s] < 1 || a.count[s] > 2 * (long long)a.depths) return hipErrorInvalidValue;
  if (a.surface) {
    if (!a.z0 || !a.structure || a.smooth < 1 || a.smooth > kEnfMaxSmooth) return hipErrorInvalidValue;
    if (a.s0 < 0 || a.s1 > a.depths || a.s1 - a.s0 < a.smooth) return hipErrorInvalidValue;   // every box sum stays inside the A-scan
    hipLaunchKernelGGL(enface_surface_kernel, dim3((unsigned)a.blocks), dim3(kEnfBlock), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  } else if (a.out_surface) {
    return hipErrorInvalidValue;
  }
  if (a.nslabs == 1)
    hipLaunchKernelGGL(enface_project_kernel<1>, dim3((unsigned)a.blocks), dim3(kEnfBlock), 0, st, a);
  else if (a.nslabs <= 4)
    hipLaunchKernelGGL(enface_project_kernel<4>, dim3((unsigned)a.blocks), dim3(kEnfBlock), 0, st, a);
  else
    hipLaunchKernelGGL(enface_project_kernel<kEnfMaxSlabs>, dim3((unsigned)a.blocks), dim3(kEnfBlock), 0, st, a);
  return hipGetLastError();
}

}  // namespace fdoct
