// fdoct_manualavg.hip -- manual averaging of B-scans (include/fdoct_manualavg.h), BscanFFT.cpp:1399-1444:
//   if (manualaccumcount < manualaverages) { accumulate(bscan, manualaccum); manualaccumcount++; }
//   else { manualaccumcount = 0; manualaccum = manualaccum / manualaverages; log(manualaccum, manualaccum);
//          bscandispmanual = 20.0 * manualaccum / 2.303; ...; manualaccum = Mat::zeros(...); }
// for all the B-scans of a call as ONE kernel.  A lane owns elements of the image (four side by side where 16-byte accesses are
// possible, one otherwise), loads their running sums from the accumulator once, walks the call's images in order with the sums
// in registers as doubles, writes mean and dB at every emission position (and zeroes the sums there), and stores the sums once.
// The pass moves every input byte once (an image the reference's mode drops is not fetched unless it is the call's last), every
// emitted byte once and 16 bytes of accumulator per element: it is bandwidth-bound, and nothing but the additions depends on a load, so the loop
// issues the loads of MAVG_UNROLL images before it adds the first of them.
// Where an emission falls follows from (accumulated, m, mode) alone (ManualAvgArgs::first / period), so every branch on it is
// uniform across the launch.  Per element the arithmetic is the same on both paths -- the sums in image order, one IEEE division
// by m, the logarithm, 20.0 * that, / 2.303, all in double, one rounding to float -- so paths, memory spaces, reruns and any
// split of a sequence of images into calls give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "fdoct_manualavg_kernels.h"

namespace fdoct {

namespace {

constexpr int MAVG_BLOCK = 256;
constexpr int MAVG_WAVES_PER_CU = 16;
constexpr int MAVG_UNROLL = 8;  // images whose loads are in flight per lane: 8 x 16 bytes

template <int W> struct MavgVec;
template <> struct MavgVec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
  static __device__ __forceinline__ void store(float* p, const float (&x)[1]) { *p = x[0]; }
  static __device__ __forceinline__ void load_sums(const double* p, double (&s)[1]) { s[0] = *p; }
  static __device__ __forceinline__ void store_sums(double* p, const double (&s)[1]) { *p = s[0]; }
};
template <> struct MavgVec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  }
  static __device__ __forceinline__ void store(float* p, const float (&x)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
  }
  static __device__ __forceinline__ void load_sums(const double* p, double (&s)[4]) {
    const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
    s[0] = a.x, s[1] = a.y, s[2] = b.x, s[3] = b.y;
  }
  static __device__ __forceinline__ void store_sums(double* p, const double (&s)[4]) {
    *reinterpret_cast<double2*>(p) = make_double2(s[0], s[1]);
    *reinterpret_cast<double2*>(p + 2) = make_double2(s[2], s[3]);
  }
};

// Elements e .. e + W - 1 (all inside the image) through the whole call.
template <int W>
__device__ __forceinline__ void mavg_elements(const ManualAvgArgs& a, long long e) {
  const float* __restrict__ in = a.in + e;
  double s[W];
  MavgVec<W>::load_sums(a.acc + e, s);
  const double dm = (double)a.m;
  int next = a.first;      // the next emission position
  long long out = e;       // ... and where it goes: slot * count + e
  for (int i0 = 0; i0 < a.nb; i0 += MAVG_UNROLL) {
    MavgVec<W> x[MAVG_UNROLL];
    int nl = next;
#pragma unroll
    for (int u = 0; u < MAVG_UNROLL; u++) {
      // no branch around a load (the compiler would wait for every load in flight at each): a slot past the last image, or of
      // an image that is dropped, repeats the address of a neighbouring slot, and nothing reads what it loads
      const int i = i0 + u;
      const bool emit = i == nl;
      if (emit) nl += a.period;
      x[u].load(in + (long long)min(i + (a.drop && emit ? 1 : 0), a.nb - 1) * a.count);
    }
    // the loads are issued here, whole and before the first addition: the compiler may not move one below this line (it
    // otherwise sinks the first image's load into a branch of its own and waits there for all of them)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int u = 0; u < MAVG_UNROLL; u++) {
      const int i = i0 + u;
      const bool live = i < a.nb, emit = live && i == next;
      // 1403: accumulate(bscan, manualaccum), as a select: the only branches of the loop are the emissions
      const bool add = live && !(a.drop && emit);
#pragma unroll
      for (int k = 0; k < W; k++) s[k] = add ? s[k] + (double)x[u].v[k] : s[k];
      if (emit) {
        float mean[W], db[W];
#pragma unroll
        for (int k = 0; k < W; k++) {
          const double q = s[k] / dm;                                      // 1419
          mean[k] = (float)q;
          db[k] = a.out_db ? (float)(__dmul_rn(20.0, log(q)) / 2.303) : 0.f;  // 1421-1423
          s[k] = 0.0;                                                      // 1444
        }
        if (a.out_mean) MavgVec<W>::store(a.out_mean + out, mean);
        if (a.out_db) MavgVec<W>::store(a.out_db + out, db);
        out += a.count;
        next += a.period;
      }
    }
  }
  MavgVec<W>::store_sums(a.acc + e, s);
}

template <bool VEC>
__global__ __launch_bounds__(MAVG_BLOCK) void manualavg_kernel(ManualAvgArgs a) {
  const long long tid = (long long)blockIdx.x * MAVG_BLOCK + threadIdx.x, stride = (long long)gridDim.x * MAVG_BLOCK;
  const long long quads = VEC ? a.count >> 2 : 0;
  for (long long q = tid; q < quads; q += stride) mavg_elements<4>(a, q << 2);
  for (long long e = (quads << 2) + tid; e < a.count; e += stride) mavg_elements<1>(a, e);  // everything, or the count % 4 tail
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

void manualavg_plan_launch(ManualAvgArgs* a, int num_cu) {
  // images and slots are `count` floats apart: beyond the first of either, groups of four stay aligned only if count % 4 == 0
  const bool one_image = a->nb == 1;  // (one image emits at most once: slot 0)
  a->vec = a->count >= 4 && (a->count % 4 == 0 || one_image) && aligned16(a->in) && aligned16(a->acc) &&
           (!a->out_mean || aligned16(a->out_mean)) && (!a->out_db || aligned16(a->out_db));
  const long long items = a->vec ? (a->count >> 2) + (a->count & 3) : a->count;
  const long long resident = resident_blocks(num_cu, MAVG_WAVES_PER_CU, MAVG_BLOCK);
  a->blocks = (int)std::max(1LL, std::min((items + MAVG_BLOCK - 1) / MAVG_BLOCK, resident));
}

hipError_t launch_manualavg(const ManualAvgArgs& a, hipStream_t st) {
  auto k = a.vec ? manualavg_kernel<true> : manualavg_kernel<false>;
  hipLaunchKernelGGL(k, dim3(a.blocks), dim3(MAVG_BLOCK), 0, st, a);
  return hipGetLastError();
}

}  // namespace fdoct
