// fdoct_fused_dev.h -- device helpers shared by the phases of fused_kernel (fdoct_kernels.hip): the measurement builds' switches,
// the same-wave LDS hand-off, the packed sample chunk of each input type, the group reductions and the constant-plane read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdoct_fft_reg.h"
#include "fdoct_kernels.h"

namespace fdoct {

// Stage-skipping profiling aid (tools/ablate.sh): only in builds with -DFDOCT_RUNTIME_ABLATE.
#ifdef FDOCT_RUNTIME_ABLATE
#define FDOCT_ABL(bit) ((a.ablate & (bit)) != 0)
#elif defined(FDOCT_CT_ABLATE)  // compile-time mask: the skipped stage costs nothing at all (one build per mask)
#define FDOCT_ABL(bit) (((FDOCT_CT_ABLATE) & (bit)) != 0)
#else
#define FDOCT_ABL(bit) false
#endif

// Orders this wave's LDS traffic: a wave's DS operations execute in program
// order, so a compiler-level fence is all a same-wave write->read hand-off needs.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Where a row's cycles go (measurement builds, -DFDOCT_FUSED_PROBE; tools/mkvariant.sh): the cycle counter is read at the phase
// boundaries of the row loop and the differences summed per phase over a wave's rows.  (Each read waits for the wave's
// outstanding LDS / scalar-memory operations -- s_memtime returns through the same counter -- so a phase is charged with the
// latency of what it issued; the build is for attribution, its rate is a few per cent below the shipped kernel's.)
#ifdef FDOCT_FUSED_PROBE
struct FusedProbe {
  unsigned long long acc[FUSED_PROBE_PHASES] = {}, t = 0;
  __device__ __forceinline__ void start() { t = __builtin_readcyclecounter(); }
  __device__ __forceinline__ void mark(int i) {
    // (scheduling barriers either side: without them the compiler moves a phase's arithmetic across the read -- the first
    // build of this probe showed 0.1 % for the radix-16 step)
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long n = __builtin_readcyclecounter();
    __builtin_amdgcn_sched_barrier(0);
    acc[i] += n - t;
    t = n;
  }
};
#define FDOCT_FPR(p, i) (p).mark(i)
#else
struct FusedProbe {};
#define FDOCT_FPR(p, i) do {} while (0)
#endif

// ------------------------------------------------------------ input types --
// One 8-sample chunk s0..s7 of a row as loaded (prefetched) from HBM.  unpack() gives the four pairs
// (s0,s2) (s4,s6) (s1,s3) (s5,s7): evens and odds apart, so that the slope step's "previous sample" of an odd
// pair IS the even pair, and the de-interleaved staging stores are whole registers quads (no shuffles).
// chunk_pair_offset(q) = index of the first sample of pair q; the second one is two samples later.
__device__ __forceinline__ constexpr int chunk_pair_offset(int q) { return (q & 1) * 4 + (q >> 1); }
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
typedef uint32_t u2v __attribute__((ext_vector_type(2)));
template <typename IN_T>
struct RawChunk;
template <>
struct RawChunk<uint16_t> {
  uint4 v;
  __device__ __forceinline__ void load(const void* row, int i0) {
    // streaming load: camera samples are read once (nt keeps them from displacing the twiddle / plane lines in L2; +1.2 %,
    // DESIGN.md 5 -- the sc0/sc1 scope bits change nothing)
    const u4v t = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(static_cast<const uint16_t*>(row) + i0));
    v = make_uint4(t.x, t.y, t.z, t.w);
  }
  __device__ __forceinline__ void zero() { v = make_uint4(0, 0, 0, 0); }
  __device__ __forceinline__ void pin() { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
  __device__ __forceinline__ void pin_ordered() { asm volatile("" : "+v"(v.x) : : "memory"); }
  __device__ __forceinline__ void unpack(v2f* x) const {
    x[0] = mk((float)(v.x & 0xffffu), (float)(v.y & 0xffffu));
    x[1] = mk((float)(v.z & 0xffffu), (float)(v.w & 0xffffu));
    x[2] = mk((float)(v.x >> 16), (float)(v.y >> 16));
    x[3] = mk((float)(v.z >> 16), (float)(v.w >> 16));
  }
};
template <>
struct RawChunk<uint8_t> {
  uint2 v;
  __device__ __forceinline__ void load(const void* row, int i0) {
    const u2v t = __builtin_nontemporal_load(reinterpret_cast<const u2v*>(static_cast<const uint8_t*>(row) + i0));
    v = make_uint2(t.x, t.y);
  }
  __device__ __forceinline__ void zero() { v = make_uint2(0, 0); }
  __device__ __forceinline__ void pin() { asm volatile("" : "+v"(v.x), "+v"(v.y)); }
  __device__ __forceinline__ void pin_ordered() { asm volatile("" : "+v"(v.x) : : "memory"); }
  __device__ __forceinline__ void unpack(v2f* x) const {
    x[0] = mk((float)(v.x & 0xffu), (float)((v.x >> 16) & 0xffu));
    x[1] = mk((float)(v.y & 0xffu), (float)((v.y >> 16) & 0xffu));
    x[2] = mk((float)((v.x >> 8) & 0xffu), (float)(v.x >> 24));
    x[3] = mk((float)((v.y >> 8) & 0xffu), (float)(v.y >> 24));
  }
};
template <>
struct RawChunk<float> {
  float4 a, b;
  __device__ __forceinline__ void load(const void* row, int i0) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v* p = reinterpret_cast<const f4v*>(static_cast<const float*>(row) + i0);
    const f4v ta = __builtin_nontemporal_load(p), tb = __builtin_nontemporal_load(p + 1);
    a = make_float4(ta.x, ta.y, ta.z, ta.w);
    b = make_float4(tb.x, tb.y, tb.z, tb.w);
  }
  __device__ __forceinline__ void zero() { a = b = make_float4(0, 0, 0, 0); }
  __device__ __forceinline__ void pin() {
    asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w), "+v"(b.x), "+v"(b.y), "+v"(b.z), "+v"(b.w));
  }
  __device__ __forceinline__ void pin_ordered() { asm volatile("" : "+v"(a.x) : : "memory"); }
  __device__ __forceinline__ void unpack(v2f* x) const {
    x[0] = mk(a.x, a.z);
    x[1] = mk(b.x, b.z);
    x[2] = mk(a.y, a.w);
    x[3] = mk(b.y, b.w);
  }
};

template <int T>
__device__ __forceinline__ float group_min(float v) {
#pragma unroll
  for (int m = T / 2; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
  return v;
}
template <int T>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int m = T / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

// One DPP step of a wave-wide f64 sum: v + (v moved by `CTRL`).  Only lane 63's total is used, so lanes that
// the row mask leaves unwritten may hold anything; row shifts read 0 past the row edge (bound_ctrl).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add_f64(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int tlo = __builtin_amdgcn_mov_dpp(lo, CTRL, ROW_MASK, 0xf, true);
  const int thi = __builtin_amdgcn_mov_dpp(hi, CTRL, ROW_MASK, 0xf, true);
  return v + __hiloint2double(thi, tlo);
}

// Sum over the T lanes of a row group, returned to every lane of the group.  T == 64: DPP
// row shifts / broadcasts (no LDS, no address registers) and a scalar broadcast of lane 63.
template <int T>
__device__ __forceinline__ double group_sum(double v) {
  if constexpr (T == 64) {
    v = dpp_add_f64<0x111, 0xf>(v);  // row_shr:1  -> lane i: v[i-1..i]
    v = dpp_add_f64<0x112, 0xf>(v);  // row_shr:2  -> v[i-3..i]
    v = dpp_add_f64<0x114, 0xf>(v);  // row_shr:4  -> v[i-7..i]
    v = dpp_add_f64<0x118, 0xf>(v);  // row_shr:8  -> lane 15 of each row: the row's total
    v = dpp_add_f64<0x142, 0xa>(v);  // row_bcast:15 -> rows 1,3 add the previous row's total
    v = dpp_add_f64<0x143, 0xc>(v);  // row_bcast:31 -> rows 2,3 add lane 31
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
    return __hiloint2double(hi, lo);
  } else {
#pragma unroll
    for (int m = T / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
  }
}

// One DPP step of a wave-wide f32 sum (lanes the row mask leaves out add 0).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add_f32(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, true));
}
// The two cross-row steps of that sum, one v_add_f32_dpp each: row_bcast:15 into rows 1 and 3, then row_bcast:31 into rows 2
// and 3.  The destination is tied to v, so rows outside a mask keep v.  (Written with the builtin above, each step is three
// instructions -- a zero, a v_mov_b32_dpp into it, an add: the compiler does not fold a partial row mask into a float add,
// because the rows left out would hold v where the source says v + 0, and those differ for v = -0.)  That difference cannot
// reach group_sum_f32's result, which is lane 63 alone: lane 63 is in both masks, so it is added to in both steps; what it
// adds is lane 47 as the row shifts left it (a DPP step reads its sources before any lane is written) and then lane 31, which
// is in row 1 and so was itself added to in the first step.  No lane that a mask leaves out is read again.
// The compiler does not see a DPP read inside an asm statement, so the two wait states that a VALU write of v needs before
// a DPP read of it are in the statement itself.  The five that a VALU write of EXEC (v_cmpx) needs before a DPP operation are
// not: the callers run this at the top level of a row, with every lane on (which the broadcasts assume as well: no bound_ctrl),
// and the compiler writes EXEC from the scalar unit there.  A caller under a v_cmpx would have to wait them out itself.
__device__ __forceinline__ float dpp_add_cross_rows_f32(float v) {
  asm("s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf"
      : "+v"(v));
  return v;
}

// Sum over the T lanes of a row group in f32, returned to every lane of the group (T == 64: the DPP chain of
// group_sum; ONE_EACH: one v_add_f32_dpp per step, the cross-row steps included -- the same bits either way).
template <int T, bool ONE_EACH>
__device__ __forceinline__ float group_sum_f32(float v) {
  if constexpr (T == 64) {
    v = dpp_add_f32<0x111, 0xf>(v);
    v = dpp_add_f32<0x112, 0xf>(v);
    v = dpp_add_f32<0x114, 0xf>(v);
    v = dpp_add_f32<0x118, 0xf>(v);
    if constexpr (ONE_EACH) {
      v = dpp_add_cross_rows_f32(v);
    } else {
      v = dpp_add_f32<0x142, 0xa>(v);
      v = dpp_add_f32<0x143, 0xc>(v);
    }
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
  } else {
#pragma unroll
    for (int m = T / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
  }
}

// fma with a half-float second operand (the low / high half of hp), converted inside the instruction: a * f16(hp) + c.
__device__ __forceinline__ float fma_mix_lo(float a, uint32_t hp, float c) {
  float r;
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[0,1,0]" : "=v"(r) : "v"(a), "v"(hp), "v"(c));
  return r;
}
__device__ __forceinline__ float fma_mix_hi(float a, uint32_t hp, float c) {
  float r;
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(r) : "v"(a), "v"(hp), "v"(c));
  return r;
}

// Reads the 8 constants of chunk c of one constant plane pair in the RawChunk pair order.
// Plane layout (see the staging loop in the kernel): chunk c, parity h, lane ln -> c*8T + h*4T + 4*ln.
template <int T>
__device__ __forceinline__ void load_consts(const float* plane_lane, int c, v2f* out) {
  const float4 q0 = *reinterpret_cast<const float4*>(plane_lane + 8 * T * c);
  const float4 q1 = *reinterpret_cast<const float4*>(plane_lane + 8 * T * c + 4 * T);
  out[0] = mk(q0.x, q0.y);
  out[1] = mk(q0.z, q0.w);
  out[2] = mk(q1.x, q1.y);
  out[3] = mk(q1.z, q1.w);
}

// The four sample pairs of an 8-sample group that is stored evens first, then odds (a.ib2d, a.il2d): the RawChunk pair order.
__device__ __forceinline__ void evens_odds_pairs(const float4& q0, const float4& q1, v2f* out) {
  out[0] = mk(q0.x, q0.y);
  out[1] = mk(q0.z, q0.w);
  out[2] = mk(q1.x, q1.y);
  out[3] = mk(q1.z, q1.w);
}

// One sample pair into a running minimum and maximum (the row-wise normalisation of both kernel forms).
__device__ __forceinline__ void pair_minmax(const v2f& p, float& mn, float& mx) {
  mn = fminf(mn, fminf(p.x, p.y));
  mx = fmaxf(mx, fmaxf(p.x, p.y));
}

}  // namespace fdoct
