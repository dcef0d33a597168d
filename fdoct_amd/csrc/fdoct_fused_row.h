// fdoct_fused_row.h -- the pieces of fused_kernel's row loop (fdoct_kernels.hip) that are functions: row slots and tickets, the
// real-path untangle with its magnitudes, the full-frame background's prefetch (issue_ib2d), the resident plane loads
// (load_plane) and the second word of the fast path's division (second_word).  The other phases are lambdas and blocks of the
// kernel: profiles/fused_phases_codeobj_identity.txt says which were tried as functions and what differed.
// X is the kernel's FusedTraits; `a` its arguments; l the lane inside its row group, lane the lane in the wave.
#pragma once
#include "fdoct_fused_dev.h"
#include "fdoct_fused_traits.h"

namespace fdoct {

// ------------------------------------------------------------ row ticket --
// Row slots: slot s of this workgroup is rows (s*gridDim.x + blockIdx.x)*RPW .. +RPW-1, so the chip sweeps the
// batch front to back.  Waves take slots from a workgroup-wide ticket counter instead of a fixed stride: the
// hardware favours the oldest wave of a SIMD, which with a static split finishes its share long before its
// younger sibling and leaves the SIMD with one wave for the last quarter of the launch.
template <class X>
__device__ __forceinline__ long long slot_row(unsigned s) {
  return ((long long)s * gridDim.x + blockIdx.x) * X::RPW;
}
// one row per wave (T == 64): everything row-related is wave-uniform; saying so keeps the 64-bit row arithmetic on the
// scalar unit (the compiler cannot see it through the loop-carried ticket)
template <class X>
__device__ __forceinline__ long long uni64(long long v) {
  if constexpr (X::RPW == 1) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
  } else {
    return v;
  }
}
// A claimed ticket as the wave-uniform value it is (the claiming lane's).
__device__ __forceinline__ unsigned ticket_value(unsigned t) { return (unsigned)__builtin_amdgcn_readfirstlane((int)t); }

// The claim of a row top: a row slot -- or, with four rows per wave, a tile, which only a group's leader (mem == 0) claims.
template <class X, class Claim>
__device__ __forceinline__ unsigned claim_row(const Claim& claim, unsigned mem) {
    if constexpr (X::TRO_INPLACE) return mem == 0u ? claim() : 0u;
    return claim();
}

// ------------------------------------------------------------ magnitudes (A8) --
// Real path: the untangle of the NC-point complex transform of a 2 NC-point real row, and the magnitudes of both halves.
// Bins k and NC-k come out of the same two values: with Zp = Z[NC-k],
//   A = Z[k] + conj(Zp), B = Z[k] - conj(Zp), q = w^k * B:  2X[k] = A - i*q,  2|X[NC-k]| = |A + i*q|
// (E[NC-k] = conj E[k], O[NC-k] = conj O[k], w^(NC-k) = -conj w^k; the 1/2 is folded into the
// window on the host).  So each lane takes its LOWER-half registers m < P/2 (bins k = l + T*m <
// NC/2), fetches the partner Z[NC-k] from lane (T-l)%T -- register P-1-m there, or (P-m)%P when
// l == 0 -- and produces both magnitudes: half the permutes and half the arithmetic of doing
// every bin on its own.  acc[m] = |X[l + T*m]|, acc[P/2 + m] = |X[NC - l - T*m]|; the slot that
// would be bin NC (lane 0, m = 0) carries bin NC/2 (self-paired, lane 0 register P/2) instead.
template <class X>
__device__ __forceinline__ void untangle_magnitudes(const v2f* z, float* acc, v2f utw, int lane, int l) {
  constexpr int T = X::T, P = X::P;
  const int plane = ((lane & ~(T - 1)) | ((T - l) & (T - 1))) << 2;  // byte address for bpermute
  // keep the per-bin phasors utw*const from being hoisted out of the row loop (they would cost
  // resident registers or, worse, scratch reloads): utw is opaque from here
  v2f utw_row = utw;
  asm volatile("" : "+v"(utw_row));
  constexpr int PH = P / 2;
  v2f pz[PH];
  // every lane publishes the register its reader wants; all permutes are issued before any of
  // the arithmetic (one LDS round trip)
  static_for<0, PH>([&](auto mc) {
    constexpr int m = decltype(mc)::value;
    constexpr int pm1 = P - 1 - m;      // asked for by lane T-l' != 0
    constexpr int pm0 = (P - m) % P;    // asked for by lane 0 (of itself)
    const float sx = (l == 0) ? z[pm0].x : z[pm1].x;
    const float sy = (l == 0) ? z[pm0].y : z[pm1].y;
    pz[m] = mk(__int_as_float(__builtin_amdgcn_ds_bpermute(plane, __float_as_int(sx))),
               __int_as_float(__builtin_amdgcn_ds_bpermute(plane, __float_as_int(sy))));
  });
  __builtin_amdgcn_sched_barrier(0);
  static_for<0, PH>([&](auto mc) {
    constexpr int m = decltype(mc)::value;
    const v2f A_ = add_conj(z[m], pz[m]);
    const v2f B_ = sub_conj(z[m], pz[m]);
    // w^k = exp(2*pi*i*(l + T*m)/N) = utw * exp(2*pi*i*m/(2P))
    const v2f q = cmul(twc<m, 2 * P, true>(utw_row), B_);
    const v2f Xa = add_mulmi(A_, q);   // A - i*q
    const v2f Xb = sub_mulmi(A_, q);   // A + i*q
    const v2f Xa2 = Xa * Xa, Xb2 = Xb * Xb;
    const float lo_mag = fast_sqrt(Xa2.x + Xa2.y);
    acc[m] = X::AVG ? acc[m] + lo_mag : lo_mag;
    float hi2 = Xb2.x + Xb2.y;
    if constexpr (m == 0) {
      // bin NC/2: Z[NC/2] = zc is its own partner and only lane 0 keeps the result, so only lane 0's phasor counts:
      // utw = (1, +-0) there (exp of 0) and the PH/(2P) turn is an exact quarter turn.  Run through the general formula
      // that gives  A = zc + conj(zc) = (2x, +0),  B = zc - conj(zc) = (+0, 2y),  q = i*utw*B = (-2y, +0) and
      // X = A - i*q = (2x + 0, 0 + 2y): every step is exact (doubling is; x - x and the products with 0 are zeros,
      // and adding a zero changes at most the sign of a zero), so X is zc + zc up to the sign of a zero component.
      // The square discards that sign (both give +0), hence |X|^2 below has the bits the general formula had for
      // every finite zc, zeros of either sign included -- and one square root serves both selections.
      const v2f Xc = z[PH] + z[PH];
      const v2f Xc2 = Xc * Xc;
      const float mid2 = Xc2.x + Xc2.y;
      hi2 = (l == 0) ? mid2 : hi2;
    }
    const float hi = fast_sqrt(hi2);
    acc[PH + m] = X::AVG ? acc[PH + m] + hi : hi;
  });
}

// IB2D: (re)load r_ib with the reciprocal-background row of output row o (any o: rows repeat every H)
template <class X>
__device__ __forceinline__ void issue_ib2d(const FusedArgs& a, long long o, v2f* r_ib, uint4* r_il16, unsigned char* il_dma, int l) {
  constexpr int T = X::T, WCH = X::WCH;
  constexpr bool IB2D = X::IB2D;
  if constexpr (IB2D) {
    const unsigned rr = (o < a.total_out_rows) ? (unsigned)o % (unsigned)a.H : 0u;  // host guarantees rows < 2^31
    const float4* p4 = reinterpret_cast<const float4*>(a.ib2d + (size_t)rr * X::WC + 8 * l);
#pragma unroll
    for (int c = 0; c < WCH; c++) {
      const float4 q0 = p4[2 * T * c], q1 = p4[2 * T * c + 1];
      evens_odds_pairs(q0, q1, r_ib + 4 * c);
    }
    if constexpr (X::ILDMA) {
      typedef const __attribute__((address_space(1))) void* gptr_t;
      typedef __attribute__((address_space(3))) void* lptr_t;
      const uint4* h4 = reinterpret_cast<const uint4*>(a.il16_2d) + (size_t)rr * (X::WC / 8) + l;
#pragma unroll
      for (int c = 0; c < WCH; c++)   // lane l's 16 bytes of chunk c land at slot + (c T + l) 16: the order the row top reads them in
        __builtin_amdgcn_global_load_lds((gptr_t)(h4 + T * c), (lptr_t)(il_dma + c * T * 16), 16, 0, 0);
    } else if constexpr (X::IL16) {
      const uint4* h4 = reinterpret_cast<const uint4*>(a.il16_2d) + (size_t)rr * (X::WC / 8) + l;
#pragma unroll
      for (int c = 0; c < WCH; c++) r_il16[c] = h4[T * c];
    }
  }
}

// IL16: d plus what the first word of 1/background leaves out, c0 * rho, rho * 2^38 being pair i of the lane's half floats ilh
// (c0s = c0 * 2^-38; the row top in the kernel says why that is enough).
template <class X>
__device__ __forceinline__ v2f second_word(const uint4* ilh, float c0s, v2f d, int i) {
  if constexpr (X::IL16) {
    const uint4 hq = ilh[i >> 2];
    const uint32_t hp = (i & 3) == 0 ? hq.x : (i & 3) == 1 ? hq.y : (i & 3) == 2 ? hq.z : hq.w;
    return mk(fma_mix_lo(c0s, hp, d.x), fma_mix_hi(c0s, hp, d.y));
  } else {
    return d;
  }
}

// Chunk c of a per-column table straight from global memory (W == WC), 32 bytes per lane, into the RawChunk pair order.
template <int T>
__device__ __forceinline__ void load_plane(const float* tab, int c, v2f* out, int l) {
  const float4* p4 = reinterpret_cast<const float4*>(tab + 8 * (l + T * c));
  const float4 q0 = p4[0], q1 = p4[1];
  out[0] = mk(q0.x, q0.z);
  out[1] = mk(q1.x, q1.z);
  out[2] = mk(q0.y, q0.w);
  out[3] = mk(q1.y, q1.w);
}

// 2^-38: the scale of the half-float pattern of the second word of 1/background (kPrec16Shift on the host)
constexpr float kTwoPowMinus38 = 3.637978807091713e-12f;

}  // namespace fdoct
