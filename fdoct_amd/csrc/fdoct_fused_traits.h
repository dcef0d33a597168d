// fdoct_fused_traits.h -- what one instantiation of fused_kernel (fdoct_kernels.hip) derives from its template parameters: the
// sizes, and every compile-time switch of the row loop with the reason it exists.  The kernel and the pieces of it in
// fdoct_fused_tro.h and fdoct_fused_row.h read them as X::NAME.  The rules shared with the host stay in fdoct_fused_rules.h
// and are called from here.
#pragma once
#include "fdoct_kernels.h"

namespace fdoct {

template <int LOG2NC, int T_, int R1, int R2, int R3, int KIND, int WCH_, typename IN_T, bool CPLX, bool LEAN_, int STAGE_, bool AVG_,
          bool IB2D_, int NORM, bool TRO, bool PRECT>
struct FusedTraits {
  // the kernel's own parameters that the pieces outside the kernel read (see the comment in front of fused_kernel)
  static constexpr int T = T_, WCH = WCH_, STAGE = STAGE_;
  static constexpr bool AVG = AVG_, LEAN = LEAN_, IB2D = IB2D_;

  static constexpr int NC = 1 << LOG2NC;
  static constexpr int P = NC / T;
  static constexpr int RPW = 64 / T;  // rows per wave
  static constexpr int WC = 8 * T * WCH;
  static constexpr int NPR = 4 * WCH;  // sample pairs per lane
  static constexpr int LP = (R1 == 32) ? 5 : (R1 == 16) ? 4 : (R1 == 8) ? 3 : 2;
  static_assert(R1 * R2 * R3 == NC, "radix plan");
  static_assert(KIND == 0 || (KIND == 1 && T == 64 && R1 == 16 && R2 == 4 && R3 == 16) ||
                    (KIND == 2 && T == 64 && R1 == 32 && R2 == 4 && R3 == 16),
                "row-swap plans are 16 x 4 x 16 / 32 x 4 x 16 on a full wave");
  static constexpr int NPASS = (R3 > 1) ? 3 : 2;
  static_assert(P % 4 == 0, "gather table is read four entries at a time");
  // 1/background as two floats (fdoct_capi.cpp::reciprocal_words): always on the any-option kernel; the fast path has both
  // instantiations (PRECT: fdoct_set_precise_division)
  static constexpr bool PREC = !LEAN || PRECT;
  // the second word's form on the fast-path kernels with at most 32 samples per lane: a plane of half floats (fdoct_fused_rules.h)
  static constexpr bool IL16 = PRECT && fused_il_half(LEAN, WCH);
  static_assert(!(PRECT && !LEAN), "the any-option kernel always multiplies by both words");
  static_assert(!(PRECT && IB2D && !IL16), "a full-frame background on the fast path: the second word is prefetched as half floats");

  // The row loop's trims (one v_add_f32_dpp per cross-row step of the wave sums; the row ticket as a plain ds_add_rtn_u32): the
  // same results bit for bit, taken where they are measured to pay -- the 1024-point one-exchange plan writing rows.  The
  // transposed-store kernels are at 256 VGPRs with scratch and allocate worse with either; with the ticket's wait fixed inside
  // an asm statement the plans with four rows per wave lose what the compiler gains by placing it (EXPERIMENTS.md section 7).
  static constexpr bool TRIM = KIND == 1 && !TRO;
  static_assert(!TRO || (LEAN && STAGE == 0 && !CPLX && fused_tro_compiled(KIND, T, WCH) && (FUSED_TR_ROWS % (64 / T)) == 0),
                "fused transposed store: fast path; a wave's rows lie in one tile");
  // (transposed-store kernels leave out of LDS what they read once into registers, so that the ring of finished rows can be
  // larger: fdoct_fused_rules.h, fused_tw3_in_lds / fused_gi_in_lds)
  static constexpr bool TW3_LDS = fused_tw3_in_lds(KIND, LEAN, STAGE, TRO, IB2D && IL16), GI_LDS = fused_gi_in_lds(KIND, LEAN, STAGE, CPLX, AVG, TRO);

  // Fast-path row-swap plan (the benchmark configuration): everything that does not depend on the row --
  // the per-column constants, the gather addresses and the FFT twiddles -- stays in registers (2 waves per
  // SIMD, 256 VGPRs), which removes half of the LDS traffic per row.  Every other instantiation re-reads
  // them from LDS each row.
  static constexpr bool RES = fused_resident_consts(KIND, LEAN, AVG, WCH, STAGE);
  static constexpr bool GRES = LEAN && STAGE != 2 && KIND == 1 && !CPLX && !AVG;  // (with averaging the accumulators need those registers)
  static constexpr bool RESTW = LEAN && KIND == 1 && STAGE != 1;
  // IB2D + both words: the half-float pattern of the same background row is prefetched with it -- into a per-wave LDS slot by
  // the global -> LDS loads of gfx950 (global_load_lds_dwordx4: no registers held through the transform; ILDMA), or, where the
  // LDS belongs to the ring of the transposed store, into 16 registers
  static constexpr bool ILDMA = IB2D && IL16 && !TRO;
  // (the transposed-store variant, and every variant that multiplies by both words of the reciprocal background, is a
  // few registers over the budget with everything resident: their 12 step-3 twiddles come from LDS every row)
  static constexpr int RES2 = !RESTW ? 0 : (TRO ? 0 : (PREC ? (IL16 ? ((IB2D && !ILDMA) ? FDOCT_PREC16_T2_IB2D : (ILDMA ? FDOCT_PREC16_T2_DMA : FDOCT_PREC16_T2)) : FDOCT_PREC_T2) : 12));
  // (the transposed store with a full-frame background and both words holds 48 prefetch registers: its step-5 twiddles come
  // from LDS too, or the row loop spills)
  static constexpr bool RES3 = RESTW && !(TRO && IB2D && IL16);
  static_assert(TW3_LDS || RES3, "the step-5 table stays out of LDS only where its entries are resident");
  static_assert(GI_LDS || GRES, "the gather table stays out of LDS only where its addresses are resident");
  static_assert(!(IB2D || NORM) || (RES && STAGE == 0), "fast-path options: resident-constant kernels only");
  // The averaging fast-path kernels with more than 32 samples per lane (C4): the half-float pattern of the second word stays
  // RESIDENT -- 4 registers per chunk, loaded once per wave (the kernel has them to spare since the low words' source became a
  // compile-time property) -- instead of sixteen 16-byte loads of the float low words per input A-scan from the global plane.
  static constexpr bool IL16R = LEAN && PRECT && fused_il_global(LEAN, AVG, WCH, T) && STAGE != 2;
  // The ticket is claimed a row's work before it is consumed: at the row top for the prefetch in mid-row, or -- in
  // the FFT-stage kernel, which prefetches at the row top -- one whole row ahead (EARLY).
  static constexpr bool EARLY = STAGE == 2;
  // Two-word division on the fast-path kernels with at most 32 samples per lane (PREC): the 32 low words of a lane are
  // row-invariant, but there is no register to keep them in through the transform; they are read from the workgroup's LDS
  // plane at every row top (ilx).  (Re-loading them from a global plane behind the previous pass's magnitudes instead -- older
  // than the row's stores, so that the wait never includes a store -- was measured and lost: 489-491 against 509 M A-scans/s
  // on C2, tools/ab.sh.  The LDS-bound averaging kernels with more samples per lane do read them from global memory: prec == 3.)
  static constexpr bool ILX = PREC && LEAN && WCH <= 4;
  static_assert(!IL16 || ILX, "half-float second word: the kernels that read the row's low words at its top");
  // staging layout (even/odd sample planes when the gather stride is about 2): fixed by the plan on the fast path,
  // where W == WC and N == NC or 2 NC (the same rule as the host's select_plan)
  static constexpr bool SPLIT_LEAN = (2 * WC >= 3 * NC) && (WC <= 3 * NC);
  // The three forms of the row top (arms of one ladder in the kernel).  FMAX: fast path with at most 32 samples per lane.
  // CMEAN: the fast-path rows that are too wide for it (C4, C1): the same mean.  Neither: the any-option kernel.
  static constexpr bool FMAX = LEAN && WCH <= 4;
  static constexpr bool CMEAN = LEAN;
  // Fast-path normalisations.  With the two-word division (PREC) the normalised sample p = (v - min) * scale is carried as two
  // floats as well -- rounding it is a rounding at the size of the DC level, random from sample to sample -- and formed
  // inside the division (NPREC: v stays the camera sample, nmn / nsc are the row's or the frame's).
  static constexpr bool NPREC = NORM != 0 && PREC;

  // The transposed store (geometry: fdoct_fused_tro.h).  TRO_INPLACE: four rows per wave, tiles owned by groups of GW waves.
  static constexpr bool TRO_INPLACE = TRO && RPW == 4;
  static constexpr unsigned GW = (unsigned)fused_tro_group_waves();   // waves of a group (TRO_INPLACE): a tile is 4 GW rows
  static constexpr unsigned TR = TRO_INPLACE ? 4u * GW : (unsigned)FUSED_TR_ROWS;  // rows of a tile
  // one write-out step: lane (dg, rq) takes rows 4 rq .. 4 rq + 3 and bins 4 dg .. 4 dg + 3 of the step's TRO_SB bins
  static constexpr int TRO_RQ = TR / 4, TRO_DGN = 64 / TRO_RQ, TRO_SB = 4 * TRO_DGN;
};

}  // namespace fdoct
