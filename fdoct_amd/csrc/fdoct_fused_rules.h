// fdoct_fused_rules.h -- the compile-time rules the fused kernels and the host share (one definition for kernel and host): block
// limits, which tables and planes a kernel stages in LDS, the form of the second reciprocal word, the transposed store's tiles
// and ring.  Plain C++ without HIP: the kernels see it through fdoct_kernels.h, the launch value through fdoct_launch.h.
#pragma once
#include <cstddef>

// Largest workgroup any fused kernel is compiled for (fdoct_capi.cpp checks a caller's geometry against it).
constexpr int FDOCT_MAX_BLOCK = 768;

namespace fdoct {

// Threads per workgroup the fused kernel is compiled for (register budget = 512 / (threads/256) VGPRs per
// lane).  Plans with 32 FFT points per lane hold twice the per-lane state (the 2048-point ones are LDS-limited to
// <= 8 waves per CU anyway),
// the general (predicated, every-option) kernel carries more live state than the fast-path one, and the
// fast-path row-swap plan (kind 1) keeps its row-invariant tables in registers: all of these trade
// occupancy for registers instead of spilling.
constexpr int fused_max_block(int nc, int T, bool lean, int kind) {
  return (nc / T >= 32 || !lean || kind == 1) ? 512 : FDOCT_MAX_BLOCK;  // nc/T = FFT points held per lane
}

// Fast-path kernels of the row-swap plans keep the per-column constants (1/background, window, slope weights) in
// registers; the host then leaves those three planes out of the workgroup's LDS (FusedArgs::lds_planes = 0), which is
// what lets the 2048-point plans run 7 instead of 5 waves per CU.  One definition for kernel and host.
constexpr bool fused_resident_consts(int kind, bool lean, bool avg, int wch, int stage) {
  return lean && (kind == 1 || (kind == 2 && !avg)) && wch <= 4 && stage != 2;
}

enum { FDOCT_K_U8 = 0, FDOCT_K_U16 = 1, FDOCT_K_F32 = 2 };

// The fast-path kernels exist in two instantiations: multiplying by one word of the reciprocal background or by both
// (fdoct_capi.cpp::reciprocal_words; fdoct_set_precise_division).  The any-option kernel always uses both.
// FDOCT_PREC_T2: how many of the 12 step-3 twiddles of the 1024-point plan stay in registers in the kernels that can
// multiply by both words (the rest come from LDS every row: the low words' 32 registers are in flight at the row top).
constexpr int FDOCT_PREC_T2 = 6;
// The form of the second word on the fast-path kernels with at most 32 samples per lane (fused_kernel's IL16; fused_il_half).
// The missing part of the quotient, v * il, is (v * ib) * (il / ib) = (c0 + d) * rho with rho = il / ib, |rho| <= 2^-24, and
// d * rho lies below the rounding of d itself: the correction is c0 * rho_i -- a row-dependent scalar times a column-dependent
// pattern that needs no more than ~10 bits.  The pattern is a plane of HALF floats (rho * 2^38: 2 W bytes of LDS, 16
// registers in flight instead of 32, every step-3 twiddle resident again) applied by v_fma_mix_f32, which converts its f16
// operand inside the fma.  (Round 4's form, il as floats multiplied by the samples, is what the kernels with wider rows keep.)
constexpr int FDOCT_PREC16_T2 = 10;      // step-3 twiddles resident in the half-float form (16 registers in flight at the row top): 516 M A-scans/s with 10 or 8, 513 with 12
constexpr int FDOCT_PREC16_T2_IB2D = 0;  // ... with a full-frame background (16 more registers hold the next row's pattern): 443 against 422 M A-scans/s with 4
constexpr int FDOCT_PREC16_T2_DMA = 8;   // ... with a full-frame background whose pattern row is prefetched into LDS (fused_il16_dma_bytes): 478 M A-scans/s against 438 with 12 (spills) and 442 with the pattern row in registers
// The averaging kernels with more than 32 samples per lane keep the half-float pattern in registers (fused_kernel, IL16R).  A
// full-frame background's pattern row is prefetched into LDS by global_load_lds_dwordx4 (no registers; fused_kernel, ILDMA):
// LDS bytes per computing wave of that prefetch slot (one definition for kernel and host)
constexpr size_t fused_il16_dma_bytes(bool ib2d, bool both_words_half, bool tro, int wc) { return (ib2d && both_words_half && !tro) ? (size_t)2 * wc : 0; }
constexpr int kPrec16Shift = 38;  // rho * 2^38: at most 2^14 in magnitude
constexpr bool fused_il_half(bool lean, int wch) { return lean && wch <= 4; }
// The averaging fast-path kernels with more than 32 samples per lane keep their planes in LDS and are bound by its capacity (a
// fourth plane would cost C4 a wave per CU): they read the low words from a global plane in the same order (FusedArgs::prec = 3).
// (round 6: so do ALL fast-path kernels of the 512-point plan -- C1, 16 lanes per row, four rows per wave -- averaging or not, row-major
// or transposed store: the 4 W bytes of the plane are a sixth computing wave next to the transposed store's ring, and both
// layouts apply the second word in the same form, so their images stay bit-identical)
constexpr bool fused_il_global(bool lean, bool avg, int wch, int T = 64) { return lean && (avg || T == 16) && wch > 4; }

// Rows per tile of the fused transposed store: a workgroup owns FUSED_TR_ROWS consecutive A-scans of one B-scan at a time, so
// the depth-major output is written in segments of FUSED_TR_ROWS * 4 bytes.
constexpr int FUSED_TR_ROWS = 16;
// Slots of the LDS ring of finished rows (FUSED_TR_ROWS < slots <= 2 FUSED_TR_ROWS): what 160 KB of LDS hold of 1024-bin
// rows next to seven computing waves' buffers.
constexpr int FUSED_TR_RING = 20;
// Who writes a complete tile out: every wave takes steps of it at its hand-over points, and all waves compute.  (Measured against
// the wave whose row completes the tile writing it out at once, and against a wave set aside for it: DESIGN.md 3.1a,
// profiles/r03_tro_final_probe.txt.)
// Ring slots for numdisplaypoints = d: up to 512 depth bins a second tile fits (rows of the next tile go in while a tile is
// written out: + 7 %), above that FUSED_TR_RING is what the LDS holds.  One definition for kernel and host.
constexpr unsigned fused_tro_ring_slots(int d) { return d <= 512 ? 2u * FUSED_TR_RING : (unsigned)FUSED_TR_RING; }
// LDS bytes of the ring (a slot is d + 4 floats).
constexpr size_t fused_tro_ring_bytes(int d) { return (size_t)fused_tro_ring_slots(d) * (size_t)(d + 4) * 4; }
// Round 5: the ring takes what the LDS has left.  The transposed store is bound by how much of the next tile fits into the
// ring while a tile drains, so its kernels keep out of LDS what they only read once -- the step-5 twiddle
// table (7.7 KB: those kernels hold its 15 entries per lane in registers) and, without averaging, the gather table (4 KB:
// the addresses are resident too) -- and the launch picks the LARGEST ring of this list that fits next to eight computing
// waves (23 slots at 1024 depth bins, 22 with the half-float plane of the second word; the moduli are compile-time constants
// of the kernel: FusedArgs::tr_ring selects one).  Any value above FUSED_TR_ROWS works for the hand-over protocol; at most
// 3 FUSED_TR_ROWS, so that no more than four tiles are open at once (tr_arrived / tr_done are indexed by tile mod 4).
constexpr unsigned kTroRingChoices[] = {20, 21, 22, 23, 24, 26, 28, 32, 40, 44, 48};
// (rpw: rows per wave of the plan -- a wave's rows take consecutive slots, so the ring is a whole number of them)
constexpr unsigned fused_tro_ring_pick(size_t lds_left, int d, int rpw = 1) {
  unsigned best = 0;
  for (unsigned c : kTroRingChoices)
    if ((c % (unsigned)rpw) == 0 && (size_t)c * (size_t)(d + 4) * 4 <= lds_left) best = c;
  return best;
}
// Which tables a fused kernel stages in LDS (one rule for kernel and host).  tw3: the step-5 table of the 1024-point row-swap plan.
// (ib2d_both_words: the variant with a full-frame background and both words re-reads its step-5 twiddles every row; keeping
// them in registers there spills)
constexpr bool fused_tw3_in_lds(int kind, bool lean, int stage, bool tro, bool ib2d_both_words) {
  return !(tro && lean && kind == 1 && stage != 1 && !ib2d_both_words);
}
constexpr bool fused_gi_in_lds(int kind, bool lean, int stage, bool cplx, bool avg, bool tro) {
  return !(tro && lean && stage != 2 && kind == 1 && !cplx && !avg);
}
constexpr unsigned FDOCT_TRO_SPIN_LIMIT = 1u << 21;  // x s_sleep(8) = 512 cycles each: about half a second
// Depth bins one iteration of the tile write-out covers (numdisplaypoints must be a multiple of it).
// Four rows per wave (the 512-point plan's in-place tiles): waves per group = rows per tile / 4.  Groups of EIGHT waves own tiles of
// 32 rows and write the D x H image in 128-byte segments -- whole cache lines, which the memory system takes at its row-major rate
// where 64-byte segments stop at 3.7 TB/s (profiles/r06_rw_mix.txt) -- at no cost in LDS (the rows lie in the waves' own buffers).
// Built and measured (round 6, profiles/r06_c1_group_ab.txt, bit-identical results): 790 against 855 M A-scans/s on C1 -- a workgroup
// that is ONE group meets twice per tile with all of its waves, and what they idle there outweighs the segments.  Four it stays.
constexpr int kTroGroupWaves = 4;
constexpr int fused_tro_group_waves() { return kTroGroupWaves; }
constexpr int fused_tro_tile_rows(int rpw) { return rpw == 4 ? 4 * kTroGroupWaves : FUSED_TR_ROWS; }
constexpr int fused_tro_step_bins(int rpw = 1) { return 4 * (64 / (fused_tro_tile_rows(rpw) / 4)); }
// Which plans have the fused transposed store compiled (the fast-path row-swap 1024-point plan, one row per wave).
// Round 6: also the 512-point Stockham plan (C1: 1024 samples -> numfftpoints 1024; 16 lanes per row, FOUR rows per wave) --
// without the ring: tiles are owned by groups of four waves and the finished rows wait in the waves' own row buffers
// (fused_kernel, TRO_INPLACE).
constexpr bool fused_tro_compiled(int kind, int T, int wch) { return (kind == 1 && T == 64 && wch <= 4) || (kind == 0 && T == 16 && wch == 8); }

}  // namespace fdoct
