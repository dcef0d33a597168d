// fdoct_kernels.hip -- CDNA4 (gfx950) kernels of the FD-OCT reconstruction path.
//
// One fused kernel replaces the reference's per-frame OpenCV block
// (BscanFFT.cpp:1123-1240 / BscanFFTsim.cpp:842-955): camera samples in,
// B-scan magnitudes (and dB) out, one HBM read and one HBM write per A-scan.
//
// Work decomposition (no workgroup barrier inside the row loop):
//   * a group of T lanes (T = 16/32/64, so 4/2/1 rows per 64-wide wave) owns one
//     output A-scan at a time and loops over rows (persistent waves);
//   * the row's W samples are loaded as 16-byte vectors, 8 samples per lane per
//     chunk, coalesced; normalise / background / DC removal / window /
//     the reference's slope step are done in registers (A2, A3, A5);
//   * the lambda->k gather goes through a per-row LDS staging buffer (A5);
//   * the IDFT keeps P = NC/T complex points per lane, runs radix-R butterflies in
//     registers and exchanges data between passes through a padded LDS buffer --
//     or, for the 1024-point plan, swaps 16-lane rows with v_permlane*_swap for one
//     of the two exchanges (A7);
//   * real input uses the N/2-point complex FFT + untangle; the partner bin
//     lives in lane (T - l) and is fetched with ds_bpermute (no LDS memory);
//   * magnitude, crop, averaging, epsilon, dB and the DC mask are the epilogue
//     (A8-A10); only D floats per A-scan are written.
//   * waves claim their rows from a workgroup ticket counter (the hardware favours the
//     oldest wave of a SIMD; a static split leaves SIMDs half empty at the end);
//   * the fast-path instantiation of the 1024-point plan keeps every row-invariant
//     table (constants, gather addresses, twiddles) in registers, 2 waves per SIMD.
// The chip is power-limited under this kernel and the SIMDs issue-bound, so all complex
// arithmetic is written on 2-element vectors that lower to v_pk_add/mul/fma_f32 (two
// flops per lane per instruction) and quarter turns ride on instruction modifiers.
// MFMA is not used: the path is elementwise + FFT work, not a dense contraction.
//
// This file is the translation unit: fused_kernel (workgroup set-up and the row loop) and the dispatch.  In headers:
//   fdoct_fused_traits.h    FusedTraits: every size and compile-time switch an instantiation derives from its parameters
//   fdoct_fused_dev.h       shared device helpers: measurement switches, wave_lds_sync, RawChunk, group reductions, load_consts
//   fdoct_fused_fft.h       the LDS transforms: Stockham passes, the 1024- and 2048-point row-swap plans
//   fdoct_fused_tro.h       the transposed store's geometry: tiles, ring slots, one write-out step, ticket -> row
//   fdoct_fused_row.h       row slots and tickets, the real-path untangle, issue_ib2d, load_plane, second_word
//   fdoct_prepass_kernels.inc, fdoct_prepass_launch.inc   the small pre-pass kernels (min / max, transpose, f64 split) and their launchers
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fdoct_fft_reg.h"
#include "fdoct_kernels.h"

#ifdef FDOCT_DEV_ONE  // tuning builds: which single instantiation (see launch_typed)
#ifndef FDOCT_DEV_ONE_CPLX
#define FDOCT_DEV_ONE_CPLX false
#endif
#ifndef FDOCT_DEV_ONE_AVG
#define FDOCT_DEV_ONE_AVG 0
#endif
#endif

#include "fdoct_fused_traits.h"
#include "fdoct_fused_dev.h"
#include "fdoct_fused_fft.h"
#include "fdoct_fused_tro.h"
#include "fdoct_fused_row.h"

namespace fdoct {

// ------------------------------------------------------------ fused kernel --
// LOG2NC: log2 of the complex FFT length NC (= N/2 real path, N complex path)
// T: lanes per row (64/T rows per wave); R1*R2*R3 = NC (R3 = 1: two passes); KIND: 0 = Stockham
// passes through LDS, 1 = fft1024_rowswap; WCH: 8-sample chunks per lane (W <= WC = 8*T*WCH);
// CPLX: dispersion phase path.
// LEAN: the benchmark / common acquisition configuration, compiled without any
//   predication: W == WC, 1-row background, no pi/dark frame, no normalisation (any
//   number of averaged frames).  !LEAN handles everything else.
// STAGE: 0 = the whole chain in one launch (default).  1 = "resample stage" only: samples in, the
//   k-linear row (data_ylin packed as the FFT input, NC float2 per row) out to a.ylin.  2 = "FFT stage"
//   only: a.ylin in, magnitudes/dB out.  Stages 1+2 reproduce stage 0 bit for bit at 3x the HBM traffic;
//   they exist so that each stage can be timed against the HBM roofline on its own (north star) and as
//   the seam for stages that need the intermediate in memory.
// The window table arrives pre-multiplied by 1/2 on the real path (host side): the untangle
// needs X = (A + w*O)/2 and a power-of-two scale of the window commutes exactly with every step.
// IB2D (fast path of the row-swap plan only): the background is a full H x W frame, as the reference's 'b' key
//   stores it.  The resident 1/background registers then double as a one-row-ahead prefetch buffer of the frame row
//   the next A-scan needs (a.ib2d: each 8-sample group stored evens first, then odds -- the RawChunk pair order).
// NORM (same kernels): 1 = whole-frame min-max normalisation (main:1128-1129; always on in BscanFFTsim.cpp:845) from the
//   per-frame (min,max) of the pre-pass, the scale of the next A-scan's frame being fetched at the prefetch point;
//   2 = row-wise min-max normalisation (normalizerows, main:88-97, 1126) with a wave-wide min/max of the row.
// TRO (fast path of the row-swap 1024-point plan, one row per wave): the outputs are written in the reference's own
//   layout, bscan[depth][row] (main:1220), by the chain itself, through a ring of finished rows in LDS.  A workgroup owns
//   TR = FUSED_TR_ROWS consecutive A-scans of one B-scan at a time (a "tile").  Its waves claim the tile's rows from the
//   ticket counter; a finished row goes into slot (ticket mod fused_tro_ring_slots(D): 20, or 40 up to 512 depth bins) of the ring (row-major, 4 B per lane:
//   conflict free) and is counted in an LDS counter of its tile.  A complete tile is written out in steps of 64 depth bins:
//   a step reads 16-byte pieces of 4 rows x 4 bins per lane -- a 4 x 4 block whose transposition is a renaming of
//   registers -- and stores, per depth bin, 16 bytes per lane = TR * 4 contiguous bytes of the B-scan.  When both bscan and
//   bscandb are asked for, the ring holds bscan and the step takes the logarithm (the same instruction on the same value as
//   the epilogue would).  The steps are claimed one at a time (compare-and-swap on an LDS counter) by whichever wave passes
//   a hand-over point: after putting a row into the ring, while waiting for a ring slot, and -- its rows done -- until the
//   workgroup's last tile is out.  No workgroup barrier, and nothing of it crosses HBM or L2: per A-scan
//   only the camera samples are read and the images written.  The ring is a quarter larger than a tile, so the waves run on
//   into the next tile while one is written out; a wave waits only when the slot it needs still holds a row of a tile that
//   has not been written out, and takes write-out steps itself while it waits.  Nobody waits in a cycle: a row is counted
//   as soon as it is in the ring, a wave waits for write-outs of EARLIER tiles only, a step is claimed only when its tile
//   is complete, and every waiting wave works on the steps it waits for.
//   (Round 3 first built this with the tiles in global memory, 128 KB per workgroup and buffer: they did not stay in the
//   4 MB of L2 an XCD's 32 workgroups share, and the chain ran at the rate of the two-pass path; profiles/r03_tro_probe*.)
template <int LOG2NC, int T, int R1, int R2, int R3, int KIND, int WCH, typename IN_T, bool CPLX, bool LEAN, int STAGE, bool AVG,
          bool IB2D = false, int NORM = 0, bool TRO = false, bool PRECT = false>
__global__ __launch_bounds__(fused_max_block(1 << LOG2NC, T, LEAN, KIND)) void fused_kernel(const FusedArgs a) {
  using X = FusedTraits<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, LEAN, STAGE, AVG, IB2D, NORM, TRO, PRECT>;
  __shared__ unsigned int row_ticket;  // next unclaimed row slot of this workgroup
  __shared__ unsigned int tr_arrived[4];  // TRO: rows of tile (q mod 4) in the ring
  // TRO: tiles q = i (mod 4) that have completed so far.  Tiles need not complete in order -- with a 4-row last tile of a
  // B-scan, or the 40-slot ring, no row of tile q + 1 waits for anything of tile q -- but tiles four apart do (a row of tile
  // q + 4 needs tile q + 1 written out, which the in-order counters below allow only after tile q), so these only grow and
  // "tile q is complete" is tr_done[q & 3] > q / 4.  tro_publish() turns them into the in-order counter everything else reads.
  __shared__ unsigned int tr_done[4];
  __shared__ unsigned int tr_ready, tr_wo_next, tr_wo_done;  // TRO, write-out by all waves: complete tiles; next step to claim; steps done (cumulative)
  // TRO with FOUR rows per wave (the 512-point plan, round 6): no ring.  A GROUP of four waves (GW, fdoct_fused_rules.h) owns a tile of 16 rows; a finished
  // row is deposited in the wave's OWN row buffer (free between the untangle and the next row's staging), the group meets, writes
  // the tile out together, meets again, and goes on -- all eight waves compute (the ring cost two of them their LDS).
  __shared__ unsigned int grp_tile[4][2];   // the tile a group's leader has claimed, by sequence parity
  __shared__ unsigned int grp_pub[4];       // tiles published to a group so far
  __shared__ unsigned int grp_arrived[4];   // waves of a group whose rows are deposited (cumulative: 4 per tile)
  __shared__ unsigned int grp_done[4];      // waves of a group that have finished their share of a write-out (cumulative)
  extern __shared__ __align__(16) unsigned char smem[];
  const int cw = a.lds_planes ? X::WC : 0;          // resident-constant kernels: the host leaves the planes out
  float* c_ib = reinterpret_cast<float*>(smem);  // [WC] 1/background
  float* c_win = c_ib + cw;                      // [WC] window
  float* c_g = c_win + cw;                       // [WC] fractionalk by sample index
  float* c_il = c_g + cw;                        // [WC] low word of 1/background (a.prec == 1: every kernel reads it from here, the resident-constant ones too)
  const int cwl = (a.prec == 1 && STAGE != 2) ? (X::IL16 ? X::WC / 2 : X::WC) : 0;  // floats (the FFT-stage kernel reads no samples); IL16: 2 WC bytes
  v2f* c_tw = reinterpret_cast<v2f*>(c_il + cwl);  // twiddle tables, a.tw_count entries
  const int tw_lds = X::TW3_LDS ? a.tw_count : (R2 - 1) * R1;   // entries staged: all, or the step-3 table only
  v2f* c_ph = c_tw + tw_lds;                     // [NC] phase (CPLX only)
  uint32_t* c_gi = reinterpret_cast<uint32_t*>(c_ph + (CPLX ? X::NC : 0));  // [NC] packed gather offsets
  unsigned char* scratch0 = reinterpret_cast<unsigned char*>(c_gi + (X::GI_LDS ? X::NC : 0));

#ifdef FDOCT_CLOCKPROBE
  const unsigned long long probe_c0 = __builtin_readcyclecounter(), probe_r0 = wall_clock64();
#endif
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = lane & (T - 1);
  const int sub = lane / T;

  // ---- stage the per-column constants once per workgroup
  // layout: sample i = 8*(lane + T*c) + e  ->  slot c*8T + (e&1)*4T + 4*lane + (e>>1), i.e. each
  // chunk is split into an even and an odd plane of 4 floats per lane (the RawChunk pair order), so a
  // wave's b128 reads are contiguous
  for (int i = tid; i < cw; i += blockDim.x) {
    const bool in = i < a.W;
    const int e = i & 7, ln = (i >> 3) & (T - 1), c = i / (8 * T);
    const int slot = c * 8 * T + (e & 1) * 4 * T + 4 * ln + (e >> 1);
    c_ib[slot] = (in && a.ib) ? a.ib[i] : 0.f;
    c_win[slot] = in ? a.win[i] : 0.f;
    c_g[slot] = in ? a.g[i] : 0.f;
  }
  if constexpr (X::IL16) {  // half-float pairs, already in the order the lanes read them (fdoct_capi.cpp)
    for (int i = tid; i < cwl; i += blockDim.x) reinterpret_cast<uint32_t*>(c_il)[i] = a.il16 ? a.il16[i] : 0u;
  } else {
    for (int i = tid; i < cwl; i += blockDim.x) {  // (the same slot rule)
      const int e = i & 7, ln = (i >> 3) & (T - 1), c = i / (8 * T);
      c_il[c * 8 * T + (e & 1) * 4 * T + 4 * ln + (e >> 1)] = (i < a.W && a.il) ? a.il[i] : 0.f;
    }
  }
  {
    const v2f* gtw = reinterpret_cast<const v2f*>(a.tw);
    for (int i = tid; i < tw_lds; i += blockDim.x) c_tw[i] = gtw[i];
    if constexpr (CPLX) {
      const v2f* gph = reinterpret_cast<const v2f*>(a.phase);
      for (int i = tid; i < X::NC; i += blockDim.x) c_ph[i] = gph[i];
    }
  }
  if (tid == 0) row_ticket = X::TRO_INPLACE ? (blockDim.x >> 6) / X::GW : (blockDim.x >> 6);  // slots 0 .. nwaves-1 are the (computing) waves' first rows (groups' first tiles)
  if (TRO && tid < 4) tr_arrived[tid] = tr_done[tid] = 0u;
  if (X::TRO_INPLACE && tid < 4) grp_pub[tid] = grp_arrived[tid] = grp_done[tid] = 0u;
  if (TRO && tid == 0) tr_ready = tr_wo_next = tr_wo_done = 0u;
  // gather table: entry n = ln + T*m is stored at [(m/4)][ln][m%4] so a lane's P entries are P/4
  // b128 reads with a 16-byte lane stride (re-read every row: cheaper than P resident VGPRs)
  if constexpr (X::GI_LDS) {
    for (int i = tid; i < X::NC; i += blockDim.x) {
      const int ln = i & (T - 1), m = i / T;
      c_gi[(m >> 2) * 4 * T + 4 * ln + (m & 3)] = a.gidx[i];
    }
  }
  __syncthreads();

  const unsigned RS = (unsigned)__builtin_amdgcn_readfirstlane((int)a.tr_ring);
  float* const tro_ring = reinterpret_cast<float*>(scratch0 + (size_t)(blockDim.x >> 6) * X::RPW * a.scratch_bytes);
  const int tro_slot = a.D + 4;
  const TroGeom<X> tro{a, RS, tro_ring, tro_slot, scratch0, lane};
  // Tile tq of this workgroup has just completed (all its rows are in the ring).
  // Tiles need not complete in order (see tr_done), but everything that waits or claims counts tiles IN ORDER: the tile is
  // counted in tr_done, then the in-order counter *inorder is advanced over every tile that is complete by now -- by this
  // wave or by whichever wave's compare-and-swap wins; a wave that completes tile q + 1 before tile q leaves the counter
  // alone and the wave that completes tile q later takes it past both.  (No lost hand-over: a wave reads the counters AFTER
  // its own tile is counted, and LDS operations execute one at a time, a wave's own in program order.)  Returns the counter
  // as last read.  Three LDS round trips per tile, i.e. per FUSED_TR_ROWS rows.
  auto tro_publish = [&](unsigned tq, unsigned int* inorder) -> unsigned {
    if (lane == 0) {
      // (next user of the row counter: tile tq + 4, whose rows wait for tile tq + 1 to be written out -- after this)
      __hip_atomic_store(&tr_arrived[tq & 3u], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(&tr_done[tq & 3u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    unsigned r;
    for (;;) {
      const unsigned r_l = __hip_atomic_load(inorder, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const unsigned d_l = __hip_atomic_load(&tr_done[lane & 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      r = (unsigned)__builtin_amdgcn_readfirstlane((int)r_l);
      const unsigned dc = (unsigned)__builtin_amdgcn_readlane((int)d_l, (int)(r & 3u));
      if (dc <= (r >> 2)) break;  // tile r is not complete yet: whoever completes it goes on from here
      if (lane == 0) {
        unsigned expect = r;
        (void)__hip_atomic_compare_exchange_strong(inorder, &expect, r + 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    return r;
  };
  // Distributed write-out: no wave is set aside.  The wave whose row completes a tile publishes it (tr_ready counts the
  // complete tiles IN ORDER, tro_publish: tile q's steps exist once tiles 0 .. q are all complete); its SPT = D / SB steps are
  // then claimed one at a time (compare-and-swap on tr_wo_next, so a step is never claimed before it exists) by whichever
  // wave passes a hand-over point: after putting a row into the ring, while waiting for a ring slot, and -- all rows
  // done -- until the workgroup's last tile is out.  The wave that finishes a tile's last step releases its slots.
  // (LDS round trips are what this costs -- a returning LDS operation takes 100-200 cycles next to the chain's own LDS
  // traffic -- so they are batched: tr_wo_next and tr_ready are read together, the steps-done counter is cumulative and bumped
  // without a return value (tile q is out when it reaches (q + 1) SPT), and only the claim itself is a round trip of its own.)
  auto tro_try_step = [&](unsigned s, unsigned ready) -> bool {  // s = tr_wo_next as just read, ready = complete tiles
    const unsigned spt = (unsigned)a.D / (unsigned)X::TRO_SB;
    if (s >= ready * spt) return false;
    unsigned got = 0u;
    if (lane == 0) {
      unsigned expect = s;
      got = __hip_atomic_compare_exchange_strong(&tr_wo_next, &expect, s + 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) ? 1u : 0u;
    }
    if (!__builtin_amdgcn_readfirstlane((int)got)) return true;  // another wave took it: something is going on
    const unsigned tq = s / spt, k = s - tq * spt;
    unsigned g, r0, nrows;
    (void)tro.tile(tq, g, r0, nrows);
    asm volatile("" ::: "memory");
    tro.step(tq, g, r0, nrows, (int)k * X::TRO_SB);
    asm volatile("" ::: "memory");  // the step's LDS reads have returned (they fed stores that have been issued)
    if (lane == 0) __hip_atomic_fetch_add(&tr_wo_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return true;
  };
  auto tro_writeout = [&](int max_steps) -> bool {  // true: a step was there (taken by this wave or another)
    bool did = false;
    for (int it = 0; it < max_steps; it++) {
      const unsigned s_l = __hip_atomic_load(&tr_wo_next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const unsigned r_l = __hip_atomic_load(&tr_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (!tro_try_step((unsigned)__builtin_amdgcn_readfirstlane((int)s_l), (unsigned)__builtin_amdgcn_readfirstlane((int)r_l))) break;
      did = true;
    }
    return did;
  };
  unsigned tro_done_seen = 0u;  // steps written out, as last read (the counter only grows: a valid lower bound)

  unsigned char* scr = scratch0 + (size_t)(wave * X::RPW + sub) * a.scratch_bytes;
  float* stg = reinterpret_cast<float*>(scr);
  v2f* xch = reinterpret_cast<v2f*>(scr);

  // ---- per-lane constants kept in registers for every row
  v2f utw = mk(1.f, 0.f);
  if constexpr (!CPLX) utw = reinterpret_cast<const v2f*>(a.utw)[l];  // exp(+2*pi*i*l/N)

  const v2f* tw_p2 = c_tw;                                       // pass 2 table: (R2-1) x R1
  // pass 3 table: (R3-1) x (R1*R2) (row-swap plans: the step-5 table); kernels that hold its entries in registers and need
  // the LDS for something else (TW3_LDS false) read them once from the global table
  const v2f* tw_p3 = X::TW3_LDS ? c_tw + (R2 - 1) * R1 : reinterpret_cast<const v2f*>(a.tw) + (R2 - 1) * R1;

  uint32_t gaddr[X::GRES ? 2 * X::P : 1];
  if constexpr (X::GRES) {  // 2 LDS byte addresses per FFT point
    const uint4* gl4 = reinterpret_cast<const uint4*>(c_gi) + l;
    const uint32_t sbase = (uint32_t)(uintptr_t)scr;  // LDS byte address of this wave's staging buffer
#pragma unroll
    for (int q = 0; q < X::P / 4; q++) {
      uint4 g4;
      if constexpr (X::GI_LDS)
        g4 = gl4[q * T];
      else   // (straight from the global table: entry n = l + T m)
        g4 = make_uint4(a.gidx[l + T * (4 * q)], a.gidx[l + T * (4 * q + 1)], a.gidx[l + T * (4 * q + 2)], a.gidx[l + T * (4 * q + 3)]);
      const uint32_t g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        gaddr[2 * (4 * q + j)] = sbase + (g[j] & 0xffffu);
        gaddr[2 * (4 * q + j) + 1] = sbase + (g[j] >> 16);
      }
    }
  }

  v2f r_t2[X::RES2 ? X::RES2 : 1], r_t3[X::RES3 ? 15 : 1];
  if constexpr (X::RES2 > 0 || X::RES3) {
    v2f t2tmp[12], t3tmp[15];
    fft1024_rowswap_twiddles(lane, tw_p2, tw_p3, t2tmp, t3tmp);
    if constexpr (X::RES2 > 0) {
#pragma unroll
      for (int i = 0; i < X::RES2; i++) r_t2[i] = t2tmp[i];
    }
    if constexpr (X::RES3) {
#pragma unroll
      for (int i = 0; i < 15; i++) r_t3[i] = t3tmp[i];
    }
  }
  // NORM: scale/shift of input frame (o / H) * A + ai (host guarantees rows < 2^31)
  float nsc = 1.f, nsh = 0.f, nmn = 0.f;
  auto frame_scale = [&](long long o, int ai) {
    if constexpr (NORM == 1) {
      const unsigned fr = (o < a.total_out_rows) ? (unsigned)o / (unsigned)a.H : 0u;
      const float2 mmx = a.minmax[(size_t)fr * (AVG ? a.A : 1) + ai];
      nsc = (mmx.y - mmx.x > 2.220446049250313e-16f) ? 1.f / (mmx.y - mmx.x) : 0.f;
      nsh = -mmx.x * nsc;
      nmn = mmx.x;
    }
  };
  v2f r_ib[X::RES ? X::NPR : 1], r_win[X::RES ? X::NPR : 1], r_g[X::RES ? X::NPR : 1];
  uint4 r_il16[(IB2D && X::IL16 && !X::ILDMA) ? WCH : 1];
  // (the slots lie behind the waves' row buffers: 2 WC bytes each)
  unsigned char* const il_dma = scratch0 + (size_t)(blockDim.x >> 6) * X::RPW * a.scratch_bytes + (size_t)wave * (2 * X::WC);
  uint4 r_il16r[X::IL16R ? WCH : 1];
  if constexpr (X::IL16R) {
    const uint4* h4 = reinterpret_cast<const uint4*>(a.il16) + l;
#pragma unroll
    for (int c = 0; c < WCH; c++) r_il16r[c] = h4[T * c];
  }
  if constexpr (X::RES) {
    // straight from the global tables (W == WC here), 32 bytes per lane and chunk, into the pair order
#pragma unroll
    for (int c = 0; c < WCH; c++) {
      if constexpr (!IB2D) load_plane<T>(a.ib, c, r_ib + 4 * c, l);
      load_plane<T>(a.win, c, r_win + 4 * c, l);
      load_plane<T>(a.g, c, r_g + 4 * c, l);
    }
  }

  const long long total = a.total_out_rows;
  // The row ticket (row slots: fdoct_fused_row.h).  TRIM kernels: the add is written out as the instruction, with its wait.  As an atomic builtin inside `if (lane == 0)` the
  // compiler's atomic optimiser elects a lane a second time (v_mbcnt twice, a compare, a count of exec, a second exec mask and
  // branch, a v_readfirstlane and an add of the lane's rank) for a wave that has one lane left.  The other kernels keep the
  // builtin, where the compiler is free to place the wait (see TRIM).
  auto claim = [&]() -> unsigned {
    unsigned t = 0;
    if constexpr (!X::TRIM) {
      if (lane == 0) t = __hip_atomic_fetch_add(&row_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (lane == 0) {
      const unsigned at = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned*)&row_ticket;
      asm volatile("ds_add_rtn_u32 %0, %1, %2\n\t"
                   "s_waitcnt lgkmcnt(0)"
                   : "=&v"(t) : "v"(at), "v"(1u) : "memory");
    }
    return t;
  };
  // (An asm ds_add_rtn_u32 whose result stays in flight until it is needed would save the LDS round trip the compiler
  // waits out here at every row top -- about 0.5 % -- but nothing stops the register allocator from copying the
  // not-yet-written result register in the instantiations that are short of registers; tried and withdrawn.)
  // ---- four rows per wave: tiles are owned by GROUPS of four waves (see grp_* above).  Wave m of a group takes rows 4 m .. 4 m + 3
  // of the group's tile; in a short last tile of a B-scan (4, 8 or 12 rows) the waves without rows recompute rows of the tile and
  // deposit nothing, so that every wave of a group walks through the same two meetings per tile.
  const unsigned grp = (unsigned)wave / X::GW, mem = (unsigned)wave % X::GW;
  unsigned grp_seq = 0u;   // tiles this group has finished
  auto grp_rows = [&](unsigned tq, TroRow& tr) -> long long {
    tr.t = 0u;
    tr.tq = tq;
    if (!tro.tile(tq, tr.g, tr.r0, tr.nrows)) return a.total_out_rows;
    const unsigned rt = 4u * mem;
    tr.dummy = rt >= tr.nrows;
    tr.rt = tr.dummy ? rt % tr.nrows : rt;
    return (long long)tr.g * a.H + (tr.r0 + tr.rt);
  };
  // the tile after the current one: the leader has claimed it at the row top and publishes it, the others wait for it (it was
  // claimed most of a row ago; the bound is the exit condition a spinning wave must have all the same)
  auto grp_next_tile = [&](unsigned leader_ticket) -> unsigned {
    const unsigned seq = grp_seq + 1u;
    unsigned tq;
    if (mem == 0u) {
      tq = ticket_value(leader_ticket);
      if (lane == 0) {
        __hip_atomic_store(&grp_tile[grp][seq & 1u], tq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_store(&grp_pub[grp], seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // (LDS operations of a wave execute in order)
      }
    } else {
      for (unsigned spin = 0;; spin++) {
        const unsigned pub = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&grp_pub[grp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (pub >= seq) break;
        if (spin >= FDOCT_TRO_SPIN_LIMIT) {
          if (lane == 0) __hip_atomic_store(a.tr_fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      tq = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&grp_tile[grp][seq & 1u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    }
    return tq;
  };
  auto grp_meet = [&](unsigned int* counter, unsigned target) {   // every wave of the group adds one; all wait for the group's total
    if (lane == 0) __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    for (unsigned spin = 0;; spin++) {
      const unsigned have = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      if (have >= target) break;
      if (spin >= FDOCT_TRO_SPIN_LIMIT) {
        if (lane == 0) __hip_atomic_store(a.tr_fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  };
  TroRow tro_cur{}, tro_next{};
  long long o_wave;  // wave-uniform
  if constexpr (X::TRO_INPLACE)
    o_wave = grp_rows(grp, tro_cur);   // the groups' first tiles are their indices (row_ticket starts behind them)
  else if constexpr (TRO)
    o_wave = tro.take((unsigned)wave, tro_cur, claim);
  else
    o_wave = slot_row<X>((unsigned)wave);
  unsigned ticket = X::EARLY ? claim_row<X>(claim, mem) : 0u;

  const int W = LEAN ? X::WC : a.W;
  const bool split = LEAN ? X::SPLIT_LEAN : (a.split != 0);
  const int A = AVG ? a.A : 1;  // AVG == false: compiled for one frame per output (no frame arithmetic at all)
  const unsigned char* frames = static_cast<const unsigned char*>(a.frames);
  const int i0l = 8 * l;  // this lane's sample offset inside a chunk
  const int c0l = 4 * l;  // this lane's slot inside a constant plane (see the staging loop above)

  RawChunk<IN_T> raw[WCH];
  auto issue_loads = [&](long long o, int avg_i) {
    const bool valid = o < total;
    long long in_row = valid ? o : 0;
    if constexpr (AVG) {
      if (A > 1 && valid) {  // averaging: output row o = (group g, row r) reads frames g*A .. g*A+A-1
        const long long g = o / a.H;
        in_row = (g * A + avg_i) * (long long)a.H + (o - g * a.H);
      }
    }
    const void* row = frames + uni64<X>(in_row) * a.pitch_bytes;
#pragma unroll
    for (int c = 0; c < WCH; c++) {
      const int i0 = i0l + 8 * T * c;
      if ((LEAN || i0 < W) && !FDOCT_ABL(256))
        raw[c].load(row, i0);
      else
        raw[c].zero();
    }
  };

  // The prefetched row is "pinned" (an empty asm that names its registers) right after the
  // magnitude step and BEFORE the row's stores: the s_waitcnt the compiler needs there is
  // vmcnt(0) with the loads as the youngest VMEM operations, and the stores that follow get a
  // whole row of work to drain.  A wait at the loop top would also wait for those stores.
  // STAGE 2 streams the packed k-linear rows instead of camera samples
  v2f znext[STAGE == 2 ? X::P : 1];
  auto issue_zloads = [&](long long o, int avg_i) {
    if constexpr (STAGE == 2) {
      const bool valid = o < total;
      long long in_row = valid ? o : 0;
      if constexpr (AVG) {
        if (A > 1 && valid) {  // averaging: the resample stage left one k-linear row per INPUT A-scan (frame g*A + avg_i)
          const long long g = o / a.H;
          in_row = (g * A + avg_i) * (long long)a.H + (o - g * a.H);
        }
      }
      const v2f* zr = reinterpret_cast<const v2f*>(a.ylin) + uni64<X>(in_row) * X::NC + l;
#pragma unroll
      for (int m = 0; m < X::P; m++) znext[m] = valid ? __builtin_nontemporal_load(zr + T * m) : mk(0.f, 0.f);
    }
  };
  v2f ilx[(X::ILX && !X::IL16) ? X::NPR : 1];
  uint4 ilh[X::IL16 ? WCH : 1];  // IL16: chunk c's four half-float pairs (pair q = dword q), 16 registers instead of 32
  if (o_wave < total) {
    // (the first row like every later one: the full-frame background's rows -- and the global -> LDS load of its half-float
    // pattern -- are issued BEFORE the samples, so that a wait for the samples covers them: loads return in order)
    issue_ib2d<X>(a, o_wave + sub, r_ib, r_il16, il_dma, l);
    if constexpr (STAGE == 2)
      issue_zloads(o_wave + sub, 0);
    else
      issue_loads(o_wave + sub, 0);
    frame_scale(o_wave + sub, 0);
  }


  FusedProbe pr;
#ifdef FDOCT_FUSED_PROBE
  pr.start();
#endif
  while (o_wave < total) {
    o_wave = uni64<X>(o_wave);
    const long long o = o_wave + sub;
    const bool valid = o < total;
    long long o_next = total;
    if constexpr (X::EARLY) {
      o_next = slot_row<X>(ticket_value(ticket));  // claimed one row ago
      ticket = claim_row<X>(claim, mem);
    } else {
      ticket = claim_row<X>(claim, mem);  // back long before the prefetch below needs it
    }
    long long gi = 0;  // output group (frame when A == 1) and row inside the frame
    int r = 0;
    if constexpr (!LEAN) {
      if (a.need_rc && valid) {
        gi = o / a.H;
        r = (int)(o - gi * a.H);
      }
    }

    float acc[X::P];
#pragma unroll
    for (int m = 0; m < X::P; m++) acc[m] = 0.f;

    for (int ai = 0; ai < A; ai++) {
      v2f z[X::P];
      if constexpr (STAGE == 2) {
#pragma unroll
        for (int m = 0; m < X::P; m++) z[m] = znext[m];
        if (ai + 1 < A)
          issue_zloads(o, ai + 1);
        else
          issue_zloads(o_next + sub, 0);
      } else {
      // ---------------- A2: dark, normalise, pi frame, background
      // (fast path, low words of the reciprocal background in LDS: their reads are issued here, ahead of everything the row
      // does with them -- the samples are still packed, so this is where registers are to spare)
      if constexpr (X::IL16) {
        if constexpr (X::ILDMA) {
          // The slot was filled by global_load_lds a row ago.  Explicit wait, not the compiler's own tracking of
          // LDS writes by that instruction: the samples in `raw` were issued AFTER the DMA and loads return in order, so an
          // empty asm that consumes a sample register makes the compiler wait for it here, and its memory clobber keeps the
          // LDS reads below it.  (For every row but the first that wait already happened at the pin() in front of the
          // previous row's stores: no cost.)
          raw[0].pin_ordered();
          const uint4* h4 = reinterpret_cast<const uint4*>(il_dma) + l;
#pragma unroll
          for (int c = 0; c < WCH; c++) ilh[c] = h4[T * c];
        } else if constexpr (IB2D) {
#pragma unroll
          for (int c = 0; c < WCH; c++) ilh[c] = r_il16[c];
        } else {
          const uint4* h4 = reinterpret_cast<const uint4*>(c_il) + l;
#pragma unroll
          for (int c = 0; c < WCH; c++) ilh[c] = h4[T * c];
        }
      } else if constexpr (X::ILX) {
#pragma unroll
        for (int c = 0; c < WCH; c++) load_consts<T>(c_il + c0l, c, ilx + 4 * c);
      }
      v2f v[X::NPR];  // sample pairs: v[4c+q] = samples 8*(l+T*c) + chunk_pair_offset(q), +2
#pragma unroll
      for (int c = 0; c < WCH; c++) raw[c].unpack(v + 4 * c);
      // Fast-path normalisations (NPREC: formed inside the division below; v stays the camera sample here)
      if constexpr (NORM == 1 && !X::NPREC) {  // main:1128-1129, same expression as the general kernel below
#pragma unroll
        for (int i = 0; i < X::NPR; i++) v[i] = pk_fma(v[i], mk(nsc, nsc), mk(nsh, nsh));
      }
      if constexpr (NORM == 2) {  // main:88-97, 1126: the general kernel's row-wise normalisation, W == WC here
        float mn = INFINITY, mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < X::NPR; i++) {
          pair_minmax(v[i], mn, mx);
        }
        mn = group_min<T>(mn);
        mx = group_max<T>(mx);
        const float sc = (mx - mn > 2.220446049250313e-16f) ? 1.f / (mx - mn) : 0.f;
        if constexpr (X::NPREC) {
          nmn = mn;
          nsc = sc;
        } else {
          const float sh = -mn * sc;
#pragma unroll
          for (int i = 0; i < X::NPR; i++) v[i] = pk_fma(v[i], mk(sc, sc), mk(sh, sh));
        }
      }

      bool gnorm = false;  // any-option kernel: a normalisation is on (nmn, nsc hold its minimum and scale)
      if constexpr (!LEAN) {
        const long long in_frame = gi * A + ai;
        if (a.yd) {
          const float* ydr = a.yd + (a.yd_2d ? (size_t)r * W : 0);
#pragma unroll
          for (int c = 0; c < WCH; c++) {
            const int i0 = i0l + 8 * T * c;
            if (i0 < W) {
#pragma unroll
              for (int p = 0; p < 4; p++) v[4 * c + p] -= mk(ydr[i0 + chunk_pair_offset(p)], ydr[i0 + chunk_pair_offset(p) + 2]);
            }
          }
        }
        if (a.rowwisenormalize) {  // main:88-97,1126
          float mn = INFINITY, mx = -INFINITY;
#pragma unroll
          for (int c = 0; c < WCH; c++) {
            if (i0l + 8 * T * c < W) {
#pragma unroll
              for (int p = 0; p < 4; p++) {
                pair_minmax(v[4 * c + p], mn, mx);
              }
            }
          }
          mn = group_min<T>(mn);
          mx = group_max<T>(mx);
          // (the normalised sample (v - min) * scale is formed inside the division below, as two floats: see there)
          gnorm = true;
          nmn = mn;
          nsc = (mx - mn > 2.220446049250313e-16f) ? 1.f / (mx - mn) : 0.f;
        } else if (a.minmax) {  // main:1128-1129 whole-frame min-max, from the pre-pass
          const float2 mmx = a.minmax[in_frame];
          gnorm = true;
          nmn = mmx.x;
          nsc = (mmx.y - mmx.x > 2.220446049250313e-16f) ? 1.f / (mmx.y - mmx.x) : 0.f;
        }
      }
      // main:1132 ... / data_yb as a multiply by the host-side reciprocal; main:1138 row mean; main:1142 window; and the
      // slope step of main:1153-1173.  With x = v / yb, t = x - mean and y = t * w, the reference's
      //   s_i = y_i + g_i * (y_i - y_(i-1))        (g_i = fractionalk by SAMPLE index, see A5 below)
      // is  s_i = a_i * t_i + b_i * t_(i-1),       a_i = (1 + g_i) w_i,  b_i = -g_i w_(i-1)
      // so the host folds window and slope weights into the two per-sample planes a (a.win) and b (a.g): two packed
      // instructions per sample pair instead of four.  Sample 0 has slopes[0] = slopes[1] (main:1161):
      // a_0 = (1 - g_0) w_0, b_0 = +g_0 w_1, and t_1 stands in for t_(-1).
      float mh = 0.f, ml = 0.f;
      v2f av[X::NPR], bv[X::NPR];
      if (!FDOCT_ABL(1)) {
        v2f ibv[X::NPR];
        bool from_lds = true;
        if constexpr (!LEAN) {
          if (a.ib2d) {
            from_lds = false;
#pragma unroll
            for (int c = 0; c < WCH; c++) {
              const int i0 = i0l + 8 * T * c;
              if (i0 < W) {
                const float4* p4 = reinterpret_cast<const float4*>(a.ib2d + (size_t)r * X::WC + i0);  // rows are padded to WC
                const float4 q0 = p4[0], q1 = p4[1];
                evens_odds_pairs(q0, q1, ibv + 4 * c);  // a.ib2d holds each 8-sample group evens first, then odds
              } else {
#pragma unroll
                for (int p = 0; p < 4; p++) ibv[4 * c + p] = mk(0.f, 0.f);
              }
            }
          }
        }
        // fast path with at most 32 samples per lane: 1/background stays in registers through the sum and the
        // subtraction (resident, or read once from the LDS plane), so x is never formed -- the row sum is accumulated
        // by fma (four chains), t = fma(v, 1/yb, -mh) - ml rounds once, and the mean needs no f64
        if constexpr (X::FMAX) {
          if constexpr (X::RES) {
#pragma unroll
            for (int i = 0; i < X::NPR; i++) ibv[i] = r_ib[i];
          } else {
#pragma unroll
            for (int c = 0; c < WCH; c++) load_consts<T>(c_ib + c0l, c, ibv + 4 * c);
#pragma unroll
            for (int c = 0; c < WCH; c++) load_consts<T>(c_win + c0l, c, av + 4 * c);
          }
          // Row mean without any DC-sized sum: c0, the average of one x = v / yb per lane, is a wave-uniform estimate
          // of the mean; d = fma(v, 1/yb, -c0) is the exact product minus c0 rounded at the size of the DEVIATION from it
          // (fringes, residual envelope), so are the sums of d, and x - mean = d - mean(d).  Same operation count as summing
          // the products (whose lane sums of ~ 8 WCH x mean rounded at the size of the DC level and left 1e-8 of it in the mean:
          // 4e-6 of the DC level in depth bins 0 and 1, above the tolerance once the fringes are weaker than ~2 % of the DC level).
          // 1/yb is the two-float sum ib + il (fdoct_capi.cpp::reciprocal_words).  The f32 reciprocal alone is off by up to
          // 6e-8 of the quotient: a fixed per-column pattern of the size of the DC level, <= 4e-6 of it per depth bin -- above the
          // tolerance for fringes weaker than 1 % of the DC level.  PREC (the two-word instantiations, fdoct_set_precise_division):
          // a second fma adds v * il, rounded at the size of the deviation like the first; the low words come from the
          // workgroup's LDS plane (there is no register left to keep them resident), read at the row top (ilx).
          // (the 64 samples 8 l of the first chunk.  The middle chunk was tried in round 6 -- it is what the any-option kernel below
          // takes its single-chunk estimate from -- and left C2's flat 1e-3 dB pass rate at 0.9999 instead of 1: kept as it was.)
          const float c0 = group_sum_f32<T, X::TRIM>((X::NPREC ? (v[0].x - nmn) * nsc : v[0].x) * ibv[0].x) * (1.f / (float)T);
          // IL16: what the first word leaves out, v * il = (v * ib) * rho = (c0 + d) * rho with rho = il / ib (|rho| <= 2^-24), is
          // c0 * rho up to d * rho -- below the rounding of d.  rho * 2^38 comes as half floats (ten bits of a correction that is
          // 8 x the tolerance at fringes of 1e-3 of the DC level), v_fma_mix_f32 converts them inside the fma.
          const float c0s = c0 * kTwoPowMinus38;
          if constexpr (X::NPREC) {
            // p = (v - min) * scale as two floats (v - min is exact on the camera's integer samples; p_lo = the product's exact
            // residual), times ib + il: nothing of normalise-and-divide rounds at the size of the DC level
#pragma unroll
            for (int i = 0; i < X::NPR; i++) {
              const v2f vm = v[i] - mk(nmn, nmn);
              const v2f ph = vm * mk(nsc, nsc);
              const v2f pl = pk_fma(vm, mk(nsc, nsc), -ph);
              if constexpr (X::IL16)
                v[i] = pk_fma(pl, ibv[i], second_word<X>(ilh, c0s, pk_fma(ph, ibv[i], mk(-c0, -c0)), i));
              else
                v[i] = pk_fma(pl, ibv[i], pk_fma(ph, ilx[i], pk_fma(ph, ibv[i], mk(-c0, -c0))));
            }
          } else if constexpr (X::IL16) {
#pragma unroll
            for (int i = 0; i < X::NPR; i++) v[i] = second_word<X>(ilh, c0s, pk_fma(v[i], ibv[i], mk(-c0, -c0)), i);
          } else if constexpr (X::PREC) {
#pragma unroll
            for (int i = 0; i < X::NPR; i++) v[i] = pk_fma(v[i], ilx[i], pk_fma(v[i], ibv[i], mk(-c0, -c0)));
          } else {
#pragma unroll
            for (int i = 0; i < X::NPR; i++) v[i] = pk_fma(v[i], ibv[i], mk(-c0, -c0));
          }
          v2f s4[4] = {v[0], v[1], v[2], v[3]};
#pragma unroll
          for (int c = 1; c < WCH; c++) {
#pragma unroll
            for (int p = 0; p < 4; p++) s4[p] += v[4 * c + p];
          }
          const v2f part = (s4[0] + s4[1]) + (s4[2] + s4[3]);
          mh = group_sum_f32<T, X::TRIM>(part.x + part.y) * (1.f / (float)X::WC);  // mean of d (W == WC on this path)
          if constexpr (X::RES) {
#pragma unroll
            for (int i = 0; i < X::NPR; i++) {
              av[i] = r_win[i];
              bv[i] = r_g[i];
            }
          } else {
#pragma unroll
            for (int c = 0; c < WCH; c++) load_consts<T>(c_g + c0l, c, bv + 4 * c);
          }
#pragma unroll
          for (int i = 0; i < X::NPR; i++) v[i] -= mk(mh, mh);
        } else {
          // WCH <= 4: all reciprocal-background reads are issued up front (one LDS wait); wider rows read
          // them chunk by chunk to stay inside the register budget
          if (from_lds && WCH <= 4) {
#pragma unroll
            for (int c = 0; c < WCH; c++) load_consts<T>(c_ib + c0l, c, ibv + 4 * c);
          }
          double sum = 0.0;
          float c0 = 0.f;
          [[maybe_unused]] bool have_c0 = false;
          v2f s4[4] = {mk(0.f, 0.f), mk(0.f, 0.f), mk(0.f, 0.f), mk(0.f, 0.f)};
#pragma unroll
          for (int cc = 0; cc < WCH; cc++) {
            // (any-option kernel: the chunks from the MIDDLE of the row on -- c0 comes from the first chunk taken, see below)
            const int c = X::CMEAN ? cc : (cc + WCH / 2) % WCH;
            if (from_lds && WCH > 4) load_consts<T>(c_ib + c0l, c, ibv + 4 * c);
            // low words of 1/background (see the block above): from the LDS plane, or -- full-frame background -- from the
            // frame's own row in global memory
            // (where the low words come from is a COMPILE-TIME property of the fast-path kernels -- fused_il_global, one rule for
            // kernel and host: a run-time branch on a.prec here made the compiler zero and merge the eight registers of every
            // chunk, 130 v_mov per input A-scan of C4 -- round 5)
            v2f ilv[4] = {mk(0.f, 0.f), mk(0.f, 0.f), mk(0.f, 0.f), mk(0.f, 0.f)};
            if constexpr (X::IL16R) {
              // (resident half-float pattern: applied below as c0 * rho)
            } else if constexpr (LEAN && X::PREC && fused_il_global(LEAN, AVG, WCH, T)) {
              // (averaging fast-path kernels that are short of LDS: the same plane, in the same order, from global memory -- L1 / L2
              // hits; the wave's stores, which such a load would have to wait behind, come once per A input rows there)
              load_consts<T>(a.ilp + c0l, c, ilv);
            } else if constexpr (LEAN && X::PREC) {
              load_consts<T>(c_il + c0l, c, ilv);
            } else if (!LEAN && a.prec == 1) {
              load_consts<T>(c_il + c0l, c, ilv);
            } else if constexpr (!LEAN) {
              if (a.prec == 2 && i0l + 8 * T * c < W) {
                const float4* p4 = reinterpret_cast<const float4*>(a.il2d + (size_t)r * X::WC + i0l + 8 * T * c);
                const float4 q0 = p4[0], q1 = p4[1];
                evens_odds_pairs(q0, q1, ilv);
              }
            }
            if constexpr (X::CMEAN) {
              if (c == 0) c0 = group_sum_f32<T, X::TRIM>(v[0].x * ibv[0].x) * (1.f / (float)T);
              if constexpr (X::IL16R) {   // what the first word leaves out is c0 * rho up to d * rho (see the fast path above)
                const float c0s = c0 * kTwoPowMinus38;
                const uint32_t hq[4] = {r_il16r[c].x, r_il16r[c].y, r_il16r[c].z, r_il16r[c].w};
#pragma unroll
                for (int p = 0; p < 4; p++) {
                  const v2f d = pk_fma(v[4 * c + p], ibv[4 * c + p], mk(-c0, -c0));
                  v[4 * c + p] = mk(fma_mix_lo(c0s, hq[p], d.x), fma_mix_hi(c0s, hq[p], d.y));
                }
              } else if constexpr (X::PREC) {
#pragma unroll
                for (int p = 0; p < 4; p++) v[4 * c + p] = pk_fma(v[4 * c + p], ilv[p], pk_fma(v[4 * c + p], ibv[4 * c + p], mk(-c0, -c0)));
              } else {
#pragma unroll
                for (int p = 0; p < 4; p++) v[4 * c + p] = pk_fma(v[4 * c + p], ibv[4 * c + p], mk(-c0, -c0));
              }
#pragma unroll
              for (int p = 0; p < 4; p++) s4[p] += v[4 * c + p];
            } else {
              // (any-option kernel: the same deviation form with the f64 sum kept; chunks past the end of a narrow row stay zero.
              // c0 = the average of v / yb over the group's samples of the first chunk taken that has any -- the middle of a full
              // row.  Any c0 is correct; a POOR one costs precision: d = v / yb - c0 is rounded at its own size, and the row's first
              // sample -- round 5's c0 -- sits in the tail of the source spectrum, where a few hundred counts make v / yb noisy
              // at 1e-3: 0.6 x the tolerance on rows whose fringes a moving average had all but cancelled, round 6's sweeps.)
              const bool in_row = LEAN || (i0l + 8 * T * c < W);
              // a normalisation: p = (v - min) * scale as two floats (rounded product and its exact residual), so that the
              // normalised sample is not rounded at the size of the DC level; then the pi frame (main:1132: data_y - data_yp)
              v2f plo[4] = {mk(0.f, 0.f), mk(0.f, 0.f), mk(0.f, 0.f), mk(0.f, 0.f)};
              if constexpr (!LEAN) {
                // frames handed over as doubles (main:987): the samples' low words, carried like the normalisation's
                if constexpr (std::is_same<IN_T, float>::value) {
                  if (a.frames_lo && in_row) {
                    const float* lr = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(a.frames_lo) +
                                                                     ((gi * A + ai) * (long long)a.H + r) * a.pitch_bytes) + i0l + 8 * T * c;
#pragma unroll
                    for (int p = 0; p < 4; p++) plo[p] = mk(lr[chunk_pair_offset(p)], lr[chunk_pair_offset(p) + 2]);
                  }
                }
                // Round 6: none of the subtractions on the way rounds at the size of the DC level -- the exact residual of
                // the sample less a (non-integer) dark frame, less the normalisation's minimum, less the pi frame (two_diff)
                // joins the low word.  The dark difference itself was formed above (the row-wise min / max need it); its
                // residual is taken here from the samples still held in `raw`.
                if (a.yd && in_row) {
                  const float* ydr = a.yd + (a.yd_2d ? (size_t)r * W : 0) + i0l + 8 * T * c;
                  v2f orig[4];
                  raw[c].unpack(orig);
#pragma unroll
                  for (int p = 0; p < 4; p++) {
                    v2f e;
                    (void)two_diff(orig[p], mk(ydr[chunk_pair_offset(p)], ydr[chunk_pair_offset(p) + 2]), e);
                    plo[p] += e;
                  }
                }
                if (gnorm) {
#pragma unroll
                  for (int p = 0; p < 4; p++) {
                    v2f e;
                    const v2f vm = two_diff(v[4 * c + p], mk(nmn, nmn), e);
                    const v2f vml = plo[p] + e;
                    v[4 * c + p] = vm * mk(nsc, nsc);
                    plo[p] = pk_fma(vml, mk(nsc, nsc), pk_fma(vm, mk(nsc, nsc), -v[4 * c + p]));
                  }
                }
                if (a.yp && in_row) {
                  const float* ypr = a.yp + (a.yp_2d ? (size_t)r * W : 0) + i0l + 8 * T * c;
#pragma unroll
                  for (int p = 0; p < 4; p++) {
                    v2f e;
                    v[4 * c + p] = two_diff(v[4 * c + p], mk(ypr[chunk_pair_offset(p)], ypr[chunk_pair_offset(p) + 2]), e);
                    plo[p] += e;
                  }
                }
              }
              if (!have_c0 && (LEAN || 8 * T * c < W)) {
                const float cnt = group_sum_f32<T, X::TRIM>(in_row ? 1.f : 0.f);
                c0 = group_sum_f32<T, X::TRIM>(in_row ? v[4 * c].x * ibv[4 * c].x : 0.f) / cnt;   // (cnt >= 1: the chunk's first lane is in the row)
                have_c0 = true;
              }
#pragma unroll
              for (int p = 0; p < 4; p++)
                v[4 * c + p] = in_row ? pk_fma(plo[p], ibv[4 * c + p], pk_fma(v[4 * c + p], ilv[p], pk_fma(v[4 * c + p], ibv[4 * c + p], mk(-c0, -c0)))) : mk(0.f, 0.f);
              const v2f part = (v[4 * c] + v[4 * c + 1]) + (v[4 * c + 2] + v[4 * c + 3]);
              sum += (double)(part.x + part.y);
            }
          }
          // the a plane: issued here so its LDS latency hides under the mean reduction (WCH <= 4)
          if constexpr (WCH <= 4) {
#pragma unroll
            for (int c = 0; c < WCH; c++) load_consts<T>(c_win + c0l, c, av + 4 * c);
            __builtin_amdgcn_sched_barrier(0);
          }
          // ---------------- A3: DC removal (mean in double; CMEAN: mean of the deviations from c0, in float)
          if constexpr (X::CMEAN) {
            const v2f part = (s4[0] + s4[1]) + (s4[2] + s4[3]);
            mh = group_sum_f32<T, X::TRIM>(part.x + part.y) * (1.f / (float)X::WC);
            ml = 0.f;
          } else {
            sum = group_sum<T>(sum);
            const double mean = sum / (double)W;
            mh = (float)mean;
            ml = (float)(mean - (double)mh);
          }
          // the b plane: in flight while the mean is subtracted
          if constexpr (WCH <= 4) {
#pragma unroll
            for (int c = 0; c < WCH; c++) load_consts<T>(c_g + c0l, c, bv + 4 * c);
          }
          if constexpr (X::CMEAN) {
#pragma unroll
            for (int i = 0; i < X::NPR; i++) v[i] -= mk(mh, mh);
          } else {
#pragma unroll
            for (int i = 0; i < X::NPR; i++) v[i] = (v[i] - mk(mh, mh)) - mk(ml, ml);
          }
        }
      }
      FDOCT_FPR(pr, 0);   // row top: the prefetched samples' arrival, unpack, A2 / A3 (division, mean)
      // ---------------- A3 (window) + A5 (first half): s_i = a_i t_i + b_i t_(i-1)
      // (the reference weights the slope by fractionalk[nearestkindex[q]], a per-SAMPLE
      //  quantity, so the slope step is done here once per sample)
      if (!FDOCT_ABL(2)) {
        float* stl = stg + (split ? (i0l >> 1) : i0l);
        float prev_last = 0.f;  // t of the sample just before this lane's chunk
#pragma unroll
        for (int c = 0; c < WCH; c++) {
          if constexpr (!X::RES && WCH > 4) {
            load_consts<T>(c_win + c0l, c, av + 4 * c);
            load_consts<T>(c_g + c0l, c, bv + 4 * c);
          }
          const float last = v[4 * c + 3].y;
          float left;
          if constexpr (T == 64) {
            // wave_shr:1 -- lane i takes lane i-1's last sample, lane 0 keeps `old` = the previous
            // chunk's lane-63 sample (no LDS round trip)
            left = __int_as_float(
                __builtin_amdgcn_update_dpp(__float_as_int(prev_last), __float_as_int(last), 0x138, 0xf, 0xf, false));
            if (c + 1 < WCH) prev_last = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(last), 63));
          } else {
            left = __shfl_up(last, 1, T);
            if (l == 0) left = prev_last;  // last sample of the previous chunk (lane T-1)
            if (c + 1 < WCH) prev_last = __shfl(last, T - 1, T);
          }
          // e0 = (t0,t2), e1 = (t4,t6), o0 = (t1,t3), o1 = (t5,t7); the left neighbours of an odd pair ARE the even pair
          const v2f e0 = v[4 * c], e1 = v[4 * c + 1], o0 = v[4 * c + 2], o1 = v[4 * c + 3];
          v2f pE0 = mk(left, o0.x);
          const v2f pE1 = mk(o0.y, o1.x);
          if (c == 0 && l == 0) pE0.x = o0.x;  // sample 0: slopes[0] = slopes[1] (main:1161), see the planes above
          const v2f sE0 = pk_fma(av[4 * c + 0], e0, bv[4 * c + 0] * pE0);
          const v2f sE1 = pk_fma(av[4 * c + 1], e1, bv[4 * c + 1] * pE1);
          const v2f sO0 = pk_fma(av[4 * c + 2], o0, bv[4 * c + 2] * e0);
          const v2f sO1 = pk_fma(av[4 * c + 3], o1, bv[4 * c + 3] * e1);
          if (LEAN || (i0l + 8 * T * c < W)) {
            if (split) {
              *reinterpret_cast<float4*>(stl + 4 * T * c) = make_float4(sE0.x, sE0.y, sE1.x, sE1.y);
              *reinterpret_cast<float4*>(stl + 4 * T * c + X::WC / 2) = make_float4(sO0.x, sO0.y, sO1.x, sO1.y);
            } else {
              *reinterpret_cast<float4*>(stl + 8 * T * c) = make_float4(sE0.x, sO0.x, sE0.y, sO0.y);
              *reinterpret_cast<float4*>(stl + 8 * T * c + 4) = make_float4(sE1.x, sO1.x, sE1.y, sO1.y);
            }
          }
        }
        if (l == 0) stg[X::WC] = 0.f;  // source of data_ylin[0] and data_ylin[N-1] (defined 0)
      }
      wave_lds_sync();
      FDOCT_FPR(pr, 1);   // window + slope step, staging stores

      // prefetch the next row this group will need (its registers are free from here on)
      {
        long long no = o;
        int na = ai + 1;
        if (na == A) {
          na = 0;
          if constexpr (X::TRO_INPLACE)
            o_next = grp_rows(grp_next_tile(ticket), tro_next);
          else if constexpr (TRO)
            o_next = tro.take(ticket_value(ticket), tro_next, claim);
          else
            o_next = slot_row<X>(ticket_value(ticket));
          no = o_next + sub;
          issue_ib2d<X>(a, no, r_ib, r_il16, il_dma, l);  // r_ib was consumed at the top of this pass
        }
        issue_loads(no, na);
        frame_scale(no, na);
      }

      // ---------------- A5 (second half) + A6: gather into FFT registers
      uint32_t gsrc[X::P];  // packed 16-bit LDS byte offsets (relative to this row's staging buffer)
      if constexpr (!X::GRES) {
        const uint4* gl4 = reinterpret_cast<const uint4*>(c_gi) + l;
#pragma unroll
        for (int q = 0; q < X::P / 4; q++) {
          const uint4 g4 = gl4[q * T];
          gsrc[4 * q + 0] = g4.x; gsrc[4 * q + 1] = g4.y; gsrc[4 * q + 2] = g4.z; gsrc[4 * q + 3] = g4.w;
        }
      }
      if (FDOCT_ABL(2)) {
#pragma unroll
        for (int m = 0; m < X::P; m++) z[m] = v[m % X::NPR];
      } else if constexpr (CPLX) {
        const v2f* phl = c_ph + l;
#pragma unroll
        for (int m = 0; m < X::P; m++) {
          const float y = *reinterpret_cast<const float*>(scr + (gsrc[m] & 0xffffu));
          z[m] = phl[T * m] * mk(y, y);
        }
      } else if constexpr (X::GRES) {
#pragma unroll
        for (int m = 0; m < X::P; m++) {
          const float zx = *reinterpret_cast<const __attribute__((address_space(3))) float*>(gaddr[2 * m]);
          const float zy = *reinterpret_cast<const __attribute__((address_space(3))) float*>(gaddr[2 * m + 1]);
          z[m] = mk(zx, zy);
        }
      } else {
#pragma unroll
        for (int m = 0; m < X::P; m++) {
          const float zx = *reinterpret_cast<const float*>(scr + (gsrc[m] & 0xffffu));
          const float zy = *reinterpret_cast<const float*>(scr + (gsrc[m] >> 16));
          z[m] = mk(zx, zy);
        }
      }
      wave_lds_sync();
      FDOCT_FPR(pr, 2);   // prefetch issue, gather (+ phase multiply)
      }  // STAGE != 2

      if constexpr (STAGE == 1) {
        // resample stage: the packed k-linear row goes to memory, 8 bytes per lane, coalesced
        if (valid) {
          v2f* zr = reinterpret_cast<v2f*>(a.ylin) + o * X::NC + l;
#pragma unroll
          for (int m = 0; m < X::P; m++) __builtin_nontemporal_store(z[m], zr + T * m);
        }
      } else {
      // ---------------- A7: NC-point inverse DFT
      if constexpr (KIND == 1) {
        if (!FDOCT_ABL(4)) fft1024_rowswap<X::RES2, X::RES3>(z, lane, xch, tw_p2, tw_p3, r_t2, r_t3, pr);
      } else if constexpr (KIND == 2) {
        if (!FDOCT_ABL(4)) fft2048_rowswap(z, lane, xch, tw_p2, tw_p3, pr);
      } else if (!FDOCT_ABL(4)) {
        constexpr int NTW2 = (X::P / R2) * (R2 - 1);
        constexpr int NTW3 = (R3 > 1) ? (X::P / R3) * (R3 - 1) : 1;
        pass_compute<X::NC, T, R1, 1, false, X::LP, true>(z, l, xch, nullptr);
        v2f tw2[NTW2];
        pass_twiddles<X::NC, T, R2, R1>(tw2, l, tw_p2);  // queued behind the exchange writes
        wave_lds_sync();
        pass_readback<X::NC, T, X::LP>(z, l, xch);
        wave_lds_sync();
        if constexpr (X::NPASS == 3) {
          pass_compute<X::NC, T, R2, R1, false, X::LP, true>(z, l, xch, tw2);
          v2f tw3[NTW3];
          pass_twiddles<X::NC, T, R3, R1 * R2>(tw3, l, tw_p3);
          wave_lds_sync();
          pass_readback<X::NC, T, X::LP>(z, l, xch);
          wave_lds_sync();
          pass_compute<X::NC, T, R3, R1 * R2, true, X::LP, true>(z, l, xch, tw3);
        } else {
          pass_compute<X::NC, T, R2, R1, true, X::LP, true>(z, l, xch, tw2);
        }
      }

      // ---------------- A8: magnitude (+ untangle on the real path)
      if (FDOCT_ABL(32)) {
#pragma unroll
        for (int m = 0; m < X::P; m++) acc[m] += z[m].x + z[m].y;
      } else if constexpr (CPLX) {
        // slot m is bin l + T*m: with D <= NC/2 (the usual half-depth display) the upper half of the slots is
        // never stored, so its magnitudes (and the epilogue below) are skipped -- a wave-uniform branch
        auto mag_slots = [&](auto lo_c, auto hi_c) {
          static_for<decltype(lo_c)::value, decltype(hi_c)::value>([&](auto mc) {
            constexpr int m = decltype(mc)::value;
            const v2f q = z[m] * z[m];
            acc[m] = AVG ? acc[m] + fast_sqrt(q.x + q.y) : fast_sqrt(q.x + q.y);
          });
        };
        mag_slots(IC<0>{}, IC<X::P / 2>{});
        if (a.D > X::NC / 2) mag_slots(IC<X::P / 2>{}, IC<X::P>{});
      } else {
        untangle_magnitudes<X>(z, acc, utw, lane, l);
      }
      }  // STAGE != 1
      FDOCT_FPR(pr, 8);   // untangle + magnitude (+ accumulate)
      // the prefetched samples have had this whole pass to arrive (see the comment at the first issue_loads)
      if constexpr (STAGE == 2) {
#pragma unroll
        for (int m = 0; m < X::P; m++) asm volatile("" : "+v"(znext[m]));
      } else {
#pragma unroll
        for (int c = 0; c < WCH; c++) raw[c].pin();
        if constexpr (IB2D) {
#pragma unroll
          for (int i = 0; i < X::NPR; i++) asm volatile("" : "+v"(r_ib[i]));
          if constexpr (X::IL16 && !X::ILDMA) {
#pragma unroll
            for (int c = 0; c < WCH; c++) asm volatile("" : "+v"(r_il16[c].x), "+v"(r_il16[c].y), "+v"(r_il16[c].z), "+v"(r_il16[c].w));
          }
        }
      }
    }  // averaging loop
    if constexpr (STAGE == 1) {
      o_wave = o_next;
      continue;
    }

    if constexpr (TRO && !X::TRO_INPLACE) {
      // the ring slot of this row (ticket mod RS) last held the row of ticket - RS: its tile must have been written out
      const unsigned need = tro_cur.t >= RS ? (tro_cur.t - RS) / X::TR + 1u : 0u;
      const unsigned need_steps = need * ((unsigned)a.D / (unsigned)X::TRO_SB);
      // (the write-out this waits for may be this wave's own to do; the bound is the exit condition a spinning wave must
      // have all the same and is reported through a.tr_fault)
      for (unsigned spin = 0; tro_done_seen < need_steps; spin++) {
        tro_done_seen = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&tr_wo_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (tro_done_seen >= need_steps) break;
        if (spin >= FDOCT_TRO_SPIN_LIMIT) {
          if (lane == 0) __hip_atomic_store(a.tr_fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          break;
        }
        if (!tro_writeout(1)) __builtin_amdgcn_s_sleep(2);
      }
    }
    // ---------------- A9/A10: average, epsilon, dB, DC mask, store
    const int D = a.D;
    const bool upper_slots = !CPLX || D > X::NC / 2;  // complex path, half-depth output: slots >= P/2 are never stored
    float outv[X::P];
    // (without averaging the epsilon add goes two slots to a packed add: each half rounds like the single add)
    auto add_eps = [&](auto lo_c, auto hi_c) {
      if constexpr (AVG) {
#pragma unroll
        for (int m = decltype(lo_c)::value; m < decltype(hi_c)::value; m++) outv[m] = fmaf(acc[m], a.inv_A, a.eps);
      } else {
#pragma unroll
        for (int m = decltype(lo_c)::value; m < decltype(hi_c)::value; m += 2) {
          const v2f o = mk(acc[m], acc[m + 1]) + mk(a.eps, a.eps);
          outv[m] = o.x;
          outv[m + 1] = o.y;
        }
      }
    };
    add_eps(IC<0>{}, IC<X::P / 2>{});
    if (upper_slots) {
      add_eps(IC<X::P / 2>{}, IC<X::P>{});
    } else {
#pragma unroll
      for (int m = X::P / 2; m < X::P; m++) outv[m] = 1.f;
    }
    // slot -> depth bin.  Complex path: slot m is bin l + T*m.  Real path (see the untangle above):
    // slots m < P/2 are bins l + T*m, slots P/2 + m are bins NC - l - T*m (lane 0, m = 0: bin NC/2).
    // Stores are <per-lane base pointer> + <immediate>: lo slots ascend from orow + l, hi slots
    // descend from orow + NC - l (a wave still writes 64 consecutive floats per instruction).
    // Non-temporal stores: the output is a stream nobody on this GPU reads back soon (+0.8 % on C2).
    // BUFFER stores: a wave's RPW rows are consecutive rows of the output, so one descriptor (four SGPRs) based at the
    // wave's first row covers them and the per-lane part is one 32-bit byte offset, where a global store carries a
    // 64-bit VGPR address (+1.6 % on C2: fewer address registers read per store).  num_records = the floats of the
    // wave's valid rows: the hardware drops the rows past the end of the batch and, with one row per wave, whatever lies
    // past the crop.
    auto store_row = [&](float* obase, const float* val) {
      constexpr int NLO = CPLX ? X::P : X::P / 2;
      constexpr bool BUF = !TRO;  // (the transposed store's rows go into LDS: plain ds_write_b32)
      // o_wave is wave-uniform by construction (slot_row of a wave-uniform ticket); say so for RPW > 1 too, or the
      // descriptor would be built per lane and the stores wrapped in a waterfall loop
      const long long ow = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(o_wave >> 32)) << 32) |
                                       (unsigned)__builtin_amdgcn_readfirstlane((int)o_wave));
      const long long left = total - ow;  // >= 1 inside the row loop
      int nrows = left < X::RPW ? (int)left : X::RPW;
      float* wbase = obase + (size_t)ow * D;  // the wave's first row
      float* orow = wbase + ((X::RPW > 1) ? (size_t)sub * D : 0);
      // this row's ring slot (LDS: the stores below are ds_write_b32); the RPW rows of a wave take consecutive slots (the ring
      // is a whole number of them: fused_tro_ring_pick)
      if constexpr (X::TRO_INPLACE)
        orow = reinterpret_cast<float*>(scratch0 + (size_t)(wave * X::RPW + sub) * a.scratch_bytes);   // the row's own buffer, free since the untangle
      else if constexpr (TRO)
        orow = tro_ring + (tro.ring_mod(tro_cur.t) + (unsigned)sub) * tro_slot;
      __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(BUF ? wbase : nullptr, 0, BUF ? nrows * D * 4 : 0, 0x00020000);
      // bin index -> store; lo(m) = bin l + T*m, hi(m) = bin NC - l - T*m, hi0 = slot P/2 (lane 0: bin NC/2)
      float* plo = orow + l;
      float* phi = orow + (X::NC - l);
      // per-lane byte offsets of the ascending and of the descending run; opaque to the optimiser so that "+ constant"
      // stays an add the backend folds into the instruction's immediate offset (it does not fold the `or` it would become)
      const int vrow = (X::RPW > 1) ? 4 * sub * D : 0;
      int vlo = vrow + 4 * l, vhi = vrow + 4 * (X::NC - T * (X::P / 2 - 1) - l);
      if constexpr (BUF) asm volatile("" : "+v"(vlo), "+v"(vhi));
      auto st_lo = [&](int m, float v) {
        if constexpr (BUF)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs, vlo + 4 * T * m, 0, 2);  // aux 2 = nt
        else
          plo[T * m] = v;
      };
      auto st_hi = [&](int m, float v) {
        if constexpr (BUF)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs, vhi + 4 * T * (X::P / 2 - 1 - m), 0, 2);
        else
          phi[-T * m] = v;
      };
      auto st_hi0 = [&](float v) {  // slot P/2 of lane 0 is bin NC/2
        if constexpr (BUF)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs, vrow + 4 * ((l == 0) ? X::NC / 2 : X::NC - l), 0, 2);
        else
          *((l == 0) ? orow + X::NC / 2 : phi) = v;
      };
      if (D == X::NC || (BUF && X::RPW == 1 && (D % T) != 0)) {  // full depth: nothing to crop; ragged crop of a wave-per-row plan: the hardware drops bins >= D
#pragma unroll
        for (int m = 0; m < NLO; m++) st_lo(m, val[m]);
        if constexpr (!CPLX) {
          st_hi0(val[NLO]);
#pragma unroll
          for (int m = 1; m < X::P / 2; m++) st_hi(m, val[NLO + m]);
        }
      } else if ((D % T) == 0) {
        // cropped to whole T-bin slots (the usual half-depth display): which slots are stored is the same for every
        // lane, so the tests are scalar branches -- no per-store exec masking (and none of its SGPR pressure)
        const int nfull = D / T;
#pragma unroll
        for (int m = 0; m < NLO; m++)
          if (m < nfull) st_lo(m, val[m]);
        if constexpr (!CPLX) {
          const int h = (X::NC - D) / T;  // >= 1: hi slot m holds bins NC - T*m - l, all below D iff m > h
          if (((l == 0) ? X::NC / 2 : X::NC - l) < D) st_hi0(val[NLO]);
#pragma unroll
          for (int m = 1; m < X::P / 2; m++) {
            if (m > h) {
              st_hi(m, val[NLO + m]);
            } else if (m == h) {
              if (l != 0) st_hi(m, val[NLO + m]);  // lane 0's bin is D itself
            }
          }
        }
      } else {
#pragma unroll
        for (int m = 0; m < NLO; m++)
          if (l + T * m < D) st_lo(m, val[m]);
        if constexpr (!CPLX) {
          if (((l == 0) ? X::NC / 2 : X::NC - l) < D) st_hi0(val[NLO]);
#pragma unroll
          for (int m = 1; m < X::P / 2; m++)
            if (X::NC - l - T * m < D) st_hi(m, val[NLO + m]);
        }
      }
    };
    const bool deposit = valid && !(X::TRO_INPLACE && tro_cur.dummy);   // (a wave without rows in a short tile stores nothing)
    if (deposit && a.out_mag && !FDOCT_ABL(128)) store_row(a.out_mag, outv);
    // (transposed store with both images asked for: the ring holds bscan, the write-out step takes the logarithm)
    if (a.out_db && !(TRO && a.out_mag)) {
      float db[X::P];
#pragma unroll
      for (int m = 0; m < X::P / 2; m++) db[m] = FDOCT_ABL(64) ? outv[m] : a.db_scale * fast_log2(outv[m]);  // db_scale carries ln 2
      if (upper_slots) {
#pragma unroll
        for (int m = X::P / 2; m < X::P; m++) db[m] = FDOCT_ABL(64) ? outv[m] : a.db_scale * fast_log2(outv[m]);
      } else {
#pragma unroll
        for (int m = X::P / 2; m < X::P; m++) db[m] = 0.f;
      }
      if (a.dcmask && T > 4 && D > 4) {  // (the reference indexes row 4 unconditionally; with D <= 4 there is none: no mask)
        // depth bins 0 and 1 <- bin 4 (main:1237-1238): bins 0, 1, 4 are slot 0 of lanes 0, 1, 4
        const float d4 = __shfl(db[0], (lane & ~(T - 1)) | 4, 64);
        if (l < 2) db[0] = d4;
      }
      if (deposit && !FDOCT_ABL(128)) store_row(a.out_db, db);
      if (FDOCT_ABL(128)) {  // keep the values alive: without this the whole row would be dead code
#pragma unroll
        for (int m = 0; m < X::P; m++) asm volatile("" ::"v"(db[m]));
      }
    }
    o_wave = o_next;
    FDOCT_FPR(pr, 9);     // epilogue: average, epsilon, dB, stores (+ the transposed store's ring wait)
    if constexpr (X::TRO_INPLACE) {
      // the wave's rows lie in its own row buffers: meet the group, write the tile out together (wave m takes steps m, m + 4, ...:
      // each step reads all sixteen rows, four of them from every wave's buffers), meet again -- nobody may start staging its
      // next rows before every wave of the group has read what it needs -- and go on
      wave_lds_sync();
      const unsigned target = X::GW * (grp_seq + 1u);
      grp_meet(&grp_arrived[grp], target);
      asm volatile("" ::: "memory");
      const unsigned spt = (unsigned)a.D / (unsigned)X::TRO_SB;
      for (unsigned k = mem; k < spt; k += X::GW) tro.step(grp, tro_cur.g, tro_cur.r0, tro_cur.nrows, (int)(k * (unsigned)X::TRO_SB));
      asm volatile("" ::: "memory");   // the steps' LDS reads have returned (they fed stores that have been issued)
      wave_lds_sync();
      grp_meet(&grp_done[grp], target);
      grp_seq++;
      tro_cur = tro_next;
    } else if constexpr (TRO) {
      // the row is in the ring (a wave's LDS operations execute in order): count it for the write-out
      wave_lds_sync();
      // count the row, and read the write-out state in the same LDS round trip
      unsigned cnt = 0u;
      if (lane == 0) cnt = __hip_atomic_fetch_add(&tr_arrived[tro_cur.tq & 3u], (unsigned)X::RPW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const unsigned s_l = __hip_atomic_load(&tr_wo_next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const unsigned r_l = __hip_atomic_load(&tr_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      unsigned ready = (unsigned)__builtin_amdgcn_readfirstlane((int)r_l);
      if ((unsigned)__builtin_amdgcn_readfirstlane((int)cnt) + (unsigned)X::RPW == tro_cur.nrows)  // the tile is complete: publish it
        ready = tro_publish(tro_cur.tq, &tr_ready);
      // (one write-out step per row put into the ring: 400 M A-scans/s on C2 against 392 with two and 385 with four)
      (void)tro_try_step((unsigned)__builtin_amdgcn_readfirstlane((int)s_l), ready);
      tro_cur = tro_next;
    }
  }
  if constexpr (TRO && !X::TRO_INPLACE) {
    // all rows of this wave are done: help until the workgroup's last tile is out (it completes when its last row is in the
    // ring, which needs no help from here; the bound is the exit condition a spinning wave must have all the same)
    // (TroGeom::bperm() written out again, on purpose: calling it here exchanges two s_mov in the averaging two-word
    // transposed-store kernels -- profiles/fused_phases_codeobj_identity.txt)
    const unsigned nx_ = gridDim.x >> 3;
    const unsigned bp_ = (gridDim.x & 7u) ? blockIdx.x : (blockIdx.x & 7u) * nx_ + (blockIdx.x >> 3);
    const unsigned my_tiles = bp_ < a.tr_total_tiles ? (a.tr_total_tiles - bp_ + gridDim.x - 1u) / gridDim.x : 0u;
    for (unsigned spin = 0;; spin++) {
      const unsigned outn = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&tr_wo_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      if (outn >= my_tiles * ((unsigned)a.D / (unsigned)X::TRO_SB)) break;
      if (tro_writeout(4)) {
        spin = 0;
        continue;
      }
      if (spin >= FDOCT_TRO_SPIN_LIMIT) {
        if (lane == 0) __hip_atomic_store(a.tr_fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
  }
#ifdef FDOCT_FUSED_PROBE
  if (a.phase_probe && lane == 0 && blockIdx.x < 4 && wave < 16) {
    for (int i = 0; i < FUSED_PROBE_PHASES; i++) a.phase_probe[(blockIdx.x * 16 + wave) * FUSED_PROBE_PHASES + i] = pr.acc[i];
  }
#endif
#ifdef FDOCT_CLOCKPROBE
  if (a.probe && blockIdx.x == 0 && lane == 0 && wave < 16) {
    a.probe[2 * wave] = __builtin_readcyclecounter() - probe_c0;
    a.probe[2 * wave + 1] = wall_clock64() - probe_r0;
  }
  if (a.probe && tid == 0 && blockIdx.x < 512) {  // per-workgroup start / end on the chip-wide 100 MHz clock
    a.probe[32 + 2 * blockIdx.x] = probe_r0;
    a.probe[32 + 2 * blockIdx.x + 1] = wall_clock64();
  }
#endif
}

#ifndef FDOCT_ONLY_PLAN  // (per-plan translation units hold the fused kernels only)
#include "fdoct_prepass_kernels.inc"

#endif  // !FDOCT_ONLY_PLAN

// ---------------------------------------------------------------- dispatch --
template <typename X>
struct TypeTag {
  using type = X;
};

template <int LOG2NC, int T, int R1, int R2, int R3, int KIND, int WCH, typename IN_T, bool CPLX, bool LEAN, int STAGE = 0, bool AVG = true,
          bool IB2D = false, int NORM = 0, bool TRO = false, bool PRECT = false>
static hipError_t launch_one(const FusedArgs& a, dim3 grid, dim3 block, size_t lds, hipStream_t st) {
  auto k = fused_kernel<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, LEAN, STAGE, AVG, IB2D, NORM, TRO, PRECT>;
  static LdsGrant grant;  // one per instantiation
  if (hipError_t e = grant.ensure(k, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL(k, grid, block, lds, st, a);
  return hipGetLastError();
}

// PRECT: the fast-path instantiations that multiply by both words of the reciprocal background (a.prec != 0 on a lean
// launch); they live in translation units of their own (launch_plan<ID, true>).  The any-option kernel (always both words)
// and the one-word fast path are launch_plan<ID, false>.
template <int LOG2NC, int T, int R1, int R2, int R3, int KIND, int WCH, bool CPLX, bool PRECT>
static hipError_t launch_typed(const FusedArgs& a, int dtype, bool lean, dim3 grid, dim3 block, size_t lds,
                               hipStream_t st) {
  if (PRECT != (lean && a.prec != 0)) return hipErrorInvalidValue;  // (launch_fused picks the translation unit)
#ifdef FDOCT_DEV_ONE  // tuning builds (tools/mkvariant.sh): ONE instantiation -- plain u16 fast path, fused, no averaging
  if constexpr (FDOCT_DEV_ONE_CPLX != CPLX) return hipErrorNotSupported;
  else {
    if (!lean || dtype != FDOCT_K_U16 || a.stage != 0 || a.ib2d || a.minmax || a.rowwisenormalize) return hipErrorNotSupported;
    if ((a.A == 1) != (FDOCT_DEV_ONE_AVG == 0)) return hipErrorNotSupported;
    if constexpr (fused_tro_compiled(KIND, T, WCH) && !CPLX) {
      if (a.tro) return launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, uint16_t, CPLX, true, 0, FDOCT_DEV_ONE_AVG != 0, false, 0, true, PRECT>(a, grid, block, lds, st);
    } else if (a.tro) {
      return hipErrorNotSupported;
    }
    return launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, uint16_t, CPLX, true, 0, FDOCT_DEV_ONE_AVG != 0, false, 0, false, PRECT>(a, grid, block, lds, st);
  }
#else
  if (a.stage != 0) {  // staged mode: built for the fast-path configuration only
    if (!lean || dtype != FDOCT_K_U16) return hipErrorNotSupported;  // (capi checks this before launching)
    // the resample stage always runs over INPUT A-scans (capi hands it A = 1); the FFT stage averages (and reads no samples:
    // one instantiation serves both modes)
    if (a.stage == 1)
      return a.A == 1 ? launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, uint16_t, CPLX, true, 1, false, false, 0, false, PRECT>(a, grid, block, lds, st)
                      : hipErrorNotSupported;
    return a.A == 1 ? launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, uint16_t, CPLX, true, 2, false, false, 0, false, PRECT>(a, grid, block, lds, st)
                    : launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, uint16_t, CPLX, true, 2, true, false, 0, false, PRECT>(a, grid, block, lds, st);
  }
  if (a.tro) {  // transposed output written by the chain itself (capi checks the conditions before asking for it)
    if constexpr (fused_tro_compiled(KIND, T, WCH) && !CPLX) {
      if (!lean || a.rowwisenormalize || !a.tr_fault) return hipErrorNotSupported;
      // the plain acquisition configuration with any averaging; one frame per B-scan also with a full-frame background and /
      // or the whole-frame normalisation (what the 'b' key stores, what BscanFFTsim.cpp always does: sim:803-813, 845)
      auto tro = [&](auto in_c) {
        using IN_T = typename decltype(in_c)::type;
        if (a.ib2d || a.minmax) {
          if (a.A != 1) return hipErrorNotSupported;
          if constexpr (KIND != 1) {   // (the 512-point Stockham plan: plain and averaging only; the host keeps the rest on the two-pass route)
            return hipErrorNotSupported;
          } else {
            if constexpr (!PRECT || fused_il_half(true, WCH)) {  // (both words with a full-frame background: the half-float form only)
              if (a.ib2d && a.minmax) return launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, true, 0, false, true, 1, true, PRECT>(a, grid, block, lds, st);
              if (a.ib2d) return launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, true, 0, false, true, 0, true, PRECT>(a, grid, block, lds, st);
            } else if (a.ib2d) {
              return hipErrorNotSupported;
            }
            return launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, true, 0, false, false, 1, true, PRECT>(a, grid, block, lds, st);
          }
        }
        return a.A == 1 ? launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, true, 0, false, false, 0, true, PRECT>(a, grid, block, lds, st)
                        : launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, true, 0, true, false, 0, true, PRECT>(a, grid, block, lds, st);
      };
      if (dtype == FDOCT_K_U16) return tro(TypeTag<uint16_t>{});
      if (dtype == FDOCT_K_U8) return tro(TypeTag<uint8_t>{});
    }
    return hipErrorNotSupported;
  }
  if constexpr ((KIND == 1 || KIND == 2) && WCH <= 4) {
    // fast path with a full-frame background (capi hands the evens/odds-ordered copy) and / or a normalisation
    if (lean && (a.ib2d || a.minmax || a.rowwisenormalize)) {
      auto opts = [&](auto in_c, auto avg_c) {
        using IN_T = typename decltype(in_c)::type;
        constexpr bool AVG = decltype(avg_c)::value;
        if constexpr (!fused_resident_consts(KIND, true, AVG, WCH, 0)) {
          return hipErrorNotSupported;  // (capi keeps such configurations on the general kernel)
        } else {
        const int norm = a.rowwisenormalize ? 2 : (a.minmax ? 1 : 0);
        if (a.ib2d) {
          if constexpr (!PRECT || fused_il_half(true, WCH)) {
            if (norm == 2) return launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, true, 0, AVG, true, 2, false, PRECT>(a, grid, block, lds, st);
            if (norm == 1) return launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, true, 0, AVG, true, 1, false, PRECT>(a, grid, block, lds, st);
            return launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, true, 0, AVG, true, 0, false, PRECT>(a, grid, block, lds, st);
          } else {
            return hipErrorNotSupported;
          }
        }
        if (norm == 2) return launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, true, 0, AVG, false, 2, false, PRECT>(a, grid, block, lds, st);
        return launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, true, 0, AVG, false, 1, false, PRECT>(a, grid, block, lds, st);
        }
      };
      if (dtype == FDOCT_K_U16)
        return a.A == 1 ? opts(TypeTag<uint16_t>{}, std::false_type{}) : opts(TypeTag<uint16_t>{}, std::true_type{});
      if (dtype == FDOCT_K_U8)
        return a.A == 1 ? opts(TypeTag<uint8_t>{}, std::false_type{}) : opts(TypeTag<uint8_t>{}, std::true_type{});
      return hipErrorInvalidValue;
    }
  }
  auto plain = [&](auto in_c) {
    using IN_T = typename decltype(in_c)::type;
    if (lean)
      return a.A == 1 ? launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, true, 0, false, false, 0, false, PRECT>(a, grid, block, lds, st)
                      : launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, true, 0, true, false, 0, false, PRECT>(a, grid, block, lds, st);
    if constexpr (!PRECT)
      return launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, IN_T, CPLX, false>(a, grid, block, lds, st);
    else
      return hipErrorInvalidValue;
  };
  switch (dtype) {
    case FDOCT_K_U16: return plain(TypeTag<uint16_t>{});
    case FDOCT_K_U8: return plain(TypeTag<uint8_t>{});  // 8-bit cameras (the shipped ini's default) get the fast path too
    case FDOCT_K_F32:
      if constexpr (!PRECT)
        return launch_one<LOG2NC, T, R1, R2, R3, KIND, WCH, float, CPLX, false>(a, grid, block, lds, st);
      else
        return hipErrorInvalidValue;
    default:
      return hipErrorInvalidValue;
  }
#endif  // FDOCT_DEV_ONE
}

// The table of compiled plans: {id, log2 nc, T, R1, R2, R3, kind, WCH}.  nc = complex FFT length;
// kind 0 = Stockham passes through LDS, kind 1 = fft1024_rowswap, kind 2 = fft2048_rowswap.
#ifdef FDOCT_DEV_ONE  // fastest compile while tuning: one instantiation of one plan (-DFDOCT_DEV_ONE=<plan id>)
#define FDOCT_DEV_SINGLE
#define FDOCT_PLAN_1(X) X(1, 9, 16, 32, 16, 1, 0, 8)
#define FDOCT_PLAN_5(X) X(5, 10, 64, 16, 4, 16, 1, 4)
#define FDOCT_PLAN_7(X) X(7, 11, 64, 32, 4, 16, 2, 4)
#define FDOCT_PLAN_8(X) X(8, 11, 64, 32, 4, 16, 2, 8)
#define FDOCT_CAT_(a, b) a##b
#define FDOCT_CAT(a, b) FDOCT_CAT_(a, b)
#define FDOCT_PLANS(X) FDOCT_CAT(FDOCT_PLAN_, FDOCT_DEV_ONE)(X)
#elif defined(FDOCT_DEV_SINGLE)  // fast compile while tuning: only the benchmark plan
#define FDOCT_PLANS(X) X(5, 10, 64, 16, 4, 16, 1, 4)
#else
#define FDOCT_PLANS(X)               \
  X(0, 8, 16, 16, 16, 1, 0, 4)       \
  X(1, 9, 16, 32, 16, 1, 0, 8)       \
  X(2, 10, 64, 16, 16, 4, 0, 4)      \
  X(3, 10, 32, 32, 32, 1, 0, 8)      \
  X(4, 11, 64, 32, 8, 8, 0, 8)       \
  X(5, 10, 64, 16, 4, 16, 1, 4)      \
  X(6, 11, 64, 32, 8, 8, 0, 4)       \
  X(7, 11, 64, 32, 4, 16, 2, 4)      \
  X(8, 11, 64, 32, 4, 16, 2, 8)
#endif

template <int ID>
struct PlanOf;
#define FDOCT_PLANOF(ID, L2_, T_, R1_, R2_, R3_, K_, WCH_)                                      \
  template <>                                                                                   \
  struct PlanOf<ID> {                                                                           \
    static constexpr int L2 = L2_, T = T_, R1 = R1_, R2 = R2_, R3 = R3_, K = K_, WCH = WCH_;    \
  };
FDOCT_PLANS(FDOCT_PLANOF)
#undef FDOCT_PLANOF

// Every instantiation of one plan.  The build compiles this file once per plan (-DFDOCT_ONLY_PLAN=<id>: that
// translation unit instantiates launch_plan<id> and nothing else) plus once for everything else, in parallel.
template <int ID, bool PRECT>
hipError_t launch_plan(const FusedArgs& a, int dtype, bool cplx, bool lean, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  using P = PlanOf<ID>;
  return cplx ? launch_typed<P::L2, P::T, P::R1, P::R2, P::R3, P::K, P::WCH, true, PRECT>(a, dtype, lean, g, b, lds, st)
              : launch_typed<P::L2, P::T, P::R1, P::R2, P::R3, P::K, P::WCH, false, PRECT>(a, dtype, lean, g, b, lds, st);
}

#ifdef FDOCT_ONLY_PLAN
#ifndef FDOCT_ONLY_PRECT
#define FDOCT_ONLY_PRECT 0
#endif
template hipError_t launch_plan<FDOCT_ONLY_PLAN, FDOCT_ONLY_PRECT != 0>(const FusedArgs&, int, bool, bool, dim3, dim3, size_t, hipStream_t);
#else
#ifndef FDOCT_DEV_SINGLE
#define FDOCT_EXTERN(ID, L2, T_, R1_, R2_, R3_, K_, WCH_)                                                                    \
  extern template hipError_t launch_plan<ID, false>(const FusedArgs&, int, bool, bool, dim3, dim3, size_t, hipStream_t); \
  extern template hipError_t launch_plan<ID, true>(const FusedArgs&, int, bool, bool, dim3, dim3, size_t, hipStream_t);
FDOCT_PLANS(FDOCT_EXTERN)
#undef FDOCT_EXTERN
#endif

int fused_plan_count() {
  int n = 0;
#define FDOCT_COUNT(ID, L2, T_, R1_, R2_, R3_, K_, WCH_) n++;
  FDOCT_PLANS(FDOCT_COUNT)
#undef FDOCT_COUNT
  return n;
}

bool fused_plan_get(int id, FusedPlan* p) {
#define FDOCT_GET(ID, L2, T_, R1_, R2_, R3_, K_, WCH_)        \
  if (id == ID) {                                             \
    *p = FusedPlan{ID, 1 << L2, T_, R1_, R2_, R3_, WCH_, K_}; \
    return true;                                              \
  }
  FDOCT_PLANS(FDOCT_GET)
#undef FDOCT_GET
  return false;
}

hipError_t launch_fused(const FusedPlan& p, const FusedArgs& a, int dtype, bool cplx, bool lean, int grid, int block,
                        size_t lds, hipStream_t st) {
  dim3 g(grid), b(block);
#define FDOCT_CASE(ID, L2, T_, R1_, R2_, R3_, K_, WCH_) \
  if (p.id == ID) return (lean && a.prec) ? launch_plan<ID, true>(a, dtype, cplx, lean, g, b, lds, st) : launch_plan<ID, false>(a, dtype, cplx, lean, g, b, lds, st);
  FDOCT_PLANS(FDOCT_CASE)
#undef FDOCT_CASE
  return hipErrorInvalidValue;
}

#include "fdoct_prepass_launch.inc"

#endif  // !FDOCT_ONLY_PLAN

}  // namespace fdoct
