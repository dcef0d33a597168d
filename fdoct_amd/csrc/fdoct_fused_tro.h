// fdoct_fused_tro.h -- the transposed store of fused_kernel (fdoct_kernels.hip): the outputs written as bscan[depth][row] by the
// chain itself.  Here: the geometry (TroGeom: tiles, ring slots, one write-out step, ticket -> row).
// The ring protocol of the kernels with one row per wave and the group protocol of the kernels with four work on the kernel's
// __shared__ counters and stay lambdas of the kernel: handed the counters, the same instructions come out in another order
// (profiles/fused_phases_codeobj_identity.txt).
//
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
// TRO with FOUR rows per wave (the 512-point plan, round 6): no ring.  A GROUP of four waves (GW, fdoct_fused_rules.h) owns a
//   tile of 16 rows; a finished row is deposited in the wave's OWN row buffer (free between the untangle and the next row's
//   staging), the group meets, writes the tile out together, meets again, and goes on -- all eight waves compute (the ring
//   cost two of them their LDS).
#pragma once
#include "fdoct_fused_dev.h"

// Wait states after each 16-byte store of the tile write-out.  Measured on gfx950: a buffer_store_dwordx4 with an SGPR
// soffset followed directly by a VALU write of its first data register stores the NEW value in the last four lanes of each
// 16-lane row when the memory pipeline is busy (the compiler's hazard recogniser only covers the immediate-offset form of
// this store-data hazard); one wait state cures it, two are used.
constexpr int FDOCT_TRO_NOP = 2;

namespace fdoct {

// TRO: ticket t of this workgroup is row t % TR of its tile t / TR (the missing rows of a short tile use up tickets that
// name no row).
struct TroRow {
  unsigned t, tq, rt, g, r0, nrows;  // ticket, workgroup tile number, row in tile, B-scan, first row of the tile in the B-scan, rows of the tile
  bool dummy;                        // (four rows per wave) a short tile has no rows for this wave: it recomputes rows of the tile and stores nothing
};

// ---- geometry.  X: the kernel's FusedTraits.
template <class X>
struct TroGeom {
  const FusedArgs& a;
  // ring slots: one of a few compile-time values (kTroRingChoices), so that "mod RS" stays a multiplication; the launch picks
  // the largest that fits the LDS (wave-uniform: a scalar branch)
  const unsigned RS;
  // the ring lies behind the waves' row buffers; a slot is D + 4 floats (the pad moves consecutive rows 4 banks apart)
  float* const ring;
  const int slot;
  unsigned char* const scratch0;  // the waves' row buffers, a.scratch_bytes apart
  const int lane;

  // this workgroup's place in the order the tiles are handed out in: workgroups b, b + 8, b + 16 .. run on the same XCD
  // (round-robin dispatch) at about the same time: they get a run of NEIGHBOURING tiles, so that the two 64-byte halves of
  // every 128-byte line of the B-scan meet in one L2 (a performance matter only: any bijection of the workgroups is correct)
  __device__ __forceinline__ unsigned bperm() const {
    const unsigned nx = gridDim.x >> 3;
    return (gridDim.x & 7u) ? blockIdx.x : (blockIdx.x & 7u) * nx + (blockIdx.x >> 3);
  }
  // Tiles.  Tile q of workgroup b is tile q * grid + b of the batch (front to back); tiles never straddle B-scans
  // (the last tile of a B-scan may be short).  Wave-uniform, scalar unit.
  __device__ __forceinline__ bool tile(unsigned tq, unsigned& g, unsigned& r0, unsigned& nrows) const {  // false: past the end of the batch
    const unsigned gt = tq * gridDim.x + bperm();
    if (gt >= a.tr_total_tiles) return false;
    g = __umulhi(gt, a.tr_tpf_magic);  // gt / tiles-per-frame: floor(2^32 / tpf) under-estimates by at most one
    unsigned tf = gt - g * a.tr_tpf;
    if (tf >= a.tr_tpf) {
      g++;
      tf -= a.tr_tpf;
    }
    r0 = tf * X::TR;
    const unsigned left = (unsigned)a.H - r0;
    nrows = left < X::TR ? left : X::TR;
    return true;
  }
  __device__ __forceinline__ unsigned ring_mod(unsigned x) const {
    switch (RS) {
      case 21: return x % 21u;
      case 22: return x % 22u;
      case 23: return x % 23u;
      case 24: return x % 24u;
      case 26: return x % 26u;
      case 28: return x % 28u;
      case 32: return x % 32u;
      case 40: return x % 40u;
      case 44: return x % 44u;
      case 48: return x % 48u;
      default: return x % 20u;
    }
  }
  // One write-out step: bins s0 .. s0 + SB - 1 of tile tq, all its rows.  Lane (dg, rq) takes rows 4 rq .. 4 rq + 3 and bins
  // 4 dg .. 4 dg + 3: four ds_read_b128 (one per row), four 16-byte stores (one per bin: the lanes of a row-quad group cover
  // TR * 4 contiguous bytes of the B-scan).  When both images are asked for the ring holds bscan and the logarithm is taken
  // here (the same instruction on the same value as the epilogue's).
  __device__ __forceinline__ void step(unsigned tq, unsigned g, unsigned r0, unsigned nrows, int s0) const {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int rq = lane % X::TRO_RQ, dg = lane / X::TRO_RQ;
    const int Dn = a.D, Hn = a.H;
    if (4 * rq >= (int)nrows) return;
    const bool both = a.out_mag && a.out_db;
    const bool mask = both && a.dcmask && Dn > 4;  // dB bins 0, 1 <- bin 4 (main:1237-1238); alone, dB arrives masked
    float* const out0 = a.out_mag ? a.out_mag : a.out_db;
    const int Hs = Hn;
    const int vout = (4 * dg * Hs + 4 * rq) * 4;
    const float* rowp[4];
    if constexpr (X::TRO_INPLACE) {
      // rows 4 rq .. 4 rq + 3 of the tile lie in the row buffers of wave rq of the group (tq names the GROUP here): row i of the
      // tile is row buffer 16 group + i, buffers scratch_bytes apart (1060 floats: four banks on, like the ring's slots)
#pragma unroll
      for (int i = 0; i < 4; i++)
        rowp[i] = reinterpret_cast<const float*>(scratch0 + (size_t)(X::TR * tq + 4u * (unsigned)rq + (unsigned)i) * a.scratch_bytes) + 4 * dg + s0;
    } else {
      const unsigned sl0 = ring_mod(X::TR * tq + 4u * (unsigned)rq);  // this lane's four rows: ring slots (TR tq + 4 rq + i) mod RS
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const unsigned sl = sl0 + i >= RS ? sl0 + i - RS : sl0 + i;
        rowp[i] = ring + sl * slot + 4 * dg + s0;
      }
    }
    const size_t goff = ((size_t)g * Dn) * Hn + r0;
    __amdgpu_buffer_rsrc_t rout0 = __builtin_amdgcn_make_buffer_rsrc(out0 + goff, 0, 0x7ffffff0, 0x00020000);
    f4 v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = *reinterpret_cast<const f4*>(rowp[i]);
    // Cache policy of the stores (the last argument): 0 = write-back.  The two 64-byte halves of a 128-byte line of the B-scan
    // come from neighbouring tiles, which tile() hands to workgroups of the same XCD: with write-back stores they meet in that
    // L2 and leave it as one line.  Measured (C2, M A-scans/s): nt 277, write-back 329, sc1 357-376; with the tile pairing sc1
    // 367-380, write-back 395-406.
#pragma unroll
    for (int bb = 0; bb < 4; bb++) {
      const f4 w = {v[0][bb], v[1][bb], v[2][bb], v[3][bb]};
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, w), rout0, vout, ((s0 + bb) * Hs) * 4, 0);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_nop %0" ::"n"(FDOCT_TRO_NOP - 1));
      __builtin_amdgcn_sched_barrier(0);
    }
    if (both) {
      __amdgpu_buffer_rsrc_t rout1 = __builtin_amdgcn_make_buffer_rsrc(a.out_db + goff, 0, 0x7ffffff0, 0x00020000);
      f4 v4 = {0.f, 0.f, 0.f, 0.f};  // bin 4 of the four rows (DC mask)
      if (mask && s0 == 0 && dg == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) v4[i] = rowp[i][4];
      }
#pragma unroll
      for (int bb = 0; bb < 4; bb++) {
        f4 w = {v[0][bb], v[1][bb], v[2][bb], v[3][bb]};
        if (mask && bb < 2 && s0 == 0 && dg == 0) w = v4;
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = a.db_scale * fast_log2(w[k]);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, w), rout1, vout, ((s0 + bb) * Hs) * 4, 0);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop %0" ::"n"(FDOCT_TRO_NOP - 1));
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  // (RPW > 1, round 6: a claim names RPW consecutive rows -- RPW divides the tile and, host-checked, the frame height, so the
  // rows of a claim are all there or all missing; t, rt count ROWS: the first row of the claim)
  __device__ __forceinline__ int map(unsigned tc, TroRow& tr) const {  // tc: the claimed ticket.  0: rows; 1: no such rows in this (short) tile; 2: past the end of the batch
    const unsigned t = tc * (unsigned)X::RPW;
    tr.t = t;
    tr.tq = t / X::TR;
    tr.rt = t % X::TR;
    if (!tile(tr.tq, tr.g, tr.r0, tr.nrows)) return 2;
    return tr.rt < tr.nrows ? 0 : 1;
  }
  template <class Claim>   // claim(): the kernel's row ticket
  __device__ __forceinline__ long long take(unsigned t, TroRow& tr, const Claim& claim) const {  // t: a claimed ticket (uniform); claims on while tickets name no row
    for (;;) {
      const int k = map(t, tr);
      if (k == 0) return (long long)tr.g * a.H + (tr.r0 + tr.rt);
      if (k == 2) return a.total_out_rows;
      t = (unsigned)__builtin_amdgcn_readfirstlane((int)claim());
    }
  }
};

}  // namespace fdoct
