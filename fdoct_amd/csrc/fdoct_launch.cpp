// fdoct_launch.cpp -- make_fused_launch (fdoct_launch.h).  Plain C++ without HIP.
#include "fdoct_launch.h"

#include <algorithm>

#include "../../include/fdoct.h"

namespace fdoct {

// LDS bytes of a fused kernel's constants.  planes: the three constant planes are staged (kernels that do not keep them in
// registers); il_plane: so is the low word of the reciprocal background (FusedArgs::prec == 1); il_half: that plane holds half
// floats (fused_il_half); tw3 / gi: the step-5 twiddle table and the gather table are staged (the transposed-store kernels leave
// out what they hold in registers: fused_tw3_in_lds / fused_gi_in_lds)
static size_t const_lds_bytes(const Plan& pl, bool planes, bool il_plane, bool il_half, bool tw3 = true, bool gi = true) {
  const int WC = 8 * pl.fused->T * pl.fused->WCH;
  const size_t tw_entries = tw3 ? (size_t)pl.tw_count : (size_t)(pl.fused->R2 - 1) * pl.fused->R1;
  return (planes ? (size_t)3 : 0) * WC * 4 + (il_plane ? (size_t)WC * (il_half ? 2 : 4) : 0) + tw_entries * 8 + (pl.cplx ? (size_t)pl.NC * 8 : 0) + (gi ? (size_t)pl.NC * 4 : 0);
}

// constants of a transposed-store launch (fast path)
static size_t tro_const_lds_bytes(const Plan& pl, const FusedLaunchInputs& in) {
  const FusedPlan& p = *pl.fused;
  const bool both = in.precise_div, ib2d = in.bg_rows > 1, half = fused_il_half(true, p.WCH);
  // (the row-swap plan's transposed-store kernels hold the constant planes in registers; the 512-point Stockham plan's read them
  // from LDS like its row-major kernels, and its averaging kernels take the low words from global memory: fused_il_global)
  const bool planes = !fused_resident_consts(p.kind, true, in.A > 1, p.WCH, 0);
  const bool il_plane = both && !ib2d && !fused_il_global(true, in.A > 1, p.WCH, p.T);
  return const_lds_bytes(pl, planes, il_plane, half, fused_tw3_in_lds(p.kind, true, 0, true, ib2d && both && half),
                         fused_gi_in_lds(p.kind, true, 0, false, in.A > 1, true));
}

// Can the chain write the reference's D x H layout itself (fused_kernel's TRO instantiations), as far as handle and geometry say?
// The acquisition configurations on the plans that have them compiled: 8/16-bit frames, 1-row or full-frame background, none
// or the whole-frame normalisation, rows in fours and depth bins in whole write-out steps.
static bool tro_configured(const Plan& pl, const FusedLaunchInputs& in) {
  if (!in.want_tro || in.staged || in.force_general || pl.cplx) return false;
  const FusedPlan& p = *pl.fused;
  if (!fused_tro_compiled(p.kind, p.T, p.WCH)) return false;
  if (in.kdt != FDOCT_K_U8 && in.kdt != FDOCT_K_U16) return false;
  if (in.W != 8 * p.T * p.WCH || in.pi || in.dark || in.rowwisenormalize) return false;
  if ((in.minmax || in.bg_rows > 1) && in.A != 1) return false;  // (those instantiations exist for one frame per B-scan)
  if (p.kind != 1 && (in.minmax || in.bg_rows > 1)) return false;  // (... and for the row-swap plan only: the 512-point plan has the plain and the averaging kernel)
  if ((in.H % 4) || (in.D % fused_tro_step_bins(64 / p.T)) || in.D > pl.NC) return false;
  // (both words: a full-frame background brings its second word along with the prefetched row -- no LDS plane; a 1-row one needs
  // the plane next to the ring, which then holds one computing wave less)
  if (in.precise_div && in.bg_rows > 1 && !fused_il_half(true, p.WCH)) return false;
  // (four rows per wave: a launch override must leave whole groups of waves)
  if (64 / p.T == 4 && in.block_override && in.block_override / 64 < fused_tro_group_waves()) return false;
  return true;
}

// The transposed store's launch (block, LDS, grid, ring and tiles into *l), or none where no group of waves / no ring fits the
// LDS, which holds the constants, one row buffer per wave and the ring of finished rows (every wave computes; they share the write-out).  As
// many waves as the register budget allows, then the largest ring that fits (round 5: the store is bound by how much
// of the next tile fits into the ring while a tile drains, so the kernel keeps its once-read tables out of LDS); a wave is given
// up only where not even the smallest ring fits next to them.
static void tro_launch(const Plan& pl, const FusedLaunchInputs& in, int max_waves, size_t lds_max, FusedLaunch* l) {
  const FusedPlan& p = *pl.fused;
  const int rpw = 64 / p.T;
  const size_t tro_const = tro_const_lds_bytes(pl, in), per_wave = (size_t)pl.scratch_bytes * rpw;
  int cw = max_waves;
  if (in.block_override && in.block_override / 64 >= 1 && in.block_override / 64 < cw) cw = in.block_override / 64;
  FusedTroLaunch t;
  if (rpw == 4) {
    // whole groups of four waves, as many as registers and LDS allow; no ring (the rows wait in the waves' own buffers)
    constexpr int GW = fused_tro_group_waves();
    while (cw >= GW && tro_const + cw * per_wave > lds_max) cw--;
    cw = cw / GW * GW;
    if (cw < GW) return;
  } else {
    const size_t cap = in.ring_cap >= 20 ? (size_t)in.ring_cap * (size_t)(in.D + 4) * 4 : lds_max;  // (measurement: at most this many slots)
    for (;; cw--) {
      if (cw < 1) return;
      const size_t used = tro_const + cw * per_wave;
      if (used < lds_max && (t.ring = fused_tro_ring_pick(std::min(lds_max - used, cap), in.D, rpw))) break;
    }
  }
  l->block = cw * 64;
  l->lds = tro_const + cw * per_wave + (size_t)t.ring * (size_t)(in.D + 4) * 4;
  const unsigned tile_rows = (unsigned)fused_tro_tile_rows(rpw);
  t.tpf = (unsigned)((in.H + tile_rows - 1) / tile_rows);
  t.tpf_magic = t.tpf > 1 ? (unsigned)((1ull << 32) / t.tpf) : 0xffffffffu;
  const long long tiles = in.groups * t.tpf;
  t.total_tiles = (unsigned)tiles;
  l->grid = in.grid_override > 0 ? in.grid_override : in.num_cu;   // one workgroup per CU (the ring fills its LDS)
  if (l->grid > tiles) l->grid = tiles;
  l->tro = t;
}

int make_fused_launch(const Plan& pl, const FusedLaunchInputs& in, FusedLaunch* out, std::string* why) {
  const FusedPlan& p = *pl.fused;
  const int A = in.A;
  FusedLaunch l;
  // the unpredicated fast-path kernel applies to the plain acquisition configuration
  // (a full-frame background keeps the fast path on the row-swap plan: its resident registers prefetch the frame row)
  const bool fast_opts = fused_resident_consts(p.kind, true, A > 1, p.WCH, 0) && in.out_rows < 0x7fffffffLL && !in.staged;
  // (a full-frame background with the two-word reciprocal -- fdoct_set_precise_division -- runs on the any-option
  // kernel: the fast path's prefetch registers hold one word per sample)
  const bool bg_ok = in.bg_rows == 1 || (fast_opts && (!in.precise_div || fused_il_half(true, p.WCH)));
  const bool norm_ok = !in.minmax || fast_opts;  // whole-frame normalisation has a fast-path variant there too
  const bool lean = (in.kdt == FDOCT_K_U16 || in.kdt == FDOCT_K_U8) && in.W == 8 * p.T * p.WCH && bg_ok && !in.pi && !in.dark &&
                    (!in.rowwisenormalize || fast_opts) && norm_ok && !in.force_general;
  l.lean = lean;
  // launch geometry: as many waves per workgroup as LDS and the register budget allow
  const int rpw = 64 / p.T;
  l.lds_planes = fused_resident_consts(p.kind, lean, A > 1, p.WCH, 0) ? 0 : 1;
  // 1/background as two floats (reciprocal_words): always on the any-option kernel, by fdoct_set_precise_division on the fast path
  l.prec = (lean && !in.precise_div) ? 0 : (in.bg_rows == 1 ? 1 : 2);
  // (the averaging fast-path kernels that keep their planes in LDS are bound by its capacity: a fourth 4 W-byte plane would cost
  // C4 a wave per CU, so they read the low words from global memory instead)
  // (only the kernels with more than 32 samples per lane have that form -- a compile-time property, fused_il_global: the others
  // read the row's low words at its top from the LDS plane, resident constants or not -- fused_kernel's ILX)
  // (staged mode: the kernel that reads the samples is the resample stage, compiled WITHOUT averaging whatever A is -- it runs
  // over input A-scans -- so it takes its low words from the LDS plane like every non-averaging kernel)
  if (l.prec == 1 && fused_il_global(lean, A > 1 && !in.staged, p.WCH, p.T)) l.prec = 3;
  const size_t lds_const = const_lds_bytes(pl, l.lds_planes != 0, l.prec == 1, fused_il_half(lean, p.WCH));
  const size_t lds_max = 160 * 1024 - 64;  // the kernel's static row-ticket counter lives in LDS too
  const int max_block = fused_max_block(pl.NC, p.T, lean, p.kind);
  const int max_waves = max_block / 64;
  FusedLaunch tro;  // (its block, LDS and grid replace the row-major launch's below)
  if (lean && tro_configured(pl, in)) tro_launch(pl, in, max_waves, lds_max, &tro);
  // (a full-frame background with both words: every wave has a slot for the prefetched pattern row of its next A-scan)
  const size_t dma_per_wave = fused_il16_dma_bytes(lean && in.bg_rows > 1, l.prec == 2 && fused_il_half(lean, p.WCH), tro.tro.has_value(), 8 * p.T * p.WCH);
  const size_t per_wave = (size_t)pl.scratch_bytes * rpw + dma_per_wave;
  int waves = (int)((lds_max - lds_const) / per_wave);
  if (waves > max_waves) waves = max_waves;
  if (in.block_override) {
    int w = in.block_override / 64;
    if (w >= 1 && w <= waves) waves = w;
  }
  if (waves < 1) return *why = "row does not fit in LDS", FDOCT_ERR_UNSUPPORTED;
  if (in.staged && (!lean || in.kdt != FDOCT_K_U16))
    return *why = "staged mode is built for the plain u16 acquisition configuration only", FDOCT_ERR_UNSUPPORTED;
  l.block = waves * 64;
  l.lds = lds_const + (size_t)waves * per_wave;
  const int blocks_per_cu = (int)(lds_max / l.lds) > 0 ? (int)(lds_max / l.lds) : 1;
  const int wave_cap = (max_block / 64) / waves;  // register budget: max_block threads per CU
  int bpc = blocks_per_cu < wave_cap ? blocks_per_cu : wave_cap;
  if (bpc < 1) bpc = 1;
  // (staged mode: the resample stage runs over the input A-scans as they lie, the FFT stage over the output A-scans)
  auto grid_for = [&](long long rows) {
    const long long need = (rows + (long long)waves * rpw - 1) / ((long long)waves * rpw);
    const long long grid = in.grid_override > 0 ? in.grid_override : (long long)in.num_cu * bpc;
    return grid > need ? need : grid;
  };
  l.grid = std::max(grid_for(in.out_rows), 1LL);
  if (in.staged) l.stage1_grid = grid_for(in.in_rows);
  if (tro.tro) l.block = tro.block, l.lds = tro.lds, l.grid = tro.grid, l.tro = tro.tro;
  *out = l;
  return FDOCT_OK;
}

}  // namespace fdoct
