// fdoct_angio_kernels.h -- the device side of include/fdoct_angio.h (fdoct_angio.hip): the argument block of the two kernels, its
// launch fields through fdoct_boxtile.h's tile geometry (fdoct_angio.cpp decides them before anything is enqueued), and the
// launcher.  Internal: fdoct_angio.cpp is the only caller.
#pragma once
#include <hip/hip_runtime.h>

#include "fdoct_boxtile.h"

namespace fdoct {

constexpr int kAngMaxWin = 16;          // window sizes 1..16 on both axes: what keeps a thread's staged pixels at 10 (below)
constexpr int kAngMinRepeats = 2, kAngMaxRepeats = 64;
constexpr int kAngMaxFrames = 65536;
constexpr long long kAngMaxPixels = 1LL << 24;
constexpr int kAngPlanes = 2;           // the tile's planes: what one window pass sums
// Staged pixels a thread keeps in registers: ceil((16 + wa - 1) (64 + wd - 1) / 256), rounded up to one of the kernel's three
// instantiations -- 4: the 1 x 1 window; 6: up to 22 x 69 staged, the 5 x 5 and 7 x 6 windows; 10: up to 31 x 79, the 16 x 16 window.
constexpr int kAngKeepSmall = 4, kAngKeepMid = 6, kAngKeepLarge = 10;

// One call as the kernels see it.
struct AngioArgs {
  const float2* x = nullptr;     // groups x repeats x ascans x depths pairs, row-major
  float2* bulk = nullptr;        // groups x (repeats - 1) x ascans phasors conj(B) / |B| (use_bulk): the first kernel writes, the second reads
  float* out_var = nullptr;      // any may be null
  float* out_decorr = nullptr;
  float* out_cdecorr = nullptr;
  float* out_power = nullptr;
  int groups = 0, repeats = 0, ascans = 0, depths = 0;
  int wa = 1, wd = 1;
  int use_bulk = 0, bulk_first = 0, bulk_count = 0;   // bulk_count resolved: > 0 with use_bulk.  use_bulk is dropped with out_cdecorr
  float min_power = 0.f;
  // decided by angio_plan_launch
  int tiles_r = 0, tiles_d = 0;
  long long tiles = 0;
  int keep = 0;                  // kAngKeepSmall, kAngKeepMid or kAngKeepLarge
  int blocks = 0, bulk_blocks = 0;
  unsigned lds_bytes = 0;
};

// Fills the launch fields from the others.  Nothing is enqueued.
inline void angio_plan_launch(AngioArgs* a, int num_cu) {
  box_plan_launch(a, kAngPlanes, a->groups, a->ascans, (long long)a->groups * (a->repeats - 1) * a->ascans, num_cu);
  const int staged = box_staged_rows(a->wa) * box_staged_depths(a->wd);
  a->keep = staged <= kAngKeepSmall * kBoxBlock ? kAngKeepSmall : staged <= kAngKeepMid * kBoxBlock ? kAngKeepMid : kAngKeepLarge;
}

// The bulk sums (a.use_bulk) and the stage, in that order on `st`.
hipError_t launch_angio(const AngioArgs& a, hipStream_t st);

}  // namespace fdoct
