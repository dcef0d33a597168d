// fdoct_launch.h -- the launch of the fused kernel family as a value: which instantiation a call takes (fast path or any-option,
// how the second reciprocal word is applied, which planes go to LDS) and its geometry (block, dynamic LDS, grid; the stage-1 grid
// of staged mode; ring and tiles of the transposed store), made from the handle's plan and what the decision reads of handle and
// call (make_fused_launch).  Plain C++ without HIP, like the planner: tests/native/launch_check.cpp pins it without a GPU.
#pragma once
#include <optional>
#include <string>

#include "fdoct_fused_rules.h"
#include "fdoct_plan.h"

namespace fdoct {

struct FusedLaunchInputs {
  int W = 0, H = 0, D = 0, A = 1;
  int kdt = FDOCT_K_U16;       // sample type the kernel reads (FDOCT_K_*)
  int bg_rows = 1;             // background: one spectrum, or a full frame of H rows
  bool pi = false, dark = false, rowwisenormalize = false;
  bool minmax = false;         // the whole-frame normalisation's min / max pass runs
  bool frames_lo = false;      // the samples come with a plane of low words (frames handed over as doubles)
  bool precise_div = true, staged = false, force_general = false;
  int block_override = 0, grid_override = 0, num_cu = 256;
  long long in_rows = 0, out_rows = 0, groups = 0;  // input A-scans, output A-scans, B-scans
  bool want_tro = false;       // the call asks for D x H and nothing about it (alignment, passes in front) rules the chain's own store out
  unsigned ring_cap = 0;       // FDOCT_TRO_RING (measurement: at most this many ring slots; 0: no cap)
};

struct FusedTroLaunch {
  unsigned ring = 0;           // FusedArgs::tr_ring (0: four rows per wave, the tiles wait in the waves' own buffers)
  unsigned tpf = 0, tpf_magic = 0, total_tiles = 0;
};

struct FusedLaunch {
  bool lean = false;           // the unpredicated fast-path kernel
  int prec = 0, lds_planes = 0;  // FusedArgs::prec, FusedArgs::lds_planes
  int block = 0;               // threads per workgroup ...
  size_t lds = 0;              // ... its dynamic LDS ...
  long long grid = 0;          // ... and workgroups of the chain's launch (staged mode: of the FFT stage)
  long long stage1_grid = 0;   // staged mode: workgroups of the resample stage (same block and LDS)
  std::optional<FusedTroLaunch> tro;  // the chain writes D x H itself; none: it does not apply to this configuration
};

// The launch for a plan with a fused kernel: FDOCT_OK, or an error code with the reason in *why (*out is then untouched).  Reads
// nothing but its arguments.
int make_fused_launch(const Plan& pl, const FusedLaunchInputs& in, FusedLaunch* out, std::string* why);

}  // namespace fdoct
