// fdoct_plan.h -- the kernel plan of a handle as a value: which kernel family a configuration takes and the geometry each
// family's launch needs (make_plan).  Plain C++ without HIP, so that a host program can check the planner's decisions without a
// GPU (tests/native/plan_check.cpp).
#pragma once
#include <cstddef>
#include <optional>
#include <string>
#include <vector>

#include "fdoct_wave_rules.h"

namespace fdoct {

constexpr int GENERIC_MAX_PASSES = 16;  // Stockham passes of one transform of the generic kernel (GenericArgs)
#ifndef GENERIC_MAX_RADIX
#define GENERIC_MAX_RADIX 8  // largest power-of-two butterfly of the generic kernel (8 or 16)
#endif

// One compiled plan of the fused kernel (fdoct_kernels.hip: FDOCT_PLANS).
struct FusedPlan {
  int id, nc, T, R1, R2, R3, WCH, kind;
};

int fused_plan_count();
bool fused_plan_get(int id, FusedPlan* p);

// What a plan is made from.
struct PlanInputs {
  int W = 0, M = 1, N = 0, D = 0;
  bool phase = false;          // a dispersion phase is set (complex rows)
  int plan_override = -1;      // fdoct_set_plan: -1 automatic, -2 the generic path, -3 rows in HBM, >= 0 that fused plan
  bool force_general = false;  // fdoct_set_plan: the fused kernel's any-option form (a launch choice: no decision here reads it)
};

// The zero-pad stage at full length inside generic_kernel: one +i DFT of length n, as Stockham passes of n or, for a length with
// a prime factor above 5, Bluestein around blu_m points (the radices are then those of blu_m).
struct GenericDftPlan {
  int n = 0, blu_m = 0;
  std::vector<int> rad;
};

// The any-configuration path: fdoct_generic.hip, or the long-row path (fdoct_big.hip) where the rows do not fit the LDS.
struct GenericPlan {
  std::vector<int> rad_n, rad_nh, rad_wh, rad_mwh, rad_blu;  // Stockham radices of N, N/2, W/2, M W/2 and blu_m
  int blu_m = 0;          // > 0: the final transform (N or N/2 points) has a prime factor > 5 and runs as Bluestein of this length
  bool zp_full = false;   // the zero-pad stage at full length (odd widths, half lengths with a prime factor above 5)
  int zn = 0;             // ... the padded spectrum's length, W + 2 floor((M W - W) / 2)
  GenericDftPlan gzf, gzi;  // ... its W-point and zn-point +i transforms
  bool inplace = false;   // ONE DFT buffer in LDS (rows whose two ping-pong buffers do not fit: generic_kernel<1024, 1, true>)
  bool radix16 = false;   // the pass plans hold radix-16 butterflies (the 1024-thread kernels)
  bool use_big = false;   // the long-row path
  // not FDOCT_OK: this path cannot take the configuration though a fused plan can; a call that needs this path fails with it
  int rc = 0;
  std::string why;
};

struct Plan {
  std::optional<FusedPlan> fused;  // none: the generic path runs every call
  bool cplx = false;               // complex rows (dispersion phase)
  int NC = 0;                      // points of the final transform: N, or N/2 for real rows
  int split = 0, scratch_bytes = 0, tw_count = 0;  // of the fused plan
  GenericPlan gen;                 // always made: a call the fused kernels cannot take (misaligned frames) runs on it
  WaveTwLayout wave_tw;            // the wave-per-row kernels' twiddle blob for this geometry (fdoct_wave_rules.h): its tables are filled and its LDS sized by it
};

// The plan for `in`: FDOCT_OK, or an error code with the reason in *why.  Reads nothing but its arguments and the measurement
// switches of the environment (FDOCT_NO_ZP_FULL, FDOCT_GENERIC_INPLACE_ABOVE, FDOCT_GENERIC_RADIX16, FDOCT_FORCE_LONG_ROWS),
// and writes *out only on success.
int make_plan(const PlanInputs& in, Plan* out, std::string* why);

// real rows run the N-point DFT as an N/2-point complex one (see generic_kernel)
inline bool generic_real_half(const PlanInputs& in) { return !in.phase && (in.N % 2) == 0; }
// length of each DFT buffer of generic_kernel
int generic_buffer_len(const PlanInputs& in, const GenericPlan& g);
// its LDS: the row, the DFT buffer(s) (buffers = 0: as many as the plan runs with), the magnitude sums
size_t generic_lds_bytes(const PlanInputs& in, const GenericPlan& g, int buffers = 0);

}  // namespace fdoct
