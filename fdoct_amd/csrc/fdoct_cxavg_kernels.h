// fdoct_cxavg_kernels.h -- the device side of include/fdoct_cxavg.h (fdoct_cxavg.hip): the argument block of the three kernels, its
// launch fields (fdoct_cxavg.cpp decides them before anything is enqueued), and the launcher.  Internal: fdoct_cxavg.cpp is the
// only caller.
#pragma once
#include <hip/hip_runtime.h>

#include "fdoct_boxtile.h"

namespace fdoct {

constexpr int kCxaMinRepeats = 2, kCxaMaxRepeats = 64;
constexpr int kCxaMaxFrames = 65536;
constexpr long long kCxaMaxPixels = 1LL << 24;
constexpr int kCxaBlock = 256;          // one workgroup per (group, A-scan)
constexpr int kCxaWavesPerCu = 16;      // the grids' cap: four workgroups a CU
constexpr int kCxaRegPairs = 16;        // pairs a thread keeps in the register form: 65 .. 82 VGPRs, no scratch
constexpr int kCxaFormRegister = 1, kCxaFormStreaming = 2;
constexpr int kCxaAlignNone = 0, kCxaAlignRow = 1, kCxaAlignFrame = 2;

// One call as the kernels see it.
struct CxavgArgs {
  const float2* x = nullptr;     // nframes x ascans x depths pairs, row-major; group g's repeat n is frame g stride + n
  float2* rows = nullptr;        // align 2: groups x repeats x ascans sums C[g][n][r] (the ref's are never written nor read)
  float2* phasors = nullptr;     // align 2: groups x repeats phasors U[g][n]
  float2* out_mean = nullptr;    // any may be null
  float* out_mag = nullptr;
  float* out_incoh = nullptr;
  float* out_coh = nullptr;
  int groups = 0, repeats = 0, stride = 0, ref = 0, ascans = 0, depths = 0;
  int align = 0, first = 0, count = 0;   // count resolved: > 0 with align 1 and 2.  align is dropped where only out_incoh is asked for
  // decided by cxavg_plan_launch
  int form = 0;                  // kCxaFormRegister or kCxaFormStreaming
  int slots = 0;                 // register form: the kernel's instantiation, repeats rounded up to 2, 4, 8 or 16
  int blocks = 0, row_blocks = 0, phasor_blocks = 0;
};

// The register form's instantiations are <NR, 16 / NR>, NR = 2, 4, 8, 16: NR repeats of 256 (16 / NR) depths at most.  A call takes
// the smallest NR that holds its repeats, and the form if its depths fit as well: 0 where they do not.
inline int cxavg_register_slots(int repeats, int depths) {
  int nr = 2;
  while (nr < repeats) nr *= 2;
  return nr <= kCxaRegPairs && (long long)nr * ((depths + kCxaBlock - 1) / kCxaBlock) <= kCxaRegPairs ? nr : 0;
}

// Fills the launch fields from the others.  Nothing is enqueued.
inline void cxavg_plan_launch(CxavgArgs* a, int num_cu) {
  a->slots = cxavg_register_slots(a->repeats, a->depths);
  a->form = a->slots ? kCxaFormRegister : kCxaFormStreaming;
  const long long cap = resident_blocks(num_cu, kCxaWavesPerCu, kCxaBlock);
  const long long items = (long long)a->groups * a->ascans;
  a->blocks = (int)(items < cap ? items : cap);
  const long long rows = items * a->repeats, per_group = (long long)a->groups * a->repeats;
  const long long row_cap = resident_blocks(num_cu, kBoxWavesPerCu, kBoxBulkBlock);
  a->row_blocks = a->align == kCxaAlignFrame ? (int)(rows < row_cap ? rows : row_cap) : 0;
  a->phasor_blocks = a->align == kCxaAlignFrame ? (int)((per_group + kCxaBlock - 1) / kCxaBlock) : 0;
}

// The per-row sums and the phasors (a.align == 2), then the stage, in that order on `st`.
hipError_t launch_cxavg(const CxavgArgs& a, hipStream_t st);

}  // namespace fdoct
