// fdoct_enface_kernels.h -- the device side of include/fdoct_enface.h (fdoct_enface.hip): the argument block of the two kernels,
// its launch fields (fdoct_enface.cpp decides them before anything is enqueued), and the launcher.  Internal: fdoct_enface.cpp is
// the only caller.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "fdoct_grid.h"

namespace fdoct {

constexpr int kEnfMaxSlabs = 8, kEnfMaxSmooth = 16, kEnfMaxMedian = 15;
constexpr int kEnfMaxPositions = 65536;
constexpr long long kEnfMaxPixels = 1LL << 24;   // ascans x depths
constexpr int kEnfBlock = 256;                   // four wavefronts, one A-scan each
constexpr int kEnfWavesPerCu = 32;               // the cap of both grids: 8 workgroups a compute unit
constexpr int kEnfChunk = 256;                   // depths a wavefront takes per step: 4 consecutive ones a lane

// One call as the kernels see it.
struct EnfaceArgs {
  const float* vol = nullptr;        // positions x ascans x depths, row-major
  const float* structure = nullptr;  // what the surface kernel reads: the structure volume, or vol
  int32_t* z0 = nullptr;             // positions x ascans raw surfaces (surface != 0): the first kernel writes, the second reads
  float* out_mean = nullptr;         // any may be null
  float* out_max = nullptr;
  int32_t* out_argmax = nullptr;
  int32_t* out_surface = nullptr;
  int positions = 0, ascans = 0, depths = 0;
  int surface = 0, s0 = 0, s1 = 0, smooth = 1, median = 1;   // [s0, s1): the search range, resolved
  float threshold = 0.f;
  int nslabs = 0;
  int first[kEnfMaxSlabs] = {}, count[kEnfMaxSlabs] = {};    // count clamped to 2 x depths: what lies beyond is clipped anyway
  // decided by enface_plan_launch
  long long rows = 0;                // positions x ascans
  int blocks = 0;
};

// Fills the launch fields from the others.  Nothing is enqueued.
inline void enface_plan_launch(EnfaceArgs* a, int num_cu) {
  a->rows = (long long)a->positions * a->ascans;
  const int waves = kEnfBlock / 64;
  a->blocks = (int)std::min<long long>((a->rows + waves - 1) / waves, resident_blocks(num_cu, kEnfWavesPerCu, kEnfBlock));
}

// The surface kernel (a.surface != 0) and the projection, in that order on `st`.
hipError_t launch_enface(const EnfaceArgs& a, hipStream_t st);

}  // namespace fdoct
