// fdoct_doppler_kernels.h -- the device side of include/fdoct_doppler.h (fdoct_doppler.hip): the argument block of the two
// kernels, the pair images' shape as a plain function (fdoct_doppler.cpp refuses with it before anything is enqueued), the launch
// fields through fdoct_boxtile.h's tile geometry, and the launchers.  Internal: fdoct_doppler.cpp is the only caller.
#pragma once
#include <hip/hip_runtime.h>

#include "fdoct_boxtile.h"

namespace fdoct {

constexpr int kDopMaxWin = 32;        // window sizes 1..32 on both axes
constexpr int kDopPlanes = 3;         // the tile's planes: T re, T im, |X1|^2 + |X2|^2

// One call as the kernels see it.
struct DopplerArgs {
  const float2* x = nullptr;     // nframes x ascans x depths pairs, row-major
  float2* bulk = nullptr;        // pair_images x pair_rows phasors B / |B| (use_bulk), written by the first kernel and read by the second
  float* out_phase = nullptr;    // any may be null
  float2* out_corr = nullptr;
  float* out_power = nullptr;
  int ascans = 0, depths = 0;
  int pair_images = 0, pair_rows = 0;
  long long partner = 0;         // X2 lies `partner` pairs behind X1: lag * depths (A-scans) or lag * ascans * depths (frames)
  int wa = 1, wd = 1;
  int use_bulk = 0, bulk_first = 0, bulk_count = 0;   // bulk_count resolved: > 0 with use_bulk
  float scale = 1.f, min_power = 0.f;
  // decided by doppler_plan_launch
  int tiles_r = 0, tiles_d = 0;
  long long tiles = 0;
  int blocks = 0, bulk_blocks = 0;
  unsigned lds_bytes = 0;
};

// The pair images of nframes x ascans: false where the lag leaves none.  axis 0: A-scans, 1: frames.
inline bool doppler_pairs(int axis, int lag, int nframes, int ascans, int* pair_images, int* pair_rows) {
  if (lag < 1 || nframes < 1 || ascans < 1) return false;
  const long long pi = axis ? (long long)nframes - lag : nframes, pr = axis ? ascans : (long long)ascans - lag;
  if (pi < 1 || pr < 1) return false;
  *pair_images = (int)pi, *pair_rows = (int)pr;
  return true;
}

// Fills the launch fields from the others.  Nothing is enqueued.
inline void doppler_plan_launch(DopplerArgs* a, int num_cu) {
  box_plan_launch(a, kDopPlanes, a->pair_images, a->pair_rows, (long long)a->pair_images * a->pair_rows, num_cu);
}

// The bulk sums (a.use_bulk) and the stage, in that order on `st`.
hipError_t launch_doppler(const DopplerArgs& a, hipStream_t st);

}  // namespace fdoct
