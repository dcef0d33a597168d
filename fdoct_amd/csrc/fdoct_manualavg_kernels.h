// fdoct_manualavg_kernels.h -- the manual averaging's kernel (fdoct_manualavg.hip) behind include/fdoct_manualavg.h: its argument
// block, the schedule of a call's emissions and the host-side sizing of its launch.  Internal: fdoct_manualavg.cpp is the only caller.
#pragma once
#include <hip/hip_runtime.h>

#include "fdoct_grid.h"

namespace fdoct {

// One call as the kernel sees it.  Image i of the call (0 <= i < nb) is an emission position when i == first + k * period; with
// `drop` (the reference's mode) the image at such a position is not added and the emission comes instead of it, without it the
// image is added first.  The same for every element, so every branch on it is uniform across the launch.
struct ManualAvgArgs {
  const float* in = nullptr;    // nb images of `count` floats, packed
  double* acc = nullptr;        // `count` running sums
  float* out_mean = nullptr;    // either may be null; slot e starts at e * count
  float* out_db = nullptr;
  long long count = 0;
  int nb = 0, m = 1;
  int drop = 1, first = 0, period = 2;
  // decided by manualavg_plan_launch
  int vec = 0;                  // 16-byte loads and stores on whole groups of four elements; the rest (or everything) one by one
  int blocks = 0;
};

// The emission positions of a call that starts with `accumulated` images in (0..m): *first and *period as above.  Reference
// mode (main:1401-1444): the image that finds m in; keep-all: the image that makes m.
inline void manualavg_schedule(int m, bool reference, int accumulated, int* first, int* period) {
  *period = reference ? m + 1 : m;
  *first = reference ? m - accumulated : (accumulated >= m ? 0 : m - 1 - accumulated);
}
// ... how many of nb images are such positions, and the counter after them.
inline int manualavg_emissions(int first, int period, int nb) { return nb > first ? (nb - 1 - first) / period + 1 : 0; }
inline int manualavg_counter_after(int first, int period, int accumulated, int nb) {
  const int e = manualavg_emissions(first, period, nb);
  return e ? nb - 1 - (first + (e - 1) * period) : accumulated + nb;
}

// Fills vec and blocks from the others (pointers enter through their alignment).  Nothing is enqueued.
void manualavg_plan_launch(ManualAvgArgs* a, int num_cu);
hipError_t launch_manualavg(const ManualAvgArgs& a, hipStream_t st);

}  // namespace fdoct
