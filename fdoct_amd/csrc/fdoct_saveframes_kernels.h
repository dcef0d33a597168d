// fdoct_saveframes_kernels.h -- the kernels (fdoct_saveframes.hip) behind include/fdoct_saveframes.h: the argument block of a call,
// the host-side sizing of its launches and the size of its scratch.  Internal: fdoct_saveframes.cpp is the only caller.
#pragma once
#include <hip/hip_runtime.h>

#include "fdoct_grid.h"

namespace fdoct {

// One call as the kernels see it.  An image is `count` = depths * ascans floats; element e of it is (ascan e / depths, depth
// e % depths) in the H x D layout and (depth e / ascans, ascan e % ascans) in the D x H one.
struct SaveFramesArgs {
  const float* in = nullptr;        // nframes images, packed
  unsigned char* gray = nullptr;    // nframes pictures of depths x ascans bytes, or null
  float* out_bscan = nullptr;       // nframes / group images each, or null (both null: no fold)
  float* out_db = nullptr;
  double* part = nullptr;           // gray: (min, max) of d per image and part, saveframes_part_doubles() of them
  long long count = 0;
  int nframes = 0, depths = 0, ascans = 0;
  int group = 1;                    // frames per fold group (1 without a fold)
  int in_transposed = 0, out_transposed = 0, dc_mask = 0;
  double eps = 1e-5;
  // decided by saveframes_plan_launch
  int vec = 0;                      // the scan reads 16 bytes per lane
  int parts = 0, scan_groups = 0;   // the scan's grid: x (= partial extrema per image), y
  int map_blocks = 0;               // the picture pass's grid
};

// Fills the launch fields from the others (pointers enter through their alignment).  Nothing is enqueued.
void saveframes_plan_launch(SaveFramesArgs* a, int num_cu);
// Doubles of scratch a call with pictures needs (after saveframes_plan_launch).
inline size_t saveframes_part_doubles(const SaveFramesArgs& a) { return (size_t)a.nframes * a.parts * 2; }
// The scan (fold + partial extrema), then, with pictures, the pass that writes them.
hipError_t launch_saveframes(const SaveFramesArgs& a, hipStream_t st);

}  // namespace fdoct
