// fdoct_calibrate_kernels.h -- launchers of the calibration stage (fdoct_calibrate.hip) behind include/fdoct_calibrate.h: min / max
// and cv::normalize(NORM_MINMAX) on rows of doubles, the division by the frame count, BscanDark's composition.
// Internal: fdoct_calibrate.cpp is the only caller.  Everything enqueues only; nothing here allocates or synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include "fdoct_grid.h"

namespace fdoct {

// How the min / max of `groups` groups of samples is reduced.  A group is one row of W doubles (per_row) or the whole plane of
// `rows` rows (groups = 1); its samples are cut into runs of 2 doubles (16 bytes), cpr = ceil(W / 2) a row.  A TEAM of T
// neighbouring lanes (a power of two, 1 .. 64: no wider than a row has runs, so that rows shorter than a wave do not idle one)
// folds one SEGMENT of a group: runs seg * T + lane, + S * T, ...  S segments a group, so that few groups still fill the capped
// grid; more teams of work than the grid has are taken in a grid-stride loop.  Pass 2 folds a group's S partials with a team of T2
// lanes and turns them into the group's (scale, shift).  A function of (rows, W, per_row, num_cu) alone.
struct MinMaxShape {
  long long groups = 0, items = 0;  // items: runs per group
  int rows_per_group = 0, cpr = 0;
  int T = 1, S = 1, T2 = 1;
  int blocks = 0, blocks2 = 0;      // workgroups of the two passes, capped at 16 waves per CU
  size_t ws_doubles = 0;            // workspace: 2 * groups * S partials, then 2 * groups coefficients
  size_t coef_offset = 0;           // where the coefficients start, in doubles
};
MinMaxShape minmax_shape(int rows, int W, bool per_row, int num_cu);

// Pointer and pitch of rows of doubles; the pitch in bytes, a multiple of 8.
struct RowsF64 {
  const double* in = nullptr;
  double* out = nullptr;  // == in: in place
  size_t in_pitch = 0, out_pitch = 0;
  int rows = 0, W = 0;
};

// out = in * scale + shift per group, scale and shift from the group's min and max as fdoct_normalize_minmax forms them from
// lo and hi (multiply and add rounded separately, computed on the device by one thread a group).  Three launches: partials, fold
// and coefficients, apply.  ws holds minmax_shape(..).ws_doubles doubles.
hipError_t launch_normalize_minmax(const RowsF64& r, bool per_row, double lo, double hi, double* ws, int num_cu, hipStream_t st);

// out = in / divisor, an IEEE double division per sample.  One launch.
hipError_t launch_divide_rows(const RowsF64& r, double divisor, int num_cu, hipStream_t st);

// out[i] = (yr[i] - yd[i]) + (ys[i] - yd[i]), each operation rounded on its own (BscanDark.cpp:996); n packed doubles in
// 16-byte aligned arrays.  One launch.
hipError_t launch_compose(const double* yr, const double* ys, const double* yd, double* out, size_t n, int num_cu, hipStream_t st);

}  // namespace fdoct
