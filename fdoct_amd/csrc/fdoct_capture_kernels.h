// fdoct_capture_kernels.h -- launchers of the reference-frame capture (fdoct_capture.hip) behind include/fdoct_capture.h and
// of BscanDark's low-pass filter on captured frames (fdoct_lowpass.hip) behind include/fdoct_lowpass.h.
// Internal: fdoct_capture.cpp, fdoct_lowpass.cpp and fdoct_calibrate.cpp (whose captures start with the same accumulation) are the only callers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include "fdoct_grid.h"

namespace fdoct {

// nframes frames of H rows of W samples: row r of frame f starts pitch * (f * H + r) bytes after `frames`.  dt is an
// fdoct_dtype (u8, u16, f32, f64); `frames` and pitch are multiples of the sample size.
struct CaptureFrames {
  const void* frames = nullptr;
  int dt = 0;
  size_t pitch = 0;
  int nframes = 0, H = 0, W = 0;
};

// out[r * W + x] = sum over the frames, in frame order and in double, of sample (r, x) -- with movavgn > 0 of its
// smoothmovavg value (BscanFFT.cpp:276-294, in double, taps in the reference's order).  zero_start: the sum starts from
// 0.0 as cv::accumulate's does (a lone -0.0 comes out as +0.0); otherwise from the first frame's value (a copy).
// One launch; num_cu caps the grid.
hipError_t launch_capture_accumulate(const CaptureFrames& in, int movavgn, bool zero_start, double* out, int num_cu, hipStream_t st);

// Blocks per frame of the min / max reduction's first pass, and the doubles of workspace it needs (min and max per block).
int frame_minmax_blocks(const CaptureFrames& in, int num_cu);
inline size_t frame_minmax_partials(const CaptureFrames& in, int num_cu) { return 2 * (size_t)in.nframes * frame_minmax_blocks(in, num_cu); }
// out_min[f], out_max[f] = min / max of frame f as doubles (selections: exact).  Two launches: per-block partials, then one
// wave per frame folds them.
hipError_t launch_frame_minmax(const CaptureFrames& in, double* partials, double* out_min, double* out_max, int num_cu, hipStream_t st);

// lpfilter (BscanDark.cpp:119-167) on rows of W doubles, all in double.  What a launch looks like is a function of
// (rows, W, num_cu); of those only W decides the order of the sums.
struct LowpassShape {
  int f = 0;            // kept bins 0 .. f - 1, f = W / 10
  int G = 1, L = 0;     // slices per bin of the analysis and samples per slice
  bool staged = false;  // the row and its bins live in LDS (else: samples through the caches, bins in `ws`)
  size_t lds = 0;       // dynamic LDS bytes
  int blocks = 0;       // workgroups (one row at a time each), capped at 16 waves per CU
  size_t ws_doubles = 0;  // doubles of workspace the launch needs (0 when staged)
};
LowpassShape lowpass_shape(int rows, int W, int num_cu);
// out row r = filter(in row r); pitches in bytes, multiples of 8; in == out (same pitch) filters in place.  One launch.
hipError_t launch_lowpass_rows(const double* in, size_t in_pitch, double* out, size_t out_pitch, int rows, int W, double* ws,
                               int num_cu, hipStream_t st);

}  // namespace fdoct
