// fdoct_colour_kernels.h -- launcher of the colour front end (fdoct_colour.hip) behind include/fdoct_colour.h: the webcam's
// interleaved B,G,R frames to one channel or to the scaled sum, with the binning in the same pass.
// Internal: run_colour (fdoct_route.cpp) is the only caller.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace fdoct {

// (double(B) + double(G) + double(R)) * this, BscanFFTwebcam.cpp:1031 -- the literal the reference writes, not 1 / 765
constexpr double kColourSumScale = 0.00130718954;

// One call.  The input is out_rows * biny rows of ow * binx pixels of 3 bytes, row r starting r * pitch bytes after `bgr`
// (frames follow each other without a gap in rows: out_rows = nframes * oh).  channelnum 0 / 1 / 2: `out` takes bytes, the
// binned channel in the front end's arithmetic (bin_kernel, fdoct_generic.hip).  channelnum 3: `out` takes doubles, the block
// sum of (B + G + R) * kColourSumScale in double, rows outermost and left to right, times (double)(1.f / area).
// `out` is 16-byte aligned and out_pitch a multiple of 16 (a library workspace); `bgr` and pitch are any.
struct ColourArgs {
  const unsigned char* bgr = nullptr;
  long long pitch = 0;
  void* out = nullptr;
  long long out_pitch = 0;
  long long out_rows = 0;
  int ow = 0;
  int binx = 1, biny = 1;
  int channelnum = 0;
};

// True when the call's whole 16-pixel groups go through the kernel of 16-byte loads (aligned rows, binx 1, 2 or 4); the rest
// of each row, and every other call, goes pixel by pixel.  The result does not depend on it.
bool colour_vectorised(const ColourArgs& a);
// One launch, or two when a vectorised call's width leaves a tail.
hipError_t launch_colour(const ColourArgs& a, hipStream_t st);

}  // namespace fdoct
