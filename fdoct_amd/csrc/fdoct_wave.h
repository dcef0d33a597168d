// fdoct_wave.h -- interface of the wave-per-row kernels (fdoct_wave.hip): the acquisition configurations the reference
// ships (build/*.ini: numfftpoints 2560 / 2880 / 640, zero-pad multiplier 4 or 1), one 64-lane wave per A-scan.  Their rules --
// plans, shapes, option bits, LDS sizes -- are fdoct_wave_rules.h's.
#pragma once
#ifndef __HIPCC_RTC__  // (device part also compiled at run time, fdoct_jit.cpp: no system headers there)
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif

#include "fdoct_wave_rules.h"

namespace fdoct {

struct WaveArgs {
  const void* frames;
  long long pitch_bytes;
  long long total_out_rows;
  int dtype;  // FDOCT_K_*
  int H, D, A;
  const float* ib;  // [W] or [H*W] 1/background
  const float* il;  // its low word, indexed like ib (fdoct_capi.cpp::reciprocal_words)
  int ib_2d;
  const float* win;      // [W] window
  const float* win_lo;   // [W] what the float window leaves of the double one (OPT & FDOCT_WAVE_OPT_BANDPASS: the row is formed in double)
  const float *yp_lo, *yd_lo;  // the same of the pi and dark frames (laid out like yp, yd)
  const float* g;        // [M*W] fractionalk by sample (0 past numfftpoints)
  const uint32_t* gidx;  // [N/2] packed float indices of the sources of data_ylin[2n] (low half) and [2n+1]; M*W = the zero slot
                         // (OPT & FDOCT_WAVE_OPT_CPLX: [N], the source of data_ylin[n] in the low half)
  const float2* tw;      // twiddle blob (wave_tw_layout, fdoct_wave_rules.h); offsets in float2 units below
  int tw_count;
  int off_nc, off_lh, off_wh;      // per-pass tables of the N/2-, M*W/2- and W/2-point transforms
  int off_tww, off_twmw, off_twn;  // exp(+2 pi i k/W), k < W/2; exp(+2 pi i k/(M W)), k < W/2; exp(+2 pi i k/N), k < D
  int dcmask;
  float inv_A, eps, db_scale;
  float* out_mag;
  float* out_db;
  const float* yp;  // [W] or [H*W], OPT & FDOCT_WAVE_OPT_PI
  const float* yd;  // [W] or [H*W], OPT & FDOCT_WAVE_OPT_DARK
  int yp_2d, yd_2d;
  const void* minmax;  // float2 (min, max) per input frame, OPT & FDOCT_WAVE_OPT_FRAMENORM
  const float2* phase;  // [N] (cos, sin), OPT & FDOCT_WAVE_OPT_CPLX
  unsigned long long* probe;  // measurement builds (-DFDOCT_WAVE_PROBE): cycles per phase of one wave; null otherwise
  float2* out_cx;  // [total_out_rows * D] (re, im), 8-byte aligned, OPT & FDOCT_WAVE_OPT_CXOUT (then out_mag / out_db are not written)
};

#ifndef __HIPCC_RTC__
hipError_t launch_wave(int W, int M, int N, const WaveArgs& a, int grid, int waves, size_t lds, hipStream_t st);
#endif  // !__HIPCC_RTC__

}  // namespace fdoct
