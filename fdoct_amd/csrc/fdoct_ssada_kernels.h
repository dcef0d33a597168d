// fdoct_ssada_kernels.h -- the device side of include/fdoct_ssada.h (fdoct_ssada.hip): the argument block of the three kernels, the
// call's geometry as plain functions (fdoct_ssada.cpp refuses and plans with them before anything is enqueued), and the
// launchers.  The window stage between the split and the mean is fdoct_angio_kernels.h's launch_angio.  Internal: fdoct_ssada.cpp is
// the only caller.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>

#include "fdoct_grid.h"
#include "fdoct_lds_fft.h"

namespace fdoct {

constexpr int kSsaBlock = 256;             // threads of every kernel here
constexpr int kSsaMinN = 16, kSsaMaxN = 4096;
constexpr int kSsaMinRepeats = 2, kSsaMaxRepeats = 64;
constexpr int kSsaMaxBands = 16;
constexpr int kSsaMaxWin = 16;
constexpr int kSsaMaxBandFrames = 65536;   // nframes x bands: the window stage's frames
constexpr long long kSsaMaxPixels = 1LL << 24;
constexpr int kSsaWavesPerCu = 32;         // the grids' cap: eight workgroups a compute unit
constexpr size_t kSsaDefaultWorkspace = (size_t)2 << 30;

// One pass of a call as the kernels see it: `groups` whole groups of the call.
struct SsadaArgs {
  const float2* x = nullptr;     // groups x repeats x ascans x n pairs, row-major: the pass's first frame
  float2* bands = nullptr;       // groups x bands x repeats x ascans x depth_count pairs: the split kernel writes
  const float* band_decorr = nullptr;   // groups x bands x ascans x depth_count: the window stage's out_decorr, the mean reads (null: no out_decorr)
  const float* band_power = nullptr;    // likewise its out_power (null: neither out_power nor a mask)
  float* out_decorr = nullptr;   // groups x ascans x depth_count; either may be null
  float* out_power = nullptr;
  int groups = 0, repeats = 0, ascans = 0, nbands = 0;
  int depth_first = 0, depth_count = 0;   // depth_count resolved: >= 1
  int k_first = 0, k_count = 0;           // k_count resolved: >= 1
  double sigma = 0;
  float min_power = 0.f;
  // decided by ssada_plan_launch
  int per_wg = 0, chunks = 0;    // bands a workgroup takes, and the chunks of an A-scan
  long long items = 0;           // groups x repeats x ascans x chunks
  int blocks = 0, mean_blocks = 0;
  unsigned lds_bytes = 0;
  LdsFftPlan fft;
  // device memory: n twiddles e^(+2 pi i m / n), and behind them bands x n floats G_m(q)
  float2* tw = nullptr;
  float* gauss = nullptr;
};

inline size_t ssada_tab_bytes(int n, int bands) { return (size_t)n * sizeof(float2) + (size_t)bands * (size_t)n * sizeof(float); }

// One workgroup's LDS: the spectrum and the transform's two buffers.
inline unsigned ssada_lds_bytes(int n) { return 3u * (unsigned)n * (unsigned)sizeof(float2); }

// Bands per workgroup (include/fdoct_ssada.h states the rule: all of them).  FDOCT_SSADA_CHUNK: a measurement switch, the chunk
// itself (tools/ssada_rate.py sweeps it).
inline int ssada_chunk(int bands) {
  static const int forced = [] { const char* e = std::getenv("FDOCT_SSADA_CHUNK"); return e ? std::atoi(e) : 0; }();
  return forced > 0 && forced < bands ? forced : bands;
}

// Fills the launch fields from the others.  Nothing is enqueued.
inline void ssada_plan_launch(SsadaArgs* a, int num_cu) {
  a->per_wg = ssada_chunk(a->nbands);
  a->chunks = (a->nbands + a->per_wg - 1) / a->per_wg;
  a->items = (long long)a->groups * a->repeats * a->ascans * a->chunks;
  a->lds_bytes = ssada_lds_bytes(a->fft.n);
  const long long cap = resident_blocks(num_cu, kSsaWavesPerCu, kSsaBlock);
  a->blocks = (int)(a->items < cap ? a->items : cap);
  const long long pixels = (long long)a->groups * a->ascans * a->depth_count;
  const long long want = (pixels + kSsaBlock - 1) / kSsaBlock;
  a->mean_blocks = (int)(want < cap ? want : cap);
}

// The twiddles and the bands' table (a.tw, a.gauss) on `st`.
hipError_t launch_ssada_table(const SsadaArgs& a, hipStream_t st);
// The split of one pass: a.x -> a.bands.
hipError_t launch_ssada_split(const SsadaArgs& a, hipStream_t st);
// The band means of one pass: a.band_decorr, a.band_power -> a.out_decorr, a.out_power.
hipError_t launch_ssada_mean(const SsadaArgs& a, hipStream_t st);

}  // namespace fdoct
