// fdoct_dispersion_kernels.h -- the device side of include/fdoct_dispersion.h (fdoct_dispersion.hip): the argument block of the
// four kernels, the call's geometry as plain functions (fdoct_dispersion.cpp refuses and plans with them before anything is
// enqueued), and the launcher.  Internal: fdoct_dispersion.cpp is the only caller.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>

namespace fdoct {

constexpr int kDispBlock = 256;            // threads of every kernel here
constexpr int kDispMinN = 16, kDispMaxN = 4096;
constexpr int kDispMaxK = 65536;
constexpr long long kDispMaxRowsK = 1LL << 24;
constexpr int kDispMinChunk = 8;           // candidates per workgroup: at least 8 (the forward transform is an eighth of the work) ...
constexpr long long kDispTargetWgs = 8192; // ... and beyond that as many as still leave this many workgroups (profiles/dispersion_rate.txt)
constexpr int kDispMaxPasses = 16;

// The winner as the third kernel writes it: fdoct_dispersion_best's layout (fdoct_dispersion.cpp asserts that).
struct DispBest {
  int index, i2, i3;
  double a2, a3, metric;
};

// One call as the kernels see it.
struct DispersionArgs {
  const float2* x = nullptr;   // rows x n pairs, row-major
  int rows = 0, n = 0;
  int K = 0, a2_count = 0, a3_count = 0;
  double a2_first = 0, a2_step = 0, a3_first = 0, a3_step = 0;
  int depth_first = 0, depth_count = 0;   // depth_count resolved: >= 1
  // decided by dispersion_plan_launch
  int per_wg = 0, chunks = 0;
  long long workgroups = 0;
  unsigned lds_bytes = 0;
  // the transform: Stockham radices of n (fdoct_plan.cpp's factorisation), magic[p] = ceil(2^32 / Ns) of pass p
  int npass = 0;
  int rad[kDispMaxPasses] = {};
  unsigned magic[kDispMaxPasses] = {};
  // device memory: tab holds n twiddles e^(+2 pi i m / n), then a2_count x n phasors e^(i a2 x^2), then a3_count x n phasors e^(i a3 x^3)
  float2* tab = nullptr;
  double2* row_sums = nullptr;  // rows x K (S2, S4): the search kernel writes, the row sum reads
  double2* sums = nullptr;      // K (S2, S4)
  DispBest* best = nullptr;
  float2* cos_sin = nullptr;    // n pairs of the winner; may be null
};

// The table's entries (float2 each).
inline size_t dispersion_tab_entries(int n, int a2_count, int a3_count) { return ((size_t)1 + (size_t)a2_count + (size_t)a3_count) * (size_t)n; }

// One workgroup's LDS: the spectrum, the transform's two buffers, the block's partial sums.
inline unsigned dispersion_lds_bytes(int n) { return (unsigned)(3u * (unsigned)n * sizeof(float2) + 2u * (kDispBlock / 64) * sizeof(double)); }

// Candidates per workgroup (include/fdoct_dispersion.h states the rule).  FDOCT_DISPERSION_CHUNK: a measurement switch, the
// chunk itself (tools/dispersion_rate.py sweeps it).
inline int dispersion_chunk(long long rows, int K) {
  static const int forced = [] { const char* e = std::getenv("FDOCT_DISPERSION_CHUNK"); return e ? std::atoi(e) : 0; }();
  long long c = forced > 0 ? forced : (rows * K + kDispTargetWgs - 1) / kDispTargetWgs;
  if (forced <= 0 && c < kDispMinChunk) c = kDispMinChunk;
  if (c > K) c = K;
  return (int)c;
}

// Fills the launch fields from the others.  Nothing is enqueued.
inline void dispersion_plan_launch(DispersionArgs* a) {
  a->per_wg = dispersion_chunk(a->rows, a->K);
  a->chunks = (a->K + a->per_wg - 1) / a->per_wg;
  a->workgroups = (long long)a->rows * a->chunks;
  a->lds_bytes = dispersion_lds_bytes(a->n);
}

// The tables, the search, the row sum and the winner, in that order on `st`.
hipError_t launch_dispersion(const DispersionArgs& a, hipStream_t st);

}  // namespace fdoct
