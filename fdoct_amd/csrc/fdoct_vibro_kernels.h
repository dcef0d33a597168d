// fdoct_vibro_kernels.h -- the device side of include/fdoct_vibro.h (fdoct_vibro.hip): the argument block of the kernels, the
// chunk rule and the launch geometry as plain functions (fdoct_vibro.cpp refuses with them before anything is enqueued), and the
// launcher.  Internal: fdoct_vibro.cpp is the only caller.
#pragma once
#include <hip/hip_runtime.h>

namespace fdoct {

constexpr int kVibMaxFreq = 8;
constexpr int kVibMaxFrames = 65536;
constexpr long long kVibMaxPixels = 1LL << 24;
constexpr int kVibBlock = 256;             // four waves; a wave is one A-scan's 64 consecutive depths
constexpr int kVibWaves = kVibBlock / 64;
constexpr int kVibAhead = 4;               // frames the series pass loads ahead of the step that uses them
constexpr int kVibGridCap = 1 << 16;       // the most workgroups of the reference and series passes: a constant, not the card's
// The chunk rule (include/fdoct_vibro.h states it; profiles/vibro_rate.txt holds the sweep it is from).
constexpr int kVibTargetWaves = 1024;
constexpr int kVibMinChunk = 64;
constexpr int kVibBaseSums = 5;            // per chunk and pixel: S1, S2, St, the step total, the power sum; then 2 per frequency

// One call as the kernels see it.
struct VibroArgs {
  const float2* x = nullptr;     // T x ascans x depths pairs, row-major
  float2* refph = nullptr;       // T x ascans unit phasors conj(C) / |C| (use_ref): written by the reference pass
  double2* tab = nullptr;        // [nfreq][T] (w cos, w sin) of 2 pi nu t, written by the set-up kernel (nfreq > 0)
  double2* cst = nullptr;        // [chunks][nfreq + 1][2]: E = the sum of the table over the chunk's samples and F = the sum of t times it;
                                 // slot nfreq is the window alone, (w, 0)
  double2* head = nullptr;       // [nfreq + 1]: the table's entry at t = 0, which no chunk owns
  double2* glob = nullptr;       // [nfreq + 1][2]: the sums over all of t, G0 = head + sum of E in chunk order and G1 = sum of F
  double* part = nullptr;        // [chunks][kVibBaseSums + 2 nfreq][pixels] partial sums (chunks > 1)
  float2* out_amp = nullptr;     // any may be null
  float* out_rms = nullptr;
  float* out_drift = nullptr;
  float* out_power = nullptr;
  int T = 0, ascans = 0, depths = 0, pixels = 0;
  int use_ref = 0, ref_first = 0, ref_count = 0;   // ref_count resolved: > 0 with use_ref
  int detrend = 0, window = 0, nfreq = 0;
  double freq[kVibMaxFreq] = {0, 0, 0, 0, 0, 0, 0, 0};
  double scale = 1.0, min_power = 0.0;
  // decided by vibro_plan_launch
  int chunk_steps = 0, chunks = 0;
  int tiles_d = 0;               // waves along one A-scan
  long long tiles = 0, groups = 0, items = 0;   // waves of one chunk; workgroups of one chunk; workgroups' worth of work in all
  int series_blocks = 0, ref_blocks = 0, combine_blocks = 0;
};

__host__ __device__ inline int vibro_sums(int nfreq) { return kVibBaseSums + 2 * nfreq; }

// The plan's rule: a function of (T, pixels) alone.
inline int vibro_chunk_rule(int T, long long pixels) {
  const long long waves = (pixels + 63) / 64;
  const long long want = (kVibTargetWaves + waves - 1) / waves;
  long long cs = ((long long)(T - 1) + want - 1) / want;
  if (cs < kVibMinChunk) cs = kVibMinChunk;
  if (cs > T - 1) cs = T - 1;
  return (int)cs;
}

// Fills the launch fields from T, ascans, depths and chunk_steps (> 0).  Nothing is enqueued.
inline void vibro_plan_launch(VibroArgs* a) {
  a->pixels = a->ascans * a->depths;
  if (a->chunk_steps > a->T - 1) a->chunk_steps = a->T - 1;
  a->chunks = (a->T - 1 + a->chunk_steps - 1) / a->chunk_steps;
  a->tiles_d = (a->depths + 63) / 64;
  a->tiles = (long long)a->ascans * a->tiles_d;
  a->groups = (a->tiles + kVibWaves - 1) / kVibWaves;
  a->items = a->groups * a->chunks;
  a->series_blocks = (int)(a->items < kVibGridCap ? a->items : kVibGridCap);
  const long long rows = ((long long)a->T * a->ascans + kVibWaves - 1) / kVibWaves;
  a->ref_blocks = a->use_ref ? (int)(rows < kVibGridCap ? rows : kVibGridCap) : 0;
  a->combine_blocks = a->chunks > 1 ? (a->pixels + kVibBlock - 1) / kVibBlock : 0;
}

// The set-up kernels (nfreq > 0), the reference pass (use_ref), the series pass and the combine pass (chunks > 1), in that order
// on `st`.
hipError_t launch_vibro(const VibroArgs& a, hipStream_t st);

}  // namespace fdoct
