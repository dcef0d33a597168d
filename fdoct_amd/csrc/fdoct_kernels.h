// fdoct_kernels.h -- host/device interface between the C-ABI layer and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "fdoct_fused_rules.h"
#include "fdoct_plan.h"

namespace fdoct {

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: remember what has been granted
// on each device (one `LdsGrant` per kernel; the attribute only ever needs to grow).
struct LdsGrant {
  size_t granted[32] = {};
  std::mutex mu;  // handles on different devices may launch the same kernel from different host threads
  template <typename K>
  hipError_t ensure(K kernel, size_t lds) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    size_t& g = granted[dev & 31];
    if (lds > g) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      g = lds;
    }
    return hipSuccess;
  }
};

constexpr int FUSED_PROBE_PHASES = 12;
// Arguments of the fused kernel.  All pointers are device pointers.
struct FusedArgs {
  const void* frames;        // camera samples, row pitch in bytes
  const float* frames_lo;    // data_y handed over as doubles (main:987): frames = the f32 high words, this = the low words (same pitch), or null
  long long pitch_bytes;
  long long total_out_rows;  // groups * H
  int W, H, D, A;            // samples/row, rows/frame, output bins, frames averaged per output
  int need_rc;               // kernel must know (group,row): 2-D reference frames or min-max scalars
  int split;                 // staging layout: 1 = even/odd sample planes (see gather)
  int scratch_bytes;         // LDS bytes per row in flight
  int tw_count;              // entries in tw
  int lds_planes;            // 1: the three constant planes are staged in LDS; 0: resident-constant kernel, planes left out
  const float* ib;           // [W] 1/background (1-row mode) or null
  const float* ib2d;         // [H*W] 1/background (2-D mode) or null
  const float* il;           // [W] low word of 1/background (fdoct_capi.cpp::reciprocal_words), 1-row mode, or null
  const float* il2d;         // [H*WC] the same for the 2-D mode, laid out like ib2d
  const float* ilp;          // [WC] the 1-row low words in the order of the kernels' LDS planes (prec == 3)
  const uint32_t* il16;      // [WC/2] fused_il_half kernels: rho = il / ib scaled by 2^38 as half-float pairs, in the order the lanes read them
  const uint32_t* il16_2d;   // [H*WC/2] the same for a full-frame background (rows in frame order)
  int prec;                  // 0: one word (fast path without fdoct_set_precise_division); 1: both words, low words staged in LDS;
                             // 2: both words, full-frame background (il2d); 3: both words, low words read from ilp in global memory
  const float* yp; int yp_2d;  // pi frame or null
  const float* yd; int yd_2d;  // dark frame or null
  const float* win;          // [W] plane a_i = (1 + g_i) w_i  (window and slope weight folded; a_0, b_0: see fdoct_capi.cpp)
  const float* g;            // [W] plane b_i = -g_i w_(i-1), g = fractionalk indexed by sample
  const uint32_t* gidx;      // [NC] packed LDS byte offsets of the gather sources
  const float2* tw;          // Stockham twiddle tables
  const float2* utw;         // [T] exp(2*pi*i*l/N) (real path)
  const float2* phase;       // [N] dispersion phasors (complex path) or null
  const float2* minmax;      // [frames] whole-frame (min,max) or null
  int rowwisenormalize;
  int dcmask;
  int stage;                 // 0 = fused chain, 1 = resample stage (-> ylin), 2 = FFT stage (ylin ->)
  float2* ylin;              // [rows*NC] packed k-linear rows between the stages (staged mode only)
  int ablate;                // profiling aid: bit mask of stages to skip (results are then wrong); 0 in production
  float inv_A, eps, db_scale;
  float* out_mag;            // [groups*H*D] linear (bscan, row-major) or null
  float* out_db;             // [groups*H*D] dB or null
  // Transposed output written by the chain itself (TRO kernels): out_mag / out_db are then [groups][D][H] (the reference's
  // bscan layout, main:1220); finished rows go through a ring in LDS, tiles of FUSED_TR_ROWS rows (see fused_kernel)
  int tro;                   // 1: launch the TRO instantiation
  unsigned tr_ring;          // slots of the LDS ring of finished rows (one of kTroRingChoices)
  unsigned tr_tpf;           // tiles per frame = ceil(H / FUSED_TR_ROWS)
  unsigned tr_tpf_magic;     // floor(2^32 / tr_tpf)
  unsigned tr_total_tiles;   // groups * tr_tpf
  unsigned* tr_fault;        // one word of pinned host memory, set to 1 (a plain system-scope store) if a wave gave up waiting for a tile buffer (never, unless the protocol is broken)
#ifdef FDOCT_CLOCKPROBE
  unsigned long long* probe;  // tuning aid: {shader cycles, 100 MHz ticks} one wave spent in the kernel
#endif
#ifdef FDOCT_FUSED_PROBE
  unsigned long long* phase_probe;  // measurement build: cycles per phase of the row loop, [workgroup < 4][wave < 16][FUSED_PROBE_PHASES]
#endif
};

// Arguments of the any-configuration kernel (fdoct_generic.hip).  All pointers are device pointers.
// One in-LDS +i DFT of any length for generic_kernel's full-length zero-pad stage: Stockham radices of the length itself
// (blu_m == 0; tw = exp(+2 pi i j / n)) or, for a length with a prime factor above 5, Bluestein around two blu_m-point
// transforms (radices and tw of blu_m; chirp[n], bhat[blu_m] as fdoct_state.cpp::build_bluestein_tables makes them).
struct GenericDft {
  int n, blu_m, npass;
  int rad[GENERIC_MAX_PASSES];
  unsigned mag[GENERIC_MAX_PASSES];
  const float2 *tw, *chirp, *bhat;
};

struct GenericArgs {
  const void* frames;
  const float* frames_lo;    // low words of f64 frames (frames = their f32 high words, same pitch) or null
  long long pitch_bytes;
  long long total_out_rows;
  int dtype;                 // FDOCT_K_*
  int W, H, N, D, M, A;
  int L;                     // max(N, M*W, W): length of each DFT ping-pong buffer
  int ybuf_len;              // floats reserved for the row buffer (>= max(W, M*W), multiple of 4)
  const float* ib; int ib_2d;
  const float* il;           // low word of 1/background, indexed like ib (fdoct_capi.cpp::reciprocal_words)
  const float* yp; int yp_2d;
  const float* yd; int yd_2d;
  const float* win;          // [W] window (unscaled)
  const float* win_lo;       // [W] what the float window leaves of the double one (the band-pass forms the row in double)
  const float *yp_lo, *yd_lo;  // the same of the pi and dark frames (laid out like yp, yd)
  const float* g;            // [M*W] fractionalk indexed by sample (0 past numfftpoints)
  const int32_t* idx;        // [N] nearestkindex
  const float2* phase;       // [N] or null
  const float2* minmax;      // per input frame (min,max) or null
  const float2 *tw_n, *tw_w, *tw_mw;  // exp(+2*pi*i*j/n) for n = N, W, M*W (the last two only when M > 1)
  int rad_n[GENERIC_MAX_PASSES];
  unsigned mag_n[GENERIC_MAX_PASSES];  // ceil(2^32 / Ns) per pass
  int npass_n;
  // zero-pad upsampling (M > 1): the row is real and its padded spectrum Hermitian, so both DFTs run at half length
  const float2 *tw_wh, *tw_mwh;        // exp(+2*pi*i*j/n) for n = W/2, M*W/2
  int rad_wh[GENERIC_MAX_PASSES], rad_mwh[GENERIC_MAX_PASSES];
  unsigned mag_wh[GENERIC_MAX_PASSES], mag_mwh[GENERIC_MAX_PASSES];
  int npass_wh, npass_mwh;
  // zero-pad upsampling at FULL length (round 6): odd widths (the reference's fftshift leaves the last spectrum column in place
  // and an even multiplier pads to M W - 1 bins, main:215-241) and widths whose half-length transforms have a prime factor
  // above 5 -- W-point +i transform of the row, re-packing by pad_source's rule, zn-point +i transform, real parts.  In LDS as
  // long as two buffers of max(these transforms' lengths) fit; beyond that the long-row path (fdoct_big.hip) keeps the rows in HBM.
  int zp_full, zn;           // zn = W + 2 floor((M W - W) / 2), the padded spectrum's length
  GenericDft zf, zi;         // the W-point and the zn-point transform
  int radix16;               // 1: the pass plans hold radix-16 butterflies (the 1024-thread kernels only)
  int inplace;               // 1: ONE DFT buffer of L values (rows whose two buffers do not fit the LDS): generic_kernel<1024, 1, true>
  int bandpass;              // BscanDark.cpp:218-236 inside the zero-pad: keep spectrum bins 3 <= k < floor(W/10) only
  // real rows (no dispersion phase, even N): the N-point DFT is done as an N/2-point complex DFT + untangle
  int real_half;
  const float2* tw_nh;  // exp(+2*pi*i*j/(N/2))
  int rad_nh[GENERIC_MAX_PASSES];
  unsigned mag_nh[GENERIC_MAX_PASSES];
  int npass_nh;
  // Bluestein (numfftpoints with a prime factor above 5): the final +i transform of length n (N, or N/2 for real rows) as
  // chirp multiply -> forward DFT_Mb -> multiply by bhat -> inverse DFT_Mb -> chirp multiply; blu_m = Mb >= 2n - 1 (0: off)
  int blu_m;
  const float2 *blu_chirp, *blu_bhat, *tw_blu;  // e^(+i pi m^2/n), m < n; DFT_Mb(wrapped conj chirp)/Mb; e^(+2 pi i j/Mb)
  int rad_blu[GENERIC_MAX_PASSES];
  unsigned mag_blu[GENERIC_MAX_PASSES];
  int npass_blu;
  int rowwisenormalize, dcmask;
  float inv_A, eps, db_scale;
  float* out_mag;
  float* out_db;
  unsigned* row_ticket;      // launch-wide row counter, zero at launch (rows beyond the workgroups' first are claimed from it), or null
  float2* out_cx;            // not null: the complex A-scan instead (include/fdoct_complex.h) -- [rows*D] (re, im), A == 1, out_mag / out_db unused
};

hipError_t launch_generic(const GenericArgs& a, int grid, size_t lds, hipStream_t st);
hipError_t launch_movavg(const void* frames, int dtype, long long pitch_bytes, int W, long long rows, int n, float* out,
                         hipStream_t st);
// smoothmovavg of f64 frames: tap sums in double, out as two f32 planes (hi + lo)
hipError_t launch_movavg_f64(const double* in, long long pitch_elems, int W, long long rows, int n, float* hi, float* lo, hipStream_t st);
// ... of f32 frames (their samples need not be integers: a float tap sum would round at the size of the DC level)
hipError_t launch_movavg_f32_wide(const float* in, long long pitch_elems, int W, long long rows, int n, float* hi, float* lo, hipStream_t st);

hipError_t launch_median(const void* in, long long in_pitch, void* out, long long out_pitch, int dtype, int w, int h, int n,
                         int nframes, hipStream_t st);
hipError_t launch_bin(const void* in, long long in_pitch, void* out, long long out_pitch, int dtype, int ow, int oh, int binx,
                      int biny, int nframes, hipStream_t st);

// display post-chain (fdoct_display.hip); part: nbscans * display_parts(count) * 2 doubles of scratch
int display_parts(long long count);
hipError_t launch_display(const float* db, long long count, int nbscans, double thr, long long clamp_at, double* part,
                          const unsigned char* lut, unsigned char* gray, unsigned char* bgr, hipStream_t st);
hipError_t launch_lockin_db(const float* bscan, const float* jscan, long long count, long long jcount, float* out,
                            hipStream_t st);

// lean = the unpredicated fast-path kernel (see fused_kernel); the caller guarantees its conditions.
hipError_t launch_fused(const FusedPlan& p, const FusedArgs& a, int dtype, bool cplx, bool lean, int grid,
                        int block, size_t lds, hipStream_t st);
// whole-frame min/max; partial: scratch of minmax_partial_count(nframes) float2 (may be null: slow path only)
int minmax_partial_count(int nframes);
hipError_t launch_minmax(const void* frames, int dtype, long long pitch_bytes, int W, int H, int nframes,
                         const float* yd, int yd_2d, float2* out, float2* partial, hipStream_t st);
hipError_t launch_transpose(const float* in, float* out, int rows, int cols, int groups, hipStream_t st);
// data_y as doubles (main:987) -> two f32 planes, hi = fl32(x) and lo = fl32(x - hi): the chain carries both into the division
hipError_t launch_f64_split(const double* in, long long pitch_elems, float* hi, float* lo, int W, long long rows,
                            hipStream_t st);

}  // namespace fdoct
