/*
 * fdoct_angio.h -- OCT angiography from repeated B-scans: the motion contrast of N complex B-scans taken at one slow-axis
 * position -- speckle variance of the intensity, amplitude decorrelation (the full-spectrum form of SSADA), complex decorrelation
 * with bulk-motion correction, and the mean power -- on the device, in one read of the pairs and one write of each result.
 *
 * fdoct_complex.h's fdoct_process_complex gives the quantity everything phase-sensitive starts from; fdoct_doppler.h gives the lag
 * product of one pair of frames as images.  This is the stage that reduces the repeats of a position to its contrast.
 *
 * Input: X[g][n][r][b], groups x repeats images of ascans x depths interleaved (re, im) floats, row-major: frame g repeats + n is
 * repeat n of position g -- what fdoct_process_complex writes with FDOCT_LAYOUT_ROWMAJOR_HxD.  8-byte aligned.  A group never
 * reads another group's frames.  Below I = |X|^2, A = sqrt(I), N = repeats; the pairs are n = 0 .. N - 2, always lag 1, and
 * T[n] = X[n + 1] conj(X[n]).
 *
 * 1. Bulk-motion correction (bulk = 1).  Per group, pair and A-scan B[g][n][r] = sum of T[n] over b in [bulk_first, bulk_first +
 *    bulk_count), bulk_count = 0 meaning up to depths.  T'[n] = T[n] conj(B) / |B|, and T' = T where |B| = 0.  Without the
 *    correction T' = T.  Only out_cdecorr reads it.
 * 2. Window.  sum_win is the box of win_ascans x win_depths (each 1 .. 16) placed as fdoct_doppler.h places it: A-scans
 *    [r - (wa - 1) / 2, r + wa / 2], and likewise on depth, truncated to the image; cnt is the number of terms that remain.
 * 3. Outputs, each optional (NULL), at least one required, each [groups][ascans][depths] floats:
 *        out_var      (1 / cnt) sum_win V,  V = (1 / N) sum_n (I_n - Ibar)^2,  Ibar = (1 / N) sum_n I_n
 *        out_decorr   1 - (1 / (N - 1)) sum_n Q_n,  Q_n = (sum_win A_n A_{n+1}) / (sum_win (I_n + I_{n+1}) / 2), Q_n = 1 where the
 *                     denominator is 0
 *        out_cdecorr  1 - |sum_n sum_win T'[n]| / (sum_n sum_win (I_n + I_{n+1}) / 2), and 0 where the denominator is 0
 *        out_power    (1 / (N cnt)) sum_n sum_win I_n
 *    Where min_power > 0 and out_power lies below it, the other three are 0.
 *    A requested subset of the outputs holds the same bits as all four together; what nothing reads is not computed.
 *
 * Arithmetic.  All of it is float.  V is Welford's recurrence over n in increasing n (mean += (I - mean) / (n + 1), M2 +=
 * (I - mean_before) (I - mean_after), V = M2 / N).  Sums over n run per pixel in increasing n and come before the window sums;
 * window sums run depth first, then rows, in increasing index.  The order of every sum is fixed by the call's shape and the pixel's
 * indices alone: no floating-point atomics, and a pixel's bits depend neither on which tile, workgroup or pass of the grid
 * computes it nor on what other groups hold.  Two runs give the same bits.
 *
 * Measured on one MI355X (profiles/angio_rate.txt; 64 device-resident frames of 1000 x 1024, medians of 20 calls): 4 repeats x 16
 * groups, all four outputs, 0.245 ms with the 1 x 1 window (2.0e11 pixel-pairs/s, the pairs read at 2.1 TB/s; the in-tree float4
 * copy moves the same bytes in 0.144 ms) and 0.696 ms with 5 x 5 (7.1e10); out_cdecorr alone 0.156 and 0.384 ms; 2 x 32: 0.270 and
 * 0.919 ms.  doppler_device per group followed by torch reductions for the same four images took 2.02 and 4.13 ms (4 x 16), 3.20
 * and 5.19 ms (2 x 32) in the same run.
 *
 * fdoct_angio_plan accepts or refuses a call and reports its geometry: pure, no handle.
 * fdoct_angio runs the stage on pairs in host or device memory; it reads nothing of the handle's geometry.
 * fdoct_process_angio is fdoct_process_complex's chain followed by the stage, for camera frames of the handle's geometry
 * (ascans = height, depths = numdisplaypoints): the pairs stay in a workspace the handle owns.  Its kernel families, and its
 * refusals, are fdoct_process_complex's: FDOCT_ERR_UNSUPPORTED with averages other than 1 and for rows only the long-row path
 * takes, FDOCT_ERR_STATE without a background.  fdoct_last_kernel reports the chain's family.
 *
 * FDOCT_ERR_INVALID: a NULL input or params, a bad memory space, repeats outside 2 .. 64, nframes not a positive multiple of
 * repeats or above 65536, ascans or depths < 1, ascans depths > 2^24, a window size outside 1 .. 16, bulk neither 0 nor 1, a bulk
 * range outside [0, depths), a min_power that is not finite or is negative, all four outputs NULL, an input not aligned to 8
 * bytes, an output not aligned to 4, buffers that overlap, a byte count that does not fit size_t.  Every refusal and every
 * reservation happens before anything is enqueued and leaves the outputs untouched.
 *
 * Conventions are fdoct_doppler.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across the
 * boundary.  With device memory on both sides the call enqueues on the handle's stream and returns without a synchronisation;
 * host memory on either side goes through device buffers the handle owns and the call synchronises.  The calls change nothing
 * a later fdoct_process* reads.
 *
 * The entry points ship in libfdoct_angio.so, an add-on library over libfdoct_hip.so (link both).
 */
#ifndef FDOCT_ANGIO_H
#define FDOCT_ANGIO_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDOCT_ANGIO_MAX_WIN 16
#define FDOCT_ANGIO_MAX_REPEATS 64

typedef struct {
  int repeats;      /* B-scans per position, 2 .. 64 */
  int win_ascans;   /* 1 .. 16 */
  int win_depths;   /* 1 .. 16 */
  int bulk;         /* 0: no bulk-motion correction */
  int bulk_first;   /* first depth of the bulk sum */
  int bulk_count;   /* depths of the bulk sum; 0: up to depths */
  double min_power; /* > 0: out_var, out_decorr and out_cdecorr are 0 where out_power lies below it */
} fdoct_angio_params;

typedef struct {
  int groups;               /* nframes / repeats */
  long long tiles;          /* tiles of 16 A-scans x 64 depths, over all groups */
  long long workgroups;     /* of the stage's kernel on a card of 256 compute units: min(tiles, 4 a compute unit); a call takes its own card's count */
  size_t workspace_bytes;   /* the bulk phasors */
} fdoct_angio_info;

int fdoct_angio_plan(const fdoct_angio_params* params, int nframes, int ascans, int depths, fdoct_angio_info* info);

int fdoct_angio(fdoct_handle h, const float* re_im, fdoct_memspace space, int nframes, int ascans, int depths,
                const fdoct_angio_params* params, float* out_var, float* out_decorr, float* out_cdecorr, float* out_power,
                fdoct_memspace out_space);

int fdoct_process_angio(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                        const fdoct_angio_params* params, float* out_var, float* out_decorr, float* out_cdecorr, float* out_power,
                        fdoct_memspace out_space);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_ANGIO_H */
