/*
 * fdoct_doppler.h -- phase-resolved Doppler from complex A-scans: the Kasai autocorrelation estimator with a rectangular
 * averaging window, on the device.
 *
 * fdoct_complex.h's fdoct_process_complex gives the quantity everything phase-sensitive starts from.  This is the stage behind
 * it: the lag product of neighbouring A-scans (or of the same A-scan in neighbouring frames), an optional bulk-motion
 * correction, a box sum over a window, and the angle of the sum.  With a 1 x 1 window and no correction it is
 * np.angle(X[:, 1:] * np.conj(X[:, :-1])).
 *
 * Input: X[f][r][b], nframes images of ascans x depths interleaved (re, im) floats, row-major -- what fdoct_process_complex
 * writes with FDOCT_LAYOUT_ROWMAJOR_HxD.  8-byte aligned.
 *
 * Pair images  T[p][r][b] = X2 * conj(X1):
 *     FDOCT_DOPPLER_ASCANS   X1 = X[f][r], X2 = X[f][r + lag]: one pair image per frame, of ascans - lag rows;
 *     FDOCT_DOPPLER_FRAMES   X1 = X[f][r], X2 = X[f + lag][r]: nframes - lag pair images of ascans rows (M-mode, vibration,
 *                            repeated B-scans).
 * Bulk-motion correction (bulk = 1): per pair-image row B[p][r] = sum of T[p][r][b] over b in [bulk_first, bulk_first +
 * bulk_count), bulk_count = 0 meaning every depth; T' = T * conj(B) / |B|, and T' = T where |B| = 0.  Without it T' = T.
 * Window: R[p][r][b] = sum of T'[p][r'][b'] over r' in [r - (wa - 1) / 2, r + wa / 2] and b' in [b - (wd - 1) / 2, b + wd / 2]
 * (integer divisions; wa = win_ascans, wd = win_depths, both 1..32), truncated to the pair image -- it never reaches into
 * another pair image -- and cnt is the number of terms that remain.
 * Power: P = sum of (|X1|^2 + |X2|^2) / 2 over the same window.
 *
 * Outputs, each optional (NULL), at least one required, all of the pair images' shape [pair_images][pair_rows][depths]:
 *     out_phase   scale * atan2(Im R, Re R); 0 where min_power > 0 and P / cnt < min_power
 *     out_corr    R as (re, im) floats; must be aligned to 8 bytes
 *     out_power   P / cnt
 * Arithmetic is float; a requested subset of the outputs holds the same bits as all three together.
 *
 * fdoct_doppler_size gives the pair images' count and rows for a set of parameters, or refuses them: pure, no handle.
 * fdoct_doppler runs the stage on pairs in host or device memory; it reads nothing of the handle's geometry.
 * fdoct_process_doppler is fdoct_process_complex's chain followed by the stage, for camera frames of the handle's geometry
 * (ascans = height, depths = numdisplaypoints): the pairs stay in a workspace the handle owns.  Its kernel families, and its
 * refusals, are fdoct_process_complex's: FDOCT_ERR_UNSUPPORTED with averages other than 1 and for rows only the long-row path
 * takes, FDOCT_ERR_STATE without a background.  fdoct_last_kernel reports the chain's family.
 *
 * FDOCT_ERR_INVALID: a NULL input or params, a bad memory space, a window size outside 1..32, lag < 1, a lag that leaves no
 * pair image or no pair row, a bulk range outside [0, depths), a scale or min_power that is not finite, min_power < 0, an axis
 * that is neither value, all three outputs NULL, an input or out_corr that is not aligned to 8 bytes, out_phase or out_power
 * not aligned to 4, buffers that overlap, a batch too large.  Every refusal happens before anything is enqueued and leaves the
 * outputs untouched.
 *
 * Conventions are fdoct_complex.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across the
 * boundary.  With device memory on both sides the call enqueues on the handle's stream and returns without a synchronisation;
 * host memory on either side goes through device buffers the handle owns and the call synchronises.  The calls change nothing
 * a later fdoct_process* reads.
 *
 * The entry points ship in libfdoct_doppler.so, an add-on library over libfdoct_hip.so (link both).
 */
#ifndef FDOCT_DOPPLER_H
#define FDOCT_DOPPLER_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { FDOCT_DOPPLER_ASCANS = 0, FDOCT_DOPPLER_FRAMES = 1 } fdoct_doppler_axis;

typedef struct {
  int axis;        /* fdoct_doppler_axis */
  int lag;         /* >= 1 */
  int win_ascans;  /* wa, 1..32 */
  int win_depths;  /* wd, 1..32 */
  int bulk;        /* 0: no bulk-motion correction */
  int bulk_first;  /* first depth of the bulk sum */
  int bulk_count;  /* depths of the bulk sum; 0: all of them */
  double scale;    /* out_phase = scale * angle */
  double min_power; /* > 0: out_phase is 0 where P / cnt lies below it */
} fdoct_doppler_params;

int fdoct_doppler_size(const fdoct_doppler_params* params, int nframes, int ascans, int depths, int* pair_images, int* pair_rows);

int fdoct_doppler(fdoct_handle h, const float* re_im, fdoct_memspace space, int nframes, int ascans, int depths,
                  const fdoct_doppler_params* params, float* out_phase, float* out_corr, float* out_power, fdoct_memspace out_space);

int fdoct_process_doppler(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                          const fdoct_doppler_params* params, float* out_phase, float* out_corr, float* out_power,
                          fdoct_memspace out_space);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_DOPPLER_H */
