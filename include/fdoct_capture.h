/*
 * fdoct_capture.h -- the reference frames of a handle (background, pi, dark) captured on the GPU from camera frames.
 *
 * fdoct_set_background / _pi_frame / _dark (fdoct.h) take FINISHED data_yb / data_yp / data_yd: host doubles, already
 * accumulated and normalised.  The reference makes them from live camera frames in its key handlers; these entry points
 * do the same from frames that may already live in device memory, so that a host on the device path
 * (fdoct_process_async) neither copies `averagestoggle` frames back over PCIe nor restates the recipe:
 *   fdoct_capture_reference   the `b` key (BscanFFT.cpp:1000-1075, live branch 1041-1064), the `p` key (1077-1099),
 *                             BscanDark's dark / reference / sample captures (BscanDark.cpp:1005-1190, same recipe),
 *                             BscanFFTsim's `b` / `p` (BscanFFTsim.cpp:803-825)
 *   fdoct_get_reference       reads back what a role holds (data_yb / data_yp / data_yd as the handle keeps them)
 *   fdoct_frame_minmax        the "Max intensity" status line (BscanFFT.cpp:1105-1108, BscanFFTsim.cpp:832-835)
 *   fdoct_normalize_minmax    cv::normalize(.., NORM_MINMAX) on doubles, as BscanFFT.cpp:1031 / 1055 / 1096 use it
 * Conventions are fdoct.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across the
 * boundary.  No kernel or plan of the chain changes, and the chain consumes a captured frame exactly as it consumes one
 * passed to a setter.
 *
 * Frames.  `frames` holds nframes frames back to back in the format fdoct_process* takes: H rows of W samples at
 * pitch_bytes per row (0: packed), or -- when a front end is set (fdoct_set_frontend) -- the RAW camera frames of
 * H * biny rows of W * binx samples, which go through the median and the INTER_AREA binning first (8- and 16-bit only).
 * Pointer and pitch need the alignment of one sample only; 16-byte aligned rows are read with 16-byte loads.
 *
 * The recipe, per role (all arithmetic in double, in the reference's order, so results match a host restatement bit for
 * bit; samples are finite):
 *   every frame       front end if set; to double; FDOCT_VARIANT_MAIN with movavgn > 0: smoothmovavg (BscanFFT.cpp:276-294:
 *                     the sum over taps -n..n in that order, a tap outside the row replaced by the centre sample, plus the
 *                     centre, then / 2 / (n + 1))
 *   BACKGROUND, DARK, NONE
 *                     acc = 0; acc += frame, in frame order (cv::accumulate, 1043); if rowwisenormalize: every row to
 *                     [0.0001, 1]; if !donotnormalize: the whole frame to [0.0001, 1], else acc = acc / nframes (1050-1057;
 *                     BscanDark.cpp:1056-1063).  Both normalisations run when both flags say so.  nframes >= 1 is the
 *                     caller's averagestoggle.
 *   PI                nframes must be 1 (1081 copies one data_y); rows to [0, 1] if rowwisenormalize, the frame to [0, 1]
 *                     if !donotnormalize (1093-1096); no division.
 *   FDOCT_VARIANT_SIM BACKGROUND and PI are the (binned) frame as doubles: no moving average, no normalisation, no
 *                     division, nframes must be 1 (BscanFFTsim.cpp:803-825).  DARK and NONE follow the rule above with the
 *                     config's flags (and no moving average: the sim variant has none).
 *   options           fdoct_lowpass.h adds two switches of the handle, both off by default: BscanDark's lpfilter as the last
 *                     step of BACKGROUND, DARK and NONE, and the saveinterferograms branch (1003-1036), which accumulates the
 *                     binned frames without the moving average (1024).
 * Not covered: an asynchronous form of the capture.  BscanDark's composition data_yb = (yr - yd) + (ys - yd) and captures whose
 * normalisations stay on the device are fdoct_calibrate.h's; this call downloads its sums and normalises them on the host.
 * The division is a division (acc[i] / nframes), as the CPU restatement of this project divides everywhere the reference
 * writes `Mat / scalar`.
 */
#ifndef FDOCT_CAPTURE_H
#define FDOCT_CAPTURE_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { FDOCT_REF_BACKGROUND = 0, FDOCT_REF_PI = 1, FDOCT_REF_DARK = 2, FDOCT_REF_NONE = 3 } fdoct_ref_role;

/* The b / p / dark-key recipe on `nframes` camera frames (host or device pointer, same frame format
 * fdoct_process* takes: RAW frames when a front end is set).  The result becomes the handle's background /
 * pi / dark frame exactly as if the caller had passed it to fdoct_set_background / _pi_frame / _dark (rows = H);
 * FDOCT_REF_NONE changes no state.  out_host: H*W doubles of host memory that receive the result, or NULL.
 * Synchronous.  On any error the handle's previous state is untouched. */
int fdoct_capture_reference(fdoct_handle h, int role, const void* frames, fdoct_dtype dtype, fdoct_memspace space,
                            int nframes, size_t pitch_bytes, double* out_host);

/* The frame a role currently holds, as the doubles the setters / the capture stored: *rows = 0, 1 or H.
 * out receives rows * W doubles (cap_doubles is its capacity; too small is FDOCT_ERR_INVALID) or may be NULL to ask for
 * *rows only.  role: BACKGROUND, PI or DARK.  Needs no device. */
int fdoct_get_reference(fdoct_handle h, int role, double* out, size_t cap_doubles, int* rows);

/* "Max intensity" (main:1105-1108): min and max of every frame AFTER the front end (the reference reads opm),
 * nframes doubles each, either may be NULL; out_space says where they live.  Exact: the results are samples of the
 * input.  With device memory on both sides the call only enqueues on the handle's stream; host memory on either side
 * synchronises it. */
int fdoct_frame_minmax(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes,
                       size_t pitch_bytes, double* out_min, double* out_max, fdoct_memspace out_space);

/* Host only, no GPU needed: cv::normalize(y, y, lo, hi, NORM_MINMAX) on n doubles, as main:1031 / 1055 use it:
 * scale = (max(lo,hi) - min(lo,hi)) * (max - min > DBL_EPSILON ? 1 / (max - min) : 0), shift = min(lo,hi) - min * scale,
 * y = y * scale + shift, multiply and add rounded separately.  n = 0 is a no-op. */
int fdoct_normalize_minmax(double* y, size_t n, double lo, double hi);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_CAPTURE_H */
