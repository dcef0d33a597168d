/*
 * fdoct_lowpass.h -- BscanDark's low-pass filter on captured reference frames, and the two switches of the capture.
 *
 * With `lowpassfilter` set in BscanDark.ini, BscanDark smooths each frame it captures -- dark, reference arm, sample arm --
 * with lpfilter (BscanDark.cpp:119-167; the calls are 1070-1074, 1145-1149, 1218-1222) before it composes data_yb and
 * data_yd from them.  With `saveinterferograms` set, BscanFFT and BscanDark accumulate the binned frames WITHOUT the moving
 * average (BscanFFT.cpp:1003-1036, line 1024; BscanDark.cpp:1008-1043).  These entry points bring both to
 * the capture call of fdoct_capture.h and offer the filter on its own:
 *   fdoct_set_capture_options / fdoct_get_capture_options   the two switches of a handle
 *   fdoct_lowpass_rows                                      lpfilter on any rows of doubles
 * Conventions are fdoct.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across the
 * boundary.  No kernel or plan of the chain changes.
 *
 * The filter, per row x[0 .. W-1] of doubles (lpfilter line by line): to float; the forward DFT scaled by 1 / W,
 * F[k] = (1 / W) sum_n x[n] e^(-2 pi i k n / W); the halves [0, cx) and [cx, 2 cx), cx = W / 2 in integer division, swapped
 * (an odd W leaves its last column in place); the shifted columns [0, dcl) and [dcr, dcr + dcl) zeroed, dcl = W / 2 - W / 10,
 * dcr = W / 2 + W / 10; the halves swapped back; the unscaled inverse DFT with real output, which reads bins 0 .. W / 2 as a
 * conjugate-symmetric spectrum; to double.  With f = W / 10 in integer division that is
 *   y[m] = Re F[0] + 2 * sum_{k=1}^{f-1} Re( F[k] e^(+2 pi i k m / W) )
 * for even and odd W, and all zeros for 1 < W < 10 (W = 1 blanks nothing: the row is its own result).  The reference
 * transforms in float; the library evaluates the f bins it needs directly in double, so its result is the mathematics of
 * lpfilter to ~1e-15 of the row's largest sample and differs from a float transform by that transform's own rounding.  The
 * same row gives the same bits in host or device memory, at any pitch, in any batch.
 */
#ifndef FDOCT_LOWPASS_H
#define FDOCT_LOWPASS_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* BscanDark.ini's `lowpassfilter` and the ini's `saveinterferograms`.  Both default to 0.
 * lowpass != 0: fdoct_capture_reference ends the recipe of its accumulating roles with the filter on every row of the
 *   frame, after the normalisations or the division by nframes (the reference's order, BscanDark.cpp:1056-1074):
 *   FDOCT_REF_DARK and FDOCT_REF_NONE (BscanDark's data_yd, data_yr, data_ys) and -- an extension: BscanFFT has no such
 *   switch -- FDOCT_REF_BACKGROUND.  FDOCT_REF_PI is never filtered (BscanDark does not filter data_yp), nor are the plain
 *   copies of FDOCT_VARIANT_SIM.
 * raw_accumulate != 0: the capture skips smoothmovavg whatever the handle's movavgn is; everything else is unchanged.
 * Settings of the handle like fdoct_set_frontend's: fdoct_clone_to_device carries them, fdoct_export_state does not. */
int fdoct_set_capture_options(fdoct_handle h, int lowpass, int raw_accumulate);
int fdoct_get_capture_options(fdoct_handle h, int* lowpass, int* raw_accumulate);

/* lpfilter (BscanDark.cpp:119-167) on `rows` rows of `width` doubles; in and out may be the same array; host or device
 * memory on either side; pitch_bytes 0 = packed.  Device on both sides: enqueues on the handle's stream only. */
int fdoct_lowpass_rows(fdoct_handle h, const double* in, fdoct_memspace in_space, int rows, int width, size_t pitch_bytes,
                       double* out, fdoct_memspace out_space);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_LOWPASS_H */
