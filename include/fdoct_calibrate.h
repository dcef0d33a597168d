/*
 * fdoct_calibrate.h -- BscanDark's calibration on the GPU: the normalisations every capture ends with, the dark / reference /
 * sample captures held in device memory, and the composition of the background from them.
 *
 * BscanDark builds its background from three captures -- the `d`, `r` and `t` keys (BscanDark.cpp:1005-1222): the dark frame
 * data_yd, the reference arm data_yr and the sample arm data_ys -- as data_yb = (data_yr - data_yd) + (data_ys - data_yd)
 * (BscanDark.cpp:996).  The capture call of fdoct_capture.h makes each of the three, but downloads the sums and
 * normalises them on the host, and leaves the composition to the caller.  These entry points keep all of it on the device:
 *   fdoct_normalize_rows_minmax   cv::normalize(.., NORM_MINMAX) and normalizerows (BscanDark.cpp:82-90) on rows of doubles
 *   fdoct_calibrate_capture       one of the three captures, accumulated, normalised and filtered on the device and held there
 *   fdoct_calibrate_compose       BscanDark.cpp:996 from the three held captures; the result becomes the handle's background
 *   fdoct_calibrate_state / fdoct_calibrate_clear   which captures are held; dropping them
 * They are the C ABI of libfdoct_calibrate.so, an add-on library that is built next to libfdoct_hip.so and linked against it (the
 * core library's exported symbols are a closed set): a host links both, -lfdoct_calibrate -lfdoct_hip, and passes the handles of
 * fdoct.h to either.
 * Conventions are fdoct.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across the
 * boundary.  Every refusal happens before anything is enqueued and leaves the handle's state and every output untouched.  No
 * kernel or plan of the chain changes, and fdoct_capture_reference is what it was.
 *
 * A frame crosses PCIe once per key, downwards, and only where the handle's host mirror needs it: the handle keeps its
 * background, pi and dark frames as host doubles (fdoct_get_reference, fdoct_export_state and the table builds read them), so
 * the dark capture and the composition each end in one download.  The reference and sample captures download nothing unless
 * the caller asks for the result.
 *
 * The held captures are measurement state of the handle, like the peak holds of fdoct_roi.h: fdoct_clone_to_device does not
 * carry them, and the state blob of fdoct_export_state does not hold them.  A clone starts with three empty slots.
 */
#ifndef FDOCT_CALIBRATE_H
#define FDOCT_CALIBRATE_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { FDOCT_CAL_DARK = 0, FDOCT_CAL_REFERENCE = 1, FDOCT_CAL_SAMPLE = 2 } fdoct_cal_slot;

/* cv::normalize(y, out, lo, hi, NORM_MINMAX) on `rows` rows of `width` doubles; y and out may be the same array (in place; two
 * different arrays must not overlap); host or device memory on either side; pitch_bytes (0: packed) is that of both.
 * per_row != 0: every row on its own (normalizerows, BscanDark.cpp:82-90); per_row == 0: the rows * width samples as one plane.
 * The arithmetic is fdoct_normalize_minmax's (fdoct_capture.h), with min and max those of the row or of the plane:
 *   scale = (max(lo,hi) - min(lo,hi)) * (max - min > DBL_EPSILON ? 1 / (max - min) : 0), shift = min(lo,hi) - min * scale,
 *   y = y * scale + shift, multiply and add rounded separately
 * so that finite input gives the bits of the host helper.  Any width; the pitch a multiple of 8; pointers aligned to 8 bytes
 * (16-byte aligned rows are read with 16-byte loads).  Device memory on both sides: enqueues on the handle's stream only. */
int fdoct_normalize_rows_minmax(fdoct_handle h, const double* y, fdoct_memspace space, int rows, int width, size_t pitch_bytes,
                                double lo, double hi, int per_row, double* out, fdoct_memspace out_space);

/* One of BscanDark's three captures on `nframes` camera frames (host or device pointer, the frame format of
 * fdoct_capture_reference: RAW frames when a front end is set).  The recipe is the one fdoct_capture.h documents for the roles
 * DARK and NONE -- the front end and the colour input if set, smoothmovavg unless raw-accumulate is set (fdoct_lowpass.h), the
 * sum in frame order, every row to [0.0001, 1] if rowwisenormalize, the frame to [0.0001, 1] if !donotnormalize and else
 * acc / nframes, lpfilter last if the lowpass option is set -- in one sequence of launches with nothing coming back to the host
 * in between, and the same bits as fdoct_capture_reference returns for the same frames in the role FDOCT_REF_NONE.
 * The slot's H * W doubles stay in device memory the handle owns, replacing what the slot held.
 * FDOCT_CAL_DARK also becomes the handle's dark frame exactly as FDOCT_REF_DARK does (rows = H; BscanDark.cpp:1269 reads
 * data_yd as soon as it is captured): the one download the host mirror needs.  FDOCT_CAL_REFERENCE and FDOCT_CAL_SAMPLE change
 * nothing else, and download only if out_host is given.  out_host: H * W doubles of host memory for the result, or NULL.
 * Synchronous.  On any error the slot keeps what it held and the handle's state is untouched. */
int fdoct_calibrate_capture(fdoct_handle h, int slot, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes,
                            size_t pitch_bytes, double* out_host);

/* BscanDark.cpp:996 on the device, in double and in this order of operations: (yr - yd) + (ys - yd) from the three held slots.
 * FDOCT_ERR_STATE if a slot is empty.  The result becomes the handle's background with rows = H, exactly as if it had been
 * passed to fdoct_set_background: one download into the host mirror.  out_host: H * W doubles that receive it too, or NULL.
 * The slots stay held.  Synchronous.  On any error the background is what it was. */
int fdoct_calibrate_compose(fdoct_handle h, double* out_host);

/* held[slot] = 1 if the slot holds a capture, else 0.  Needs no device. */
int fdoct_calibrate_state(fdoct_handle h, int held[3]);

/* Empties the three slots and frees their device memory.  The handle's dark frame and background stay as they are. */
int fdoct_calibrate_clear(fdoct_handle h);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_CALIBRATE_H */
