/*
 * fdoct_colour.h -- webcam colour frames: BscanFFTwebcam's channelnum.
 *
 * BscanFFTwebcam.cpp reads its camera with cv::VideoCapture: every frame is an 8-bit, 3-channel interleaved B,G,R image.
 * Lines 1015-1038 make `mraw` of it as the ini's `channelnum` says,
 *   0, 1, 2:  that channel (B, G, R), still CV_8U;
 *   3:        (double(B) + double(G) + double(R)) * 0.00130718954, a CV_64F image in 0 ... 1,
 * and the block every program has follows: medianBlur, resize(INTER_AREA), convertTo(CV_64F), the chain.  These entry points
 * put that step on the device, where fdoct_set_frontend's median and binning already are:
 *   fdoct_set_colour_input / fdoct_get_colour_input   a handle's channelnum: its frame-taking calls read B,G,R frames
 *   fdoct_colour_extract                               the stage on its own, as fdoct_frontend is for mono frames
 *   fdoct_colour_sum_scale                             the constant
 * Conventions are fdoct.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across the
 * boundary.  No kernel or plan of the chain changes.
 *
 * The arithmetic.  Select: the channel goes through the front end's own median and binning (fdoct.h, fdoct_set_frontend), so
 * a call equals, bit for bit, the same call on a mono handle given that channel.  Sum: B + G + R is exact, the product with
 * the constant one double multiply; cv::medianBlur rejects CV_64F, so a median with the sum is FDOCT_ERR_UNSUPPORTED; the
 * binning is INTER_AREA on doubles -- the block's values added in double from 0.0, rows outermost and left to right, times
 * (double)(1.f / area) -- and the chain runs as it does for FDOCT_F64 frames of those values.
 */
#ifndef FDOCT_COLOUR_H
#define FDOCT_COLOUR_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* channelnum -1 (the default): mono frames, every call as without this header.  0 / 1 / 2: B / G / R.  3: the sum.  Anything
 * else is FDOCT_ERR_INVALID.  While it is 0 ... 3, fdoct_process, fdoct_process_async, fdoct_capture_reference and
 * fdoct_frame_minmax read their FDOCT_U8 frames as raw_h x raw_w x 3 bytes per frame, raw_w = width * binx and raw_h =
 * height * biny of fdoct_set_frontend; pitch_bytes is the pitch of the 3-channel rows, 0 = packed = 3 * raw_w; frames and
 * pitch may have any alignment.  Any other dtype is FDOCT_ERR_UNSUPPORTED, and so is channelnum 3 with a median set; such a
 * call is refused before anything is enqueued and leaves the handle as it was.  fdoct_frame_minmax reports the sum's doubles.
 * A setting of the handle like fdoct_set_frontend's: fdoct_clone_to_device carries it, fdoct_export_state does not. */
int fdoct_set_colour_input(fdoct_handle h, int channelnum);
int fdoct_get_colour_input(fdoct_handle h, int* channelnum);

/* The stage on its own, whatever the handle's setting: nframes frames of raw_h rows of raw_w B,G,R pixels at `bgr` (host or
 * device memory, pitch_bytes 0 = packed) -> packed frames of raw_h / biny rows of raw_w / binx samples at `out` (host or
 * device memory): uint8 for channelnum 0 / 1 / 2 after medianBlur(mediann) and the binning, double for channelnum 3 after
 * the binning (mediann must be 0).  The bin factors must divide the sizes.  Device memory on both sides: enqueues on the
 * handle's stream only. */
int fdoct_colour_extract(fdoct_handle h, const void* bgr, fdoct_memspace space, int nframes, int raw_w, int raw_h, size_t pitch_bytes,
                         int channelnum, int mediann, int binx, int biny, void* out, fdoct_memspace out_space);

/* 0.00130718954, the literal of BscanFFTwebcam.cpp:1031 (not 1 / 765).  Host only. */
double fdoct_colour_sum_scale(void);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_COLOUR_H */
