/*
 * fdoct_saveframes.h -- per-frame B-scan saves while averaging (`save_individual_frames_if_averaging`, `saveframes`) on the GPU.
 *
 * Eight programs of the reference carry the block, switched by the ini's saveframes (main:370, 454).  While a group of
 * `averages` frames is accumulated, every frame's own magnitudes are kept beside the accumulator
 * (bscantemp.copyTo(bscansave0/1[indextemp]), main:1198-1205); on the `s` key each of them becomes an 8-bit picture of its own
 * (main:1360-1377): transpose, + 0.000001, log, 20 / 2.303, normalize(0, 1, NORM_MINMAX), convertTo(CV_8UC1, 255.0).  The
 * manual-averaging branch does the same on the finished linear B-scans it accumulated (main:1405-1412, 1447-1467), where the
 * image is already D x H.
 *
 * Two pieces serve a host that keeps its frames in device memory:
 *   fdoct_set_raw_magnitudes   makes the chain (fdoct_process*) write a group's mean magnitude WITHOUT its epsilon; with
 *                              averages = 1 that is exactly magI.colRange(0, D) of main:1195, a frame's own magnitudes;
 *   fdoct_saveframes           one stage that reads such per-frame magnitudes once and produces from them the averaged
 *                              bscan / bscandb of main:1197-1240 (sums in double, as the reference accumulates) and every
 *                              frame's save picture.
 * So the chain runs once per camera frame, with averages = 1, and nothing it computed before changes.
 *
 * Pictures.  Always D x H, what the reference writes to disk.  All arithmetic is in double on the float input, in the
 * reference's order: d = 20.0 * ln((double)x + 0.000001) / 2.303; lo, hi = the minimum and maximum of d over that one image;
 * scale = hi - lo > DBL_EPSILON ? 1 / (hi - lo) : 0; shift = 0 - lo * scale; byte = saturate(rint_half_even((d * scale + shift)
 * * 255.0)) -- the normalise and convert of fdoct_display, with no threshold and no clamp.  A constant image gives zeros.
 * Deviation: x + 0.000001 is clamped from below at 0.000001.  Only a negative input reaches that clamp, and magnitudes are not
 * negative; cv::log is undefined there (the deviation fdoct_bscanbin.h records for its own logarithm).
 *
 * Fold.  With averages >= 1, for every group of `averages` consecutive images: acc = the sum in double, in frame order;
 * b = acc / averages + eps in double, eps the handle's variant epsilon as the reference writes it (0.00001, main:1221-1222);
 * out_bscan = (float)b; out_db = (float)(20.0 * ln(b) / 2.303), and with fdoct_config.dc_mask and depths > 4 depth row 4 of
 * out_db is copied over its depth rows 0 and 1 (main:1239-1240).  All four combinations of in_layout and out_layout give the
 * same values bit for bit.
 *
 * The reference's ping-pong.  On `s` the reference saves the INACTIVE buffer (main:1365-1368): the frames of the PREVIOUS group,
 * and nothing on the first one.  This call makes pictures of the frames it is given; a host that wants the lag keeps the
 * previous group's magnitude buffer and passes that.
 *
 * Conventions are fdoct.h's and fdoct_manualavg.h's: int return codes, the last-error text, the handle's device and stream, no
 * exception across the boundary.  With device memory on both sides a call only enqueues on the handle's stream:
 * process_async -> saveframes -> display needs no host synchronisation in between.  Host memory on either side goes through
 * device buffers the handle owns and the call synchronises.  Pointers need the alignment of their element only (4-byte stores
 * of packed bytes are used where the pointer and `ascans` allow them, and give the same bytes).  Every refusal -- bad
 * arguments, outputs that overlap the input or each other, NULL misuse -- happens before anything is enqueued and leaves every
 * output untouched.
 *
 * The two switch calls live here and not in fdoct.h so that the ABI of fdoct.h stays as it is (the rule of fdoct_roi.h and every
 * header after it); FDOCT_VERSION_MINOR is 5 from this header on.
 */
#ifndef FDOCT_SAVEFRAMES_H
#define FDOCT_SAVEFRAMES_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Off by default.  On: the epsilon handed to every kernel of the chain is 0.0f, so out_bscan of fdoct_process* is the group's
 * mean magnitude as the kernel holds it, and out_db of those calls must be NULL -- otherwise they return FDOCT_ERR_INVALID
 * before anything is enqueued (the logarithm of an epsilon-free zero has no place in the display chain).  The binning of
 * fdoct_bscanbin.h keeps clamping at the variant's epsilon whatever the chain writes.  A run-time setting like `averages`:
 * fdoct_clone_to_device carries it, the state blob does not. */
int fdoct_set_raw_magnitudes(fdoct_handle h, int on);
/* 1 or 0; FDOCT_ERR_INVALID without a handle. */
int fdoct_get_raw_magnitudes(fdoct_handle h);

/* frames: nframes linear images of depths * ascans floats each, packed, in `mem`.  in_layout: FDOCT_LAYOUT_ROWMAJOR_HxD for a
 * frame's magnitudes as the chain writes them (main:1360-1377), FDOCT_LAYOUT_TRANSPOSED_DxH for finished B-scans
 * (main:1447-1467).
 *   out_gray   nframes pictures of depths x ascans bytes, or NULL
 *   averages   >= 1: the fold over groups of that many consecutive images (nframes must be a multiple of it); 0: no fold, and
 *              both fold outputs must be NULL
 *   out_bscan, out_db   nframes / averages images each in out_layout, or NULL
 * out_gray and the fold outputs may each be absent, but not all of them; all outputs are in out_mem.  A handle of
 * FDOCT_VARIANT_SIM that asks for the fold gets FDOCT_ERR_UNSUPPORTED: sim:936-947 copies and does not accumulate. */
int fdoct_saveframes(fdoct_handle h, const float* frames, fdoct_memspace mem, fdoct_layout in_layout, int nframes, int depths,
                     int ascans, unsigned char* out_gray, int averages, float* out_bscan, float* out_db, fdoct_layout out_layout,
                     fdoct_memspace out_mem);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_SAVEFRAMES_H */
