/*
 * fdoct_bscanbin.h -- spinjnt's output binning (`bscanbinx` / `bscanbiny`) on the GPU, between the linear `bscan` and its dB.
 *
 * BscanFFTspinjnt.cpp reads bscanbinx and bscanbiny from its ini (build/BscanFFTspinjnt.ini:29-32, "binning applied in sw at
 * output").  With either of them, or a software binvalue, above 1, every averaged B-scan goes through (1856-1861)
 *   resize(bscan, bscanbinned, Size(), 1.0 / bscanbinx, 1.0 / bscanbiny, INTER_AREA);
 *   resize(multiplyfactor * bscanbinned, bscan, Size(), bscanbinx * binvaluey, bscanbiny, INTER_CUBIC);
 * with multiplyfactor = bscanbinx * bscanbiny * binvaluex * binvaluey (835), and only then through log, 20 / 2.303 and the DC
 * mask (1869-1874).  The J0 lock-in image takes the same pair before its own log (1894-1903), and so do the per-frame saves
 * (2016-2022, 2115-2121).  fdoct_bscan_bin is that stage as one kernel on the handle's device: the linear image in, the
 * resized linear image and / or its dB out, nothing in between in memory.
 * Conventions are fdoct.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across the
 * boundary.  No kernel, route or plan of the chain changes.
 *
 * Coordinates are the reference's picture, as in fdoct_roi.h: x runs along A-scans (columns of the D x H image), y along
 * depths.  binx / upx act along A-scans, biny / upy along depths.  Both layouts are accepted (FDOCT_LAYOUT_ROWMAJOR_HxD:
 * ascans x depths per B-scan; FDOCT_LAYOUT_TRANSPOSED_DxH: depths x ascans); the output has the input's layout, and both give
 * the same values bit for bit.
 *
 * The caller passes the reference's arguments as they stand: upx = bscanbinx * binvaluey (the reference's own quirk),
 * upy = bscanbiny, multiplyfactor as at 835.  The library does not second-guess them.
 *
 * Arithmetic, per B-scan, in double throughout, every sum in the order written:
 *   1. v = bscan; with jscan (one depths x ascans image shared by all B-scans), v = max(bscan - jscan, 0) + 0.001 (1849-1852).
 *   2. INTER_AREA at integer factors: b[Y][X] = (sum of the biny x binx block, rows outermost, left to right within a row)
 *      * (1 / (binx * biny)) * multiplyfactor.  depths % biny != 0 or ascans % binx != 0 is FDOCT_ERR_UNSUPPORTED (the
 *      reference leaves its integer path there).  Factors are 1..16 (1.0 / (1.0 / n) == n holds for every n <= 48, which is
 *      what keeps the reference on that path), upx and upy 1..64.
 *   3. INTER_CUBIC (A = -0.75) at scale 1 / u, along A-scans first and then along depths.  Output index d = k u + p has phase p:
 *      f = (p + 0.5) * (1 / u) - 0.5, s = floor(f), t = f - s; taps on cells k + s - 1 .. k + s + 2, each index clamped to the
 *      binned image (replicate border); c0 = ((A (t+1) - 5A)(t+1) + 8A)(t+1) - 4A, c1 = ((A+2) t - (A+3)) t^2 + 1,
 *      c2 = ((A+2)(1-t) - (A+3))(1-t)^2 + 1, c3 = 1 - c0 - c1 - c2; the four products are added left to right (top to
 *      bottom).  fdoct_bscanbin_taps gives the u tap sets; u = 1 is (0, 1, 0, 0), the identity.
 *   4. out_bscan = the cubic's value, rounded to float.  It can be <= 0: the kernel undershoots beside strong reflectors.
 *   5. out_db = 20 * ln(max(value, eps)) / 2.303, eps the handle's variant epsilon (1e-5 main, 1e-6 sim).  Without jscan and with
 *      fdoct_config.dc_mask set and out_depths > 4, depth row 4 is copied over depth rows 0 and 1 (1873-1874); with jscan
 *      there is no mask (1902-1903).
 * Deviation: cv::log documents its result for non-positive input as undefined; the reference takes the log of the cubic's
 * value as it is.  Here the value is clamped at eps first, so no NaN or infinity ever leaves the call.
 * What OpenCV itself does inside the two resizes (float coefficients and a float 1 / area on CV_64F data) is not pinned by
 * anything in this project: tests/bscanbin_model.py is the specification, in that "reference" precision and in double, and the
 * library is held to the double one within the project's tolerance.
 *
 * Asynchrony, as in fdoct_roi.h.  With device memory on both sides the call enqueues on the handle's stream and returns without
 * a synchronisation: fdoct_process_async -> fdoct_bscan_bin -> fdoct_display / fdoct_peakhold needs no host sync in
 * between.  (The first call with a new pair upx, upy uploads the tap table and waits for the stream once.)  Host memory on
 * either side goes through device buffers the handle owns and the call synchronises.  A failed call leaves outputs and handle
 * state untouched.  Input and output buffers must not overlap (FDOCT_ERR_INVALID).
 */
#ifndef FDOCT_BSCANBIN_H
#define FDOCT_BSCANBIN_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no GPU: the size of the result for an input of depths x ascans, out_depths = (depths / biny) * upy and
 * out_ascans = (ascans / binx) * upx.  Refuses what fdoct_bscan_bin refuses: FDOCT_ERR_INVALID for factors outside 1..16 /
 * 1..64, FDOCT_ERR_UNSUPPORTED for sizes the factors do not divide. */
int fdoct_bscanbin_size(int depths, int ascans, int binx, int biny, int upx, int upy, int* out_depths, int* out_ascans);

/* Host only, no GPU: the `up` distinct tap sets of the cubic pass at factor `up` (1..64), in double: taps4[4 p .. 4 p + 3] =
 * c0 .. c3 of phase p, and first_src_offset[p] (or NULL) = s - 1, the first tap's cell relative to d / up (-2 or -1). */
int fdoct_bscanbin_taps(int up, double* taps4, int* first_src_offset);

/* The stage itself on nbscans B-scans of depths x ascans floats in `mem` (jscan, or NULL, lies in `mem` too).  out_bscan and
 * out_db (either may be NULL, not both): nbscans images of out_depths x out_ascans floats in out_mem, in the input's layout. */
int fdoct_bscan_bin(fdoct_handle h, const float* bscan, const float* jscan, fdoct_memspace mem, fdoct_layout layout, int nbscans,
                    int depths, int ascans, int binx, int biny, int upx, int upy, double multiplyfactor, float* out_bscan,
                    float* out_db, fdoct_memspace out_mem);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_BSCANBIN_H */
