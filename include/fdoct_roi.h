/*
 * fdoct_roi.h -- readouts of the dB B-scans (`bscandb`) on the GPU, next to the image the chain wrote.
 *
 * The reference's instrument programs read three numbers off every displayed B-scan; these entry points compute them on
 * the handle's device, so that a host on the device path (fdoct_process_async) moves a few floats per B-scan over PCIe
 * instead of the image:
 *   fdoct_ascan_minmax        printMinMaxAscan, BscanFFT.cpp:146-171 (called at main:1116, 1786-1821)
 *   fdoct_roi_mean            printAvgROI, BscanFFT.cpp:99-144 (called at main:1290, 1833, 1845)
 *   fdoct_peakhold & co.      printPeakHoldAscan, BscanFFTpeak.cpp:466-739, with besseldbinverse (243-395) and errnull
 *                             (397-415) for the vibration amplitude
 * Conventions are fdoct.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across the
 * boundary.  The functions only read the image; no kernel or plan of the chain changes.
 *
 * Layout and coordinates.  `layout` says how each of the nbscans B-scans lies in memory: FDOCT_LAYOUT_ROWMAJOR_HxD is
 * ascans x depths (the chain's default), FDOCT_LAYOUT_TRANSPOSED_DxH is depths x ascans (the reference's `bscandb`).  Every
 * coordinate is in the reference's picture, whatever the layout: an A-scan index (ascanat, x, width) is a column of the
 * D x H image, a depth index (vertpos, y) a row.  A box that does not lie inside the image is FDOCT_ERR_INVALID.
 *
 * Which dB image.  The readouts operate on the image they are given.  BscanFFTpeak holds BEFORE the DC mask (hold at
 * BscanFFTpeak.cpp:1853, mask at 1856-1857); main's ROI mean reads AFTER it (mask at main:1239-1240, printAvgROI at 1290).
 * For an ROI that touches depth rows 0-1, the chain's output reproduces BscanFFTpeak's holds with fdoct_config.dc_mask = 0
 * and main's ROI mean with dc_mask = 1; away from those rows the setting does not matter.  printMinMaxAscan masks rows 0-3
 * of its own copy of the A-scan (154-157), so fdoct_ascan_minmax gives the same result for either image.
 *
 * Asynchrony.  With device memory, fdoct_ascan_minmax, fdoct_roi_mean and fdoct_peakhold enqueue on the handle's stream and
 * return without a synchronisation: an fdoct_process_async followed by fdoct_peakhold on the same stream needs no host
 * sync in between.  Host memory on either side, fdoct_get_peakhold and fdoct_vibration_profile synchronise the stream.
 *
 * Lifetime.  The peak-hold ROI and the four hold slots are measurement state, not set-up state: they live in the handle's
 * device memory and are freed with it, and they travel neither in fdoct_export_state / fdoct_import_state nor in
 * fdoct_clone_to_device: a clone starts with no ROI set.
 */
#ifndef FDOCT_ROI_H
#define FDOCT_ROI_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* printMinMaxAscan (BscanFFT.cpp:146-171): per B-scan, the min and max of A-scan `ascanat` over depths 0..depths-1, where
 * depth rows 0-3 are first replaced by row 4 (154-157).  Needs depths >= 5 (the reference reads row 4) and
 * 0 <= ascanat < ascans.  out_min / out_max: nbscans floats each, in out_mem; either may be NULL.  Exact: the results are
 * values of the input. */
int fdoct_ascan_minmax(fdoct_handle h, const float* bscandb, fdoct_memspace mem, fdoct_layout layout, int nbscans,
                       int depths, int ascans, int ascanat, float* out_min, float* out_max, fdoct_memspace out_mem);

/* printAvgROI (BscanFFT.cpp:99-144): per B-scan, the mean over depth rows vertpos..vertpos+2 and A-scans
 * ascanat..ascanat+width-1, summed in double (the reference's Scalar mean).  The box must pass the reference's STRICT guard
 * ascanat + width < ascans (BscanFFT.cpp:107; an A-scan box ending at the last column is refused there, and here) and its three rows
 * must fit (vertpos + 3 <= depths).  out_mean: nbscans doubles in out_mem.  The sum runs in a fixed order: reruns give the
 * same bits. */
int fdoct_roi_mean(fdoct_handle h, const float* bscandb, fdoct_memspace mem, fdoct_layout layout, int nbscans, int depths,
                   int ascans, int ascanat, int vertpos, int width, double* out_mean, fdoct_memspace out_mem);

/* The peak-hold ROI: A-scans x..x+w-1, depths y..y+hgt-1 (onMouse, BscanFFTpeak.cpp:112-180, on the D x H picture), and the
 * A-scan `ascanat` whose scalar hold runs over the same depths (ascanat may lie outside the ROI's columns).  Resets the column
 * holds of all four slots to 0 and leaves their scalar holds and counts alone, as onMouse and the m / M keys do (175-179,
 * 2655-2676).  Checked against an image when one is held (fdoct_peakhold).
 * Deviation: the reference treats an ROI at (0,0) as "not selected" (475-484); here any ROI is one, and holding before the
 * first fdoct_set_peakhold_roi is FDOCT_ERR_STATE. */
int fdoct_set_peakhold_roi(fdoct_handle h, int x, int y, int w, int hgt, int ascanat);

/* Folds nbscans dB B-scans into hold slot 1..4 (the 1-4 keys, BscanFFTpeak.cpp:497-731):
 *   column hold i  <- max(colmax_i, max over the ROI's depths of A-scan x+i)   (reduce(.., 0, MAX) and max(), 505-507, 523)
 *   scalar hold    <- max(held, max over the ROI's depths of A-scan ascanat)   (`if (maxVal > held)`, 502-503, 521-522)
 * Holds start at 0, not at -inf (Mat::zeros, 175-179; max1val = 0): a slot whose B-scans all lie below 0 dB holds 0.  Holds
 * are the f32 values of the input, bit for bit.  The reference's frame counter and key state machine (peakholdnumframes)
 * are the caller's: the library folds exactly the B-scans it is given and counts them, so a hold over 100 frames is 100
 * B-scans passed in one call or several.  FDOCT_ERR_INVALID: slot outside 1..4, the ROI or ascanat outside the image. */
int fdoct_peakhold(fdoct_handle h, int slot, const float* bscandb, fdoct_memspace mem, fdoct_layout layout, int nbscans,
                   int depths, int ascans);
/* The holds of one slot: colmax (w floats of the ROI set last, or NULL), ascanmax (the scalar hold, or NULL) and the number
 * of B-scans folded in since the slot was last cleared (or NULL).  Synchronises the handle's stream. */
int fdoct_get_peakhold(fdoct_handle h, int slot, float* colmax, float* ascanmax, long long* held_bscans);
/* Zeroes both holds of one slot and its count (the ! @ # $ keys, BscanFFTpeak.cpp:2568-2596).  Needs no ROI. */
int fdoct_clear_peakhold(fdoct_handle h, int slot);

/* The vibration readout of BscanFFTpeak.cpp, from the current holds, in double (the reference's CV_64F Mats), with
 * k = lambda0 * 1e9 / (4 * pi), pi = 3.141592653589793, and binv = fdoct_besseldb_inverse:
 *   mode 3 (slots 1,2,3; 597-644): disp = binv(max1 - max3) * k, err = (2.405 - binv(max1 - max2)) * k (errnull),
 *                                  profile[i] = binv(colmax1[i] - colmax3[i]) * k
 *   mode 4 (slots 1,2,3,4; 681-731): disp = binv(max1 - max4) * k, profile = profile(1,3) - profile(1,4), err = NaN
 * Deviations, both in mode 4: err is NaN because the reference prints a local it never set (726); and profile(1,3) is
 * computed from the current slot 1 and 3 holds, where the reference reuses the global profilearray its last mode-3 readout
 * left (650-652) -- the two agree when the slot-3 hold was the last one finished, which is the intended use.
 * lambda0 <= 0: the handle's, (float)((lambdamin + lambdamax) / 2) as BscanFFTpeak.cpp:1151 keeps it (a float).  profile_nm:
 * w doubles (or NULL); disp_nm, err_nm may be NULL.  FDOCT_ERR_STATE without an ROI.  Synchronises the handle's stream. */
int fdoct_vibration_profile(fdoct_handle h, int mode, double lambda0, double* profile_nm, double* disp_nm, double* err_nm);

/* besseldbinverse (BscanFFTpeak.cpp:243-395), host only, no GPU: x[i] = the reference's table at y[i], the inverse of
 * y = |20 log10 J0(x)| in steps of 0.05 (thresholds compared with `>`; 0 at or below 0.00543, 2.38 above 30 dB).  The
 * table is the reference's as it stands, including its top three entries, which do not follow the rule of the others. */
int fdoct_besseldb_inverse(const double* y, int n, double* x);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_ROI_H */
