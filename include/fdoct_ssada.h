/*
 * fdoct_ssada.h -- split-spectrum amplitude decorrelation (SSADA) from repeated B-scans: the spectrum of every complex A-scan is
 * split into `bands` Gaussian bands, every band is transformed back to an A-scan of lower axial resolution, the repeats of a
 * position are reduced to fdoct_angio.h's amplitude decorrelation band by band, and the bands' decorrelations are averaged.  What
 * bulk axial motion corrupts -- the axial resolution -- is given up, and the signal-to-noise comes back from the average.
 *
 * fdoct_angio.h's out_decorr is the full-spectrum form of this quantity; fdoct_dispersion.h is the stage that goes from complex
 * A-scans back to the spectrum.  This stage stands on both: the band A-scans are made as the dispersion search makes its
 * candidates', and the window stage is fdoct_angio's own kernel.
 *
 * Input: X[g][n][r][b], groups x repeats images of ascans x n interleaved (re, im) floats, row-major, A-scans of the FULL transform
 * length n (what fdoct_process_complex writes on a handle with numdisplaypoints = numfftpoints): frame g repeats + n is repeat n
 * of position g.  8-byte aligned.  Below M = bands, R = repeats, Dc the resolved depth count.
 *
 * 1. Spectrum.  z[q] = (1 / n) sum_b X[b] e^(-2 pi i b q / n) per A-scan, once.
 * 2. Band windows.  The support is [k_first, k_first + k_count), k_count = 0 meaning up to n; the spacing s = k_count / M; the
 *    centres c_m = k_first + (m + 1/2) s - 1/2.  Inside the support G_m(q) = exp(-1/2 ((q - c_m) / sigma)^2), outside it exactly 0;
 *    sigma is in bins.  Every entry is evaluated in double and rounded to float; the call builds the M x n table on the device, and
 *    fdoct_ssada_band_table writes the same table on the host.
 * 3. Band A-scans.  A_m[b] = sum_q z[q] G_m(q) e^(+2 pi i b q / n): the chain's own unscaled inverse, in float, kept for b in
 *    [depth_first, depth_first + depth_count), depth_count = 0 meaning up to n / 2.
 * 4. Per-band decorrelation.  d[g][m] is fdoct_angio.h's out_decorr of the R band images of position g -- its box window of
 *    win_ascans x win_depths (each 1 .. 16), its order of sums, its Q = 1 on a zero denominator -- and p[g][m] its out_power of the
 *    same images.  No power mask here.
 * 5. Band means.  out_decorr = (sum_m d[g][m]) / M and out_power = (sum_m p[g][m]) / M: float sums in increasing m from 0.f, then
 *    one division by (float)M.  Where min_power > 0 and out_power < min_power, out_decorr is 0.
 *
 * Outputs, each optional (NULL), at least one required:
 *        out_decorr       [groups][ascans][Dc] floats           step 5
 *        out_power        [groups][ascans][Dc] floats           step 5
 *        out_band_decorr  [groups][M][ascans][Dc] floats        d
 *        out_bands        [groups][M][repeats][ascans][Dc] pairs  the band A-scans: out_bands + (g M + m) R ascans Dc is a valid
 *                                                               fdoct_angio input of R frames
 * A requested subset holds the same bits as all four together; what nothing reads is not computed.
 *
 * Arithmetic.  All of it is float but the table.  The transform is a mixed-radix Stockham transform over LDS, its radices the
 * planner's for a complex row of n points; the product z G_m is two float multiplies.  The window stage is fdoct_angio's kernel on
 * groups x M pseudo-groups of R band images, so out_band_decorr[g][m] is fdoct_angio's out_decorr of out_bands' slice bit for bit.
 * No floating-point atomics; every sum's order is fixed by the call's shape; a group's bits depend neither on the other groups of
 * the call nor on the pass of the workspace it falls in, and a band's bits do not depend on the chunk of bands its workgroup takes.
 * Two runs give the same bits.
 *
 * The split kernel.  One workgroup of 256 threads takes one A-scan and a chunk of bands: the row into LDS, one forward transform,
 * z kept beside the transform's two buffers (3 n pairs: 96 KB at n = 4096), then per band the product, the inverse transform and
 * the store of the depth range, 8 bytes a lane, consecutive lanes on consecutive depths.  The rule that ships: a workgroup takes
 * ALL bands of its A-scan.  Measured on one MI355X (profiles/ssada_rate.txt; 64 device-resident frames of 1000 x 2048, 4 repeats x 16
 * groups, 4 bands, 1024 depths kept, medians of 20 calls): the split alone 3.47 ms with all four bands a workgroup, 4.38 ms with two
 * and 6.14 ms with one -- the forward transform is a fifth of a workgroup's work and a chunk repeats it; 64000 workgroups' worth of
 * A-scans fill the card without chunks.  That is 9.2e7 transforms a second, where the dispersion search, whose kernel this one is
 * modelled on, runs 9.6e7 of the same length.  The inverse transform's first pass reads the whole spectrum: G_m is exactly 0 only
 * outside the support, which all bands share, so a pass that skipped zeros would gain nothing with the default support and was not
 * built (EXPERIMENTS.md).  The stage as a whole (out_decorr and out_power) takes 4.19 ms with the 1 x 1 window and 5.62 ms with
 * 5 x 5; torch.fft, the table product and fdoct_angio per band took 7.02 and 8.41 ms for the same images in the same run.  The
 * split kernel uses 84 VGPRs and no scratch.  The grid is capped at eight workgroups a compute unit and loops over the A-scans.
 *
 * Workspace.  The band pairs take nframes M ascans Dc 8 bytes, and beside them d and p take nframes / R M ascans Dc 4 bytes each:
 * a group's share is M ascans Dc (8 R + 8) bytes.  The call runs in passes over whole groups, groups_per_pass = min(groups,
 * max_workspace_bytes / a group's share) -- max_workspace_bytes = 0 meaning 2 GiB -- and is refused where not even one group fits.
 * Groups are independent, so the number of passes changes no bit.  An out_bands in device memory is itself the pairs' workspace:
 * the call then runs in one pass and the handle holds d and p only, whatever the cap.  The table (n twiddles and M n floats) lies
 * beside the workspace and does not count against the cap.  The handle owns both.
 *
 * fdoct_ssada_band_table writes G as M x n floats on the host: pure, no handle.
 * fdoct_ssada_plan accepts or refuses a call and reports its geometry (for outputs in host memory): pure, no handle.
 * fdoct_ssada runs the stage on pairs in host or device memory; it reads nothing of the handle's geometry.
 * fdoct_process_ssada is fdoct_process_complex's chain followed by the stage, for camera frames of the handle's geometry (ascans =
 * height, n = numfftpoints): the pairs stay in a workspace the handle owns.  Its kernel families, and its refusals, are
 * fdoct_process_complex's; it adds FDOCT_ERR_UNSUPPORTED where numdisplaypoints != numfftpoints, as the dispersion search does.
 *
 * FDOCT_ERR_UNSUPPORTED: n outside 16 .. 4096 or with a prime factor above 5 (the transform lives in one workgroup's LDS).
 * FDOCT_ERR_INVALID: a NULL input or params, a bad memory space, n < 1, repeats outside 2 .. 64, bands outside 1 .. 16, nframes not a
 * positive multiple of repeats or nframes bands above 65536, ascans < 1, a support or a depth range outside [0, n) or without a
 * bin, ascans Dc > 2^24, a sigma that is not finite or not > 0, a window size outside 1 .. 16, a min_power that is not finite or
 * is negative, a max_workspace_bytes below one group's share, all four outputs NULL, an input or out_bands not aligned to 8
 * bytes, another output not aligned to 4, buffers that overlap, a byte count that does not fit size_t.  Every refusal and every
 * reservation happens before anything is enqueued and leaves the outputs untouched.
 *
 * Conventions are fdoct_angio.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across the
 * boundary.  With device memory on both sides the call enqueues on the handle's stream and returns without a synchronisation;
 * host memory on either side goes through device buffers the handle owns and the call synchronises (a host-memory out_bands is
 * copied down pass by pass from the workspace itself).  The calls change nothing a later fdoct_process* reads.
 *
 * The entry points ship in libfdoct_ssada.so, an add-on library over libfdoct_hip.so (link both).
 */
#ifndef FDOCT_SSADA_H
#define FDOCT_SSADA_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDOCT_SSADA_MAX_WIN 16
#define FDOCT_SSADA_MAX_REPEATS 64
#define FDOCT_SSADA_MAX_BANDS 16

typedef struct {
  int repeats;                /* B-scans per position, 2 .. 64 */
  int bands;                  /* spectral bands, 1 .. 16 */
  double sigma;               /* the bands' Gaussian width in bins, finite and > 0 */
  int k_first;                /* first bin of the bands' support */
  int k_count;                /* bins of the support; 0: up to n */
  int depth_first;            /* first depth kept */
  int depth_count;            /* depths kept; 0: up to n / 2 */
  int win_ascans;             /* 1 .. 16 */
  int win_depths;             /* 1 .. 16 */
  double min_power;           /* > 0: out_decorr is 0 where out_power lies below it */
  size_t max_workspace_bytes; /* the cap of the passes' workspace; 0: 2 GiB */
} fdoct_ssada_params;

typedef struct {
  int groups;               /* nframes / repeats */
  int depth_count;          /* Dc, resolved */
  int groups_per_pass;
  int passes;
  unsigned lds_bytes;       /* of one workgroup of the split kernel */
  long long workgroups;     /* of the split kernel's first pass on a card of 256 compute units; a call takes its own card's count */
  size_t workspace_bytes;   /* groups_per_pass times a group's share */
} fdoct_ssada_info;

int fdoct_ssada_band_table(const fdoct_ssada_params* params, int n, float* table);

int fdoct_ssada_plan(const fdoct_ssada_params* params, int nframes, int ascans, int n, fdoct_ssada_info* info);

int fdoct_ssada(fdoct_handle h, const float* re_im, fdoct_memspace space, int nframes, int ascans, int n, const fdoct_ssada_params* params,
                float* out_decorr, float* out_band_decorr, float* out_power, float* out_bands, fdoct_memspace out_space);

int fdoct_process_ssada(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                        const fdoct_ssada_params* params, float* out_decorr, float* out_band_decorr, float* out_power, float* out_bands,
                        fdoct_memspace out_space);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_SSADA_H */
