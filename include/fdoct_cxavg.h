/*
 * fdoct_cxavg.h -- coherent averaging of repeated complex B-scans: the complex mean of the N B-scans taken at one slow-axis position
 * after the repeats' common phase has been taken out, its modulus, the mean of the moduli over the same frames and the ratio of
 * the two sums -- on the device, in one read of the pairs from memory and one write of each result.
 *
 * Averaging the moduli of N repeats (the chain's `averages` and `movavgn`, fdoct_manualavg.h, fdoct_saveframes.h) keeps the noise
 * floor where it is and only smooths it; averaging the complex A-scans lowers it by about 10 log10 N dB.  fdoct_complex.h names the
 * complex average as one of the things its pairs exist for; this is its stage, next to fdoct_doppler.h, fdoct_vibro.h,
 * fdoct_dispersion.h and fdoct_angio.h.
 *
 * Input: X[f][r][b], nframes images of ascans x depths interleaved (re, im) floats, row-major -- what fdoct_process_complex writes
 * with FDOCT_LAYOUT_ROWMAJOR_HxD.  8-byte aligned.  With N = repeats and S = stride, group g's repeat n is frame g S + n, and there
 * are G = (nframes - N) / S + 1 groups: S = N gives disjoint positions (fdoct_angio.h's grouping), S < N a sliding coherent average.
 * X_n below is repeat n of the group at hand.
 *
 * 1. Alignment to repeat `ref`.  C[g][n][r] = sum of X_n[r][b] conj(X_ref[r][b]) over b in [align_first, align_first + align_count),
 *    align_count = 0 meaning up to depths.  align = 1: one phasor per group, repeat and A-scan, U = conj(C) / |C|, and 1 where
 *    |C| = 0.  align = 2: one per group and repeat, from C[g][n] = sum of C[g][n][r] over r in increasing r.  align = 0: U = 1, and
 *    the range is not read.  U[ref] is exactly 1 and is not computed.
 * 2. Outputs, each optional (NULL), at least one required, each [G][ascans][depths]:
 *        out_mean   (pairs, 8-byte aligned)  Z = (sum_n U_n X_n) / N
 *        out_mag    (floats)  |Z|
 *        out_incoh  (floats)  (sum_n |X_n|) / N: what averaging the moduli of the same frames gives, the image to hold out_mag against
 *        out_coh    (floats)  |sum_n U_n X_n| / sum_n |X_n|, and 0 where the denominator is 0: a phase-stability map in [0, 1]
 *    A requested subset of the outputs holds the same bits as all four together.
 *
 * Arithmetic.  All of it is float.  Sums over n run per pixel in increasing n, one division at the end.  The alignment sum is a
 * strided partial per thread, a butterfly within the wave and the waves in increasing index (fdoct_cxavg.hip); with align = 2 it is
 * fdoct_boxtile.h's per row and then the rows in increasing r.  The order of every sum is fixed by the call's shape and the pixel's
 * indices alone: no floating-point atomics, and a pixel's bits depend neither on which workgroup or pass of the grid computes it
 * nor on what other groups the call holds -- group g of a sliding call equals, bit for bit, a call on its N frames alone.  Two runs
 * give the same bits.
 *
 * The kernel takes one of two forms by the call's shape alone (fdoct_cxavg_info.form): where the N rows of an A-scan fit the 256
 * threads' registers -- repeats, rounded up to 2, 4, 8 or 16, times ceil(depths / 256) at most FDOCT_CXAVG_REG_PAIRS -- they are
 * read once and kept there between the alignment sum and the average (FDOCT_CXAVG_FORM_REGISTER); beyond that the alignment sum
 * reads its range and the average reads the rows again (FDOCT_CXAVG_FORM_STREAMING).
 *
 * Measured on one MI355X (profiles/cxavg_rate.txt; 64 device-resident frames of 1000 x 1024, medians of 20 calls): 4 repeats x 16
 * groups, align 1, all four outputs 0.199 ms (8.2e10 pixels/s, the pairs read at 2.6 TB/s; the in-tree float4 copy moves the same
 * bytes in 0.157 ms), out_mag alone 0.161 ms; align 0: 0.183 and 0.141 ms; align 2, with its two kernels in front: 0.446 and 0.405 ms;
 * 2 x 32: 0.276 ms (align 1), 0.256 (0), 0.472 (2).  The same four images from torch operations on the same pairs took 1.37 ms
 * (align 1), 0.81 (0) and 1.54 (2) at 4 x 16, 1.80, 1.19 and 1.97 ms at 2 x 32, in the same run.  The sliding average, 4 repeats at
 * stride 1 (61 groups, every frame read by up to four of them): 0.713 ms, 3.6 times the disjoint call's time for 3.8 times its pixels.
 *
 * fdoct_cxavg_plan accepts or refuses a call and reports its geometry: pure, no handle.
 * fdoct_cxavg runs the stage on pairs in host or device memory; it reads nothing of the handle's geometry.
 * fdoct_process_cxavg is fdoct_process_complex's chain followed by the stage, for camera frames of the handle's geometry
 * (ascans = height, depths = numdisplaypoints): the pairs stay in a workspace the handle owns.  Its kernel families, and its
 * refusals, are fdoct_process_complex's: FDOCT_ERR_UNSUPPORTED with averages other than 1 and for rows only the long-row path
 * takes, FDOCT_ERR_STATE without a background.  fdoct_last_kernel reports the chain's family.
 *
 * FDOCT_ERR_INVALID: a NULL input or params, a bad memory space, repeats outside 2 .. 64, stride outside 1 .. repeats, nframes
 * below repeats or above 65536 or with (nframes - repeats) no multiple of stride, ref outside [0, repeats), align outside 0 .. 2, an
 * alignment range outside [0, depths) (read with align 1 and 2 only), ascans or depths < 1, ascans depths > 2^24, all four outputs
 * NULL, an input or out_mean not aligned to 8 bytes, another output not aligned to 4, buffers that overlap, a byte count that does
 * not fit size_t.  Every refusal and every reservation happens before anything is enqueued and leaves the outputs untouched.
 *
 * Conventions are fdoct_angio.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across the
 * boundary.  With device memory on both sides the call enqueues on the handle's stream and returns without a synchronisation;
 * host memory on either side goes through device buffers the handle owns and the call synchronises.  The calls change nothing
 * a later fdoct_process* reads.
 *
 * The entry points ship in libfdoct_cxavg.so, an add-on library over libfdoct_hip.so (link both).
 */
#ifndef FDOCT_CXAVG_H
#define FDOCT_CXAVG_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDOCT_CXAVG_MAX_REPEATS 64
#define FDOCT_CXAVG_REG_PAIRS 16 /* pairs a thread keeps on chip in the register form */

#define FDOCT_CXAVG_FORM_REGISTER 1
#define FDOCT_CXAVG_FORM_STREAMING 2

typedef struct {
  int repeats;     /* B-scans per group, 2 .. 64 */
  int stride;      /* frames from one group's first to the next one's, 1 .. repeats */
  int ref;         /* the repeat the others are aligned to, 0 .. repeats - 1 */
  int align;       /* 0: none; 1: a phasor per group, repeat and A-scan; 2: per group and repeat */
  int align_first; /* first depth of the alignment sum */
  int align_count; /* depths of the alignment sum; 0: up to depths */
} fdoct_cxavg_params;

typedef struct {
  int groups;             /* (nframes - repeats) / stride + 1 */
  int form;               /* FDOCT_CXAVG_FORM_REGISTER or FDOCT_CXAVG_FORM_STREAMING */
  long long workgroups;   /* of the stage's kernel on a card of 256 compute units: min(groups x ascans, 4 a compute unit); a call takes its own card's count */
  size_t workspace_bytes; /* align = 2: the per-row sums and the phasors made from them */
} fdoct_cxavg_info;

int fdoct_cxavg_plan(const fdoct_cxavg_params* params, int nframes, int ascans, int depths, fdoct_cxavg_info* info);

int fdoct_cxavg(fdoct_handle h, const float* re_im, fdoct_memspace space, int nframes, int ascans, int depths,
                const fdoct_cxavg_params* params, float* out_mean, float* out_mag, float* out_incoh, float* out_coh,
                fdoct_memspace out_space);

int fdoct_process_cxavg(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                        const fdoct_cxavg_params* params, float* out_mean, float* out_mag, float* out_incoh, float* out_coh,
                        fdoct_memspace out_space);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_CXAVG_H */
