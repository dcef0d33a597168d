/*
 * fdoct_dispersion.h -- a numerical dispersion search over (a2, a3) on the device: the source of the table that
 * fdoct_set_dispersion_phase takes.
 *
 * fdoct_complex.h's fdoct_process_complex gives the complex A-scan; this stage takes A-scans of the FULL transform length, goes
 * back to the k-linear spectrum the chain transformed, applies each candidate phase as the chain applies it, transforms again and
 * scores the sharpness of the result.  The candidate whose A-scans are sharpest wins, and its (cos, sin) table comes back ready
 * for fdoct_set_dispersion_phase.
 *
 * Input: X[r][b], rows complex A-scans of n points (b < n), interleaved (re, im) floats, row-major, 8-byte aligned -- what
 * fdoct_process_complex writes with FDOCT_LAYOUT_ROWMAJOR_HxD on a handle with numdisplaypoints == numfftpoints.
 *
 *   1. z[r][q] = (1/n) sum_b X[r][b] e^(-2 pi i b q / n): the spectrum the chain transformed (real to rounding when the handle
 *      that made X has no phase set).
 *   2. Candidates: a2_i = a2_first + i a2_step (i < a2_count), a3_j = a3_first + j a3_step (j < a3_count); candidate index
 *      c = i a3_count + j, K = a2_count a3_count of them.
 *   3. phi_c(q) = a2 x^2 + a3 x^3, x = (q - n/2) / (n/2): the convention of fdoct_set_dispersion_phase's table.
 *   4. A_c[r][b] = sum_q z[r][q] e^(i phi_c(q)) e^(+2 pi i b q / n): the chain's own unscaled inverse.
 *   5. I = |A_c|^2;  S2[r][c] = sum of I, S4[r][c] = sum of I^2 over b in [depth_first, depth_first + depth_count);
 *      depth_count = 0 means up to n/2 (integer division).
 *   6. S2[c], S4[c]: the sums over rows, in increasing row order.
 *   7. metric[c] = S4[c] / S2[c]^2, and 0 where S2[c] = 0.
 *   8. The winner is the lowest index of the largest finite metric; index -1 when no metric is finite (then i2 = i3 = -1,
 *      a2 = a3 = metric = 0 and the table is zeros).
 *
 * Arithmetic: the transforms in float; the phasor is the float complex product of e^(i a2 x^2) and e^(i a3 x^3), each evaluated
 * in double and rounded to float (two tables, [a2_count][n] and [a3_count][n], built on the device by the call); I and I^2 in
 * float; every sum of them in double, in an order the launch geometry alone fixes; the sum over rows in double, in row order.
 * No floating-point atomics: a candidate's sums do not depend on scheduling, nor on which other candidates the call holds.
 *
 * Outputs, each optional (NULL), at least one required; a requested subset holds the same bits as all four together:
 *     out_sums       K x 2 doubles (S2[c], S4[c])
 *     out_row_sums   rows x K x 2 doubles (S2[r][c], S4[r][c])
 *     out_best       one fdoct_dispersion_best
 *     out_cos_sin    n (cos, sin) float pairs of the winner's phi, evaluated in double and rounded: what
 *                    fdoct_set_dispersion_phase takes with n_pairs = n
 *
 * fdoct_dispersion_phase_table writes the n (cos, sin) pairs of one (a2, a3): pure host, no handle.
 * fdoct_dispersion_plan accepts or refuses a call and reports its geometry: pure, no handle; info is written on success only.
 *     The rule: one workgroup takes one A-scan and a chunk of per_workgroup candidates -- it transforms the row forward once
 *     and runs one inverse per candidate -- so a larger chunk spends less on the repeated forward transform and a smaller one
 *     gives more workgroups.  per_workgroup = ceil(rows K / 8192) clamped to [8, K]: at least 8, which holds the forward
 *     transform to an eighth of the work, and beyond that as many as still leave 8192 workgroups.  Measured on an MI355X with
 *     64 x 64 candidates over 64 A-scans of 2048 points: 52, 69, 81, 90, 95, 96, 94, 91, 72 and 11 million transforms a second
 *     with 1, 2, 4, 8, 16, 32, 64, 128, 512 and 4096 candidates per workgroup; the rule gives 32 there.  chunks =
 *     ceil(K / per_workgroup), workgroups = rows chunks.
 * fdoct_dispersion_search runs the stage on pairs in host or device memory; it reads nothing of the handle's geometry.
 * fdoct_process_dispersion_search is fdoct_process_complex's chain into a workspace the handle owns, followed by the stage, with
 *     rows = nframes x height and n = numfftpoints.  Its kernel families, and its refusals, are fdoct_process_complex's, and it
 *     adds FDOCT_ERR_UNSUPPORTED when numdisplaypoints != numfftpoints: a calibration handle is the instrument's configuration
 *     with the display set to the full length.  If the handle has a phase set, the chain has applied it already and the search
 *     finds the RESIDUAL phase on top of it, not the total.
 *
 * Accepted: n = 2^a 3^b 5^c with 16 <= n <= 4096 (the row's spectrum and the transform's two buffers lie beside each other in
 * one workgroup's LDS); 1 <= K <= 65536; rows K <= 2^24; finite firsts and steps; a depth range inside [0, n) with at least one
 * bin.
 * FDOCT_ERR_INVALID: a NULL input or grid, a bad memory space, all outputs NULL, an input or output that is not aligned to 8
 * bytes, buffers that overlap, any bound above.  FDOCT_ERR_UNSUPPORTED: other lengths (a prime factor above 5, n > 4096).
 * Every refusal happens before anything is enqueued and leaves the outputs untouched.
 *
 * Conventions are fdoct_complex.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across the
 * boundary.  The winner is chosen on the device: with device memory on both sides the call enqueues on the handle's stream and
 * returns without a synchronisation; host memory on either side goes through device buffers the handle owns and the call
 * synchronises.  The calls change nothing a later fdoct_process* reads.
 *
 * The entry points ship in libfdoct_dispersion.so, an add-on library over libfdoct_hip.so (link both).
 */
#ifndef FDOCT_DISPERSION_H
#define FDOCT_DISPERSION_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  double a2_first;  /* a2_i = a2_first + i * a2_step */
  double a2_step;
  int a2_count;     /* >= 1 */
  double a3_first;  /* a3_j = a3_first + j * a3_step */
  double a3_step;
  int a3_count;     /* >= 1 */
  int depth_first;  /* first bin of the sums */
  int depth_count;  /* bins of the sums; 0: up to n / 2 */
} fdoct_dispersion_grid;

typedef struct {
  int index;      /* c = i2 * a3_count + i3; -1: no finite metric */
  int i2;
  int i3;
  double a2;
  double a3;
  double metric;
} fdoct_dispersion_best;

typedef struct {
  int candidates;          /* K */
  int per_workgroup;       /* candidates one workgroup takes */
  int chunks;              /* workgroups per A-scan */
  unsigned lds_bytes;      /* of one workgroup */
  long long workgroups;    /* rows * chunks */
  size_t workspace_bytes;  /* device memory the handle may hold for the call: tables, row sums, sums, the winner */
} fdoct_dispersion_info;

int fdoct_dispersion_phase_table(int n, double a2, double a3, float* cos_sin_pairs);

int fdoct_dispersion_plan(const fdoct_dispersion_grid* grid, int rows, int n, fdoct_dispersion_info* info);

int fdoct_dispersion_search(fdoct_handle h, const float* re_im, fdoct_memspace space, int rows, int n, const fdoct_dispersion_grid* grid,
                            double* out_sums, double* out_row_sums, fdoct_dispersion_best* out_best, float* out_cos_sin,
                            fdoct_memspace out_space);

int fdoct_process_dispersion_search(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes,
                                    size_t pitch_bytes, const fdoct_dispersion_grid* grid, double* out_sums, double* out_row_sums,
                                    fdoct_dispersion_best* out_best, float* out_cos_sin, fdoct_memspace out_space);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_DISPERSION_H */
