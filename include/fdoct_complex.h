/*
 * fdoct_complex.h -- the complex A-scan: the row's inverse transform itself, (re, im), where fdoct_process emits its modulus.
 *
 * The last step of the reference's block takes magnitude() of `complexI` after cv::dft(..., DFT_ROWS | DFT_INVERSE)
 * (BscanFFT.cpp:1185, 1189-1190) and drops the phase.  Everything phase-sensitive an FD-OCT instrument does -- Doppler and
 * displacement from the phase difference of neighbouring A-scans, vibration, complex averaging, a numerical dispersion search
 * (the dispersion phase of wangOCTrec4.m:130-131, 169 is tuned by looking at this quantity) -- starts from the content of
 * `complexI` in front of that step.  fdoct_process_complex is the chain of fdoct_process up to there.
 *
 * Value, per input frame and A-scan, for b < numdisplaypoints:
 *     X[b] = sum_q z[q] e^(+2 pi i b q / N),  N = numfftpoints, unscaled (DFT_INVERSE without DFT_SCALE),
 *     z[q] = (float)data_ylin[q] (main:1181), times the handle's phasor where fdoct_set_dispersion_phase is set.
 * No epsilon, no averaging, no logarithm, no DC mask.  Real rows displayed beyond N / 2: X[b] = conj(X[N - b]).  Every option in
 * front of the transform applies as in fdoct_process: the front end and colour input, smoothmovavg, dark and pi frame, both
 * normalisations, the sim variant's normalise, zero-pad and band-pass, the window, caller-supplied tables.  |X[b]| is what
 * fdoct_process gives with fdoct_set_raw_magnitudes, to rounding (the same kernel families, the same arithmetic up to the last
 * step).
 *
 * Output: for every frame and every A-scan numdisplaypoints interleaved (re, im) pairs of floats.
 *     FDOCT_LAYOUT_ROWMAJOR_HxD     out[frame][row][depth][2]
 *     FDOCT_LAYOUT_TRANSPOSED_DxH   out[frame][depth][row][2]   (the reference's picture; a tiled transpose behind the chain)
 * Both layouts hold the same values bit for bit.  out_re_im must be aligned to 8 bytes.
 *
 * Kernels.  Two families write the complex A-scan, and fdoct_last_kernel says which one a call took:
 *     FDOCT_KERNEL_WAVE_JIT   the wave-per-row kernel, compiled at run time for the handle's shape (fdoct_set_jit; the first
 *                             call pays the compile or the disk cache's load) -- every shape that kernel takes, the
 *                             power-of-two shapes fdoct_process gives to the fused kernel included;
 *     FDOCT_KERNEL_GENERIC    the workgroup-per-row kernel: every other shape whose rows fit a compute unit's LDS, and every
 *                             shape with run-time compilation turned off (fdoct_set_jit) or without libhiprtc.
 * The fused kernels do not write it, and neither does the long-row path: rows only that path takes (FDOCT_KERNEL_LONG_ROWS
 * under fdoct_process) are FDOCT_ERR_UNSUPPORTED here.
 *
 * Averaging: the handle's `averages` must be 1 (FDOCT_ERR_UNSUPPORTED otherwise).  The reference averages magnitudes; the mean
 * of complex A-scans is a different quantity, which nothing in it defines.
 *
 * Refusals happen before anything is enqueued and leave the output untouched: FDOCT_ERR_STATE without a background;
 * FDOCT_ERR_INVALID for a NULL pointer, nframes < 1, a bad dtype, layout or memory space, a pitch below a row, or an out_re_im
 * that is not aligned to 8 bytes; FDOCT_ERR_UNSUPPORTED as above.
 *
 * Conventions are fdoct_bscanbin.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across
 * the boundary.  With device memory on both sides the call enqueues on the handle's stream and returns without a
 * synchronisation; host memory on either side goes through device buffers the handle owns and the call synchronises.
 * pitch_bytes is the frames' row pitch (0: packed rows), of the raw camera rows where a front end is set.
 *
 * The call changes nothing a later fdoct_process* reads: the handle's plan, tables and kernel choice stay, so a handle that runs
 * FDOCT_KERNEL_FUSED keeps doing so, with the same results bit for bit.
 *
 * The entry point ships in libfdoct_complex.so, an add-on library over libfdoct_hip.so (link both).
 */
#ifndef FDOCT_COMPLEX_H
#define FDOCT_COMPLEX_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nframes frames of the handle's geometry in `space` -> nframes * height * numdisplaypoints (re, im) pairs in out_space. */
int fdoct_process_complex(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes,
                          size_t pitch_bytes, float* out_re_im, fdoct_memspace out_space, fdoct_layout layout);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_COMPLEX_H */
