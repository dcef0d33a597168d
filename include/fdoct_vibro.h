/*
 * fdoct_vibro.h -- phase-sensitive vibrometry from complex A-scans over time: common-mode correction by a reference surface,
 * the phase unwrapped over the frames, and per pixel the complex amplitude at up to 8 drive frequencies (a lock-in), the RMS
 * displacement, the net drift and the mean power, on the device, in one read of the pairs.
 *
 * fdoct_complex.h's fdoct_process_complex gives the quantity everything phase-sensitive starts from; fdoct_doppler.h gives wrapped
 * phase steps.  This is the stage that follows a pixel through time.
 *
 * Input: X[t][r][b], T = nframes images of ascans x depths interleaved (re, im) floats, row-major -- what fdoct_process_complex
 * writes with FDOCT_LAYOUT_ROWMAJOR_HxD.  8-byte aligned.  Time is the frame index.
 *
 * 1. Reference (ref = 1).  C[t][r] = sum of X[t][r][b] over b in [ref_first, ref_first + ref_count), ref_count = 0 meaning up to
 *    depths.  Y = X conj(C) / |C|, and Y = X where |C| = 0.  Without a reference Y = X.
 * 2. Steps.  d[s] = atan2(Im, Re) of Y[s + 1] conj(Y[s]), s = 0 .. T - 2.
 * 3. Unwrapped phase.  phi[0] = 0, phi[t] = phi[t - 1] + d[t - 1].
 * 4. Detrend.  detrend = 0: phi' = phi - mean(phi).  detrend = 1: phi' = phi - (alpha + beta t), the least-squares line over
 *    t = 0 .. T - 1.
 * 5. Time window w[t].  FDOCT_VIBRO_RECT: 1.  FDOCT_VIBRO_HANN: 0.5 - 0.5 cos(2 pi t / (T - 1)), and 1 for T = 2.
 * 6. Lock-in.  For each of nfreq (0 .. 8) frequencies nu_j in cycles per frame, 0 < nu_j <= 0.5:
 *        A_j = (2 / sum w) sum over t of w[t] phi'[t] e^(-2 pi i nu_j t).
 *    A vibration phi(t) = a sin(2 pi nu t + psi) over a whole number of cycles gives A = -i a e^(i psi): |A| is its amplitude.
 * 7. Outputs, each optional (NULL), at least one required:
 *        out_amp     [nfreq][ascans][depths] (re, im) pairs, scale A_j; must be NULL with nfreq = 0; aligned to 8 bytes
 *        out_rms     [ascans][depths], |scale| sqrt(mean over t of phi'^2)
 *        out_drift   [ascans][depths], scale phi[T - 1]
 *        out_power   [ascans][depths], the mean over t of |X|^2
 *    Where min_power > 0 and the mean power lies below it, out_amp, out_rms and out_drift are 0.
 *    A requested subset of the outputs holds the same bits as all four together.
 *
 * Arithmetic.  The products, the reference sum and atan2f are float; phi and every sum over time are double; the phasors
 * e^(-2 pi i nu t) and w[t] are evaluated in double by a set-up kernel.  The order of every sum is fixed by (T, ascans, depths,
 * chunk_steps) alone -- not by the card, by scheduling or by what other pixels hold -- and there are no floating-point atomics, so
 * two runs give the same bits, and a pixel's bits depend on its own series and its A-scan's reference range only.
 *
 * Time is split into chunks of chunk_steps steps that run side by side (adjacent chunks share one frame) and are put together
 * per pixel in chunk order, so that a single A-scan over a long record (M-mode) still fills the card.  chunk_steps = 0 takes the
 * plan's rule, a function of (T, ascans depths) only:
 *        waves = ceil(ascans depths / 64); want = ceil(1024 / waves);
 *        chunk_steps = max(ceil((T - 1) / want), 64), at most T - 1; chunks = ceil((T - 1) / chunk_steps).
 * The rule's two constants are from a sweep of chunk_steps on an MI355X (profiles/vibro_rate.txt): 1 x 1024 pixels over 4096 frames
 * took 0.90, 0.46, 0.25, 0.140, 0.097, 0.092, 0.125, 0.21, 0.39 and 1.63 ms with 4, 8, 16, 32, 64, 128, 256, 512, 1024 and 4095 steps a
 * chunk -- best with 512 to 1024 waves in flight and chunks of 64 steps or more -- and 1000 x 1024 pixels over 64 frames 0.40, 0.30,
 * 0.26 and 0.23 ms with 8, 16, 32 and 63: one chunk wherever the pixels fill the card.
 *
 * fdoct_vibro_plan accepts or refuses a call and reports its geometry: pure, no handle.
 * fdoct_vibro runs the stage on pairs in host or device memory; it reads nothing of the handle's geometry.
 * fdoct_process_vibro is fdoct_process_complex's chain followed by the stage, for camera frames of the handle's geometry
 * (ascans = height, depths = numdisplaypoints): the pairs stay in a workspace the handle owns.  Its kernel families, and its
 * refusals, are fdoct_process_complex's: FDOCT_ERR_UNSUPPORTED with averages other than 1 and for rows only the long-row path
 * takes, FDOCT_ERR_STATE without a background.  fdoct_last_kernel reports the chain's family.
 *
 * FDOCT_ERR_INVALID: a NULL input or params, a bad memory space, T < 2 or T > 65536, ascans or depths < 1, ascans depths > 2^24,
 * nfreq outside 0 .. 8, a frequency that is not finite or lies outside (0, 0.5], a reference range outside [0, depths), a detrend
 * or window that is neither value, a scale or min_power that is not finite, min_power < 0, chunk_steps < 0, all four outputs
 * NULL, out_amp set with nfreq = 0, an input or out_amp not aligned to 8 bytes, another output not aligned to 4, buffers that
 * overlap, a byte count that does not fit size_t.  Every refusal happens before anything is enqueued and leaves the outputs
 * untouched.
 *
 * Conventions are fdoct_doppler.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across the
 * boundary.  With device memory on both sides the call enqueues on the handle's stream and returns without a synchronisation;
 * host memory on either side goes through device buffers the handle owns and the call synchronises.  The calls change nothing
 * a later fdoct_process* reads.
 *
 * The entry points ship in libfdoct_vibro.so, an add-on library over libfdoct_hip.so (link both).
 */
#ifndef FDOCT_VIBRO_H
#define FDOCT_VIBRO_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { FDOCT_VIBRO_RECT = 0, FDOCT_VIBRO_HANN = 1 } fdoct_vibro_window;

#define FDOCT_VIBRO_MAX_FREQ 8

typedef struct {
  int ref;          /* 0: no reference surface */
  int ref_first;    /* first depth of the reference sum */
  int ref_count;    /* depths of the reference sum; 0: up to depths */
  int detrend;      /* 0: the mean is removed; 1: the least-squares line */
  int window;       /* fdoct_vibro_window */
  int nfreq;        /* 0 .. 8 */
  double freq[FDOCT_VIBRO_MAX_FREQ];  /* cycles per frame, each in (0, 0.5] */
  double scale;     /* radians to the caller's unit: lambda0 / (4 pi n) gives displacement */
  double min_power; /* > 0: out_amp, out_rms and out_drift are 0 where the mean power lies below it */
  int chunk_steps;  /* 0: the plan's rule */
} fdoct_vibro_params;

typedef struct {
  int chunk_steps;          /* steps a chunk takes (the last one may take fewer) */
  int chunks;
  long long workgroups;     /* of the series pass */
  size_t workspace_bytes;   /* reference phasors, chunk partials and tables together */
} fdoct_vibro_info;

int fdoct_vibro_plan(const fdoct_vibro_params* params, int nframes, int ascans, int depths, fdoct_vibro_info* info);

int fdoct_vibro(fdoct_handle h, const float* re_im, fdoct_memspace space, int nframes, int ascans, int depths,
                const fdoct_vibro_params* params, float* out_amp, float* out_rms, float* out_drift, float* out_power,
                fdoct_memspace out_space);

int fdoct_process_vibro(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                        const fdoct_vibro_params* params, float* out_amp, float* out_rms, float* out_drift, float* out_power,
                        fdoct_memspace out_space);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_VIBRO_H */
