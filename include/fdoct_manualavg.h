/*
 * fdoct_manualavg.h -- manual averaging of B-scans (`manualaveraging` / `manualaverages`) on the GPU.
 *
 * Nine programs of the reference carry the same block (BscanFFT.cpp:1399-1444; BscanFFTspinjnt.cpp:2053-2099; the same lines in
 * spin, spinj, peak, webcam and Dark), switched by the ini's manualaveraging and manualaverages (main:371-372, 456-458) and shown
 * in a window of its own, "Bscanm" (main:534-538).  State: manualaccum, a D x H image of doubles that starts at zero (main:933),
 * and manualaccumcount, 0 (main:567).  With m = manualaverages, for every finished linear bscan, in order:
 *   while manualaccumcount < m (1401-1414):  accumulate(bscan, manualaccum); manualaccumcount++;
 *   otherwise (1416-1444):                   manualaccumcount = 0; manualaccum = manualaccum / m; log(manualaccum);
 *                                            bscandispmanual = 20.0 * manualaccum / 2.303; threshold, normalise, u8 and JET
 *                                            (1426-1430: what the display call of fdoct.h does); manualaccum = zeros (1444)
 * -- and the B-scan that arrived at that step is NOT accumulated: it is dropped, so the reference's period is m + 1 images.
 * The branch has no epsilon and no DC mask: the incoming B-scans already carry the chain's epsilon.
 *
 * Here the accumulator is device memory the handle owns, the counter lives in the handle, and one call takes any number of
 * B-scans where they lie: one kernel launch per call adds them in order into running sums held in registers as doubles and,
 * at every position where the recipe emits, writes (float)(acc / m) and / or (float)(20.0 * ln(acc / m) / 2.303) and zeroes the
 * sums.  Sums, the division and the logarithm are evaluated in double in the reference's order; a mean of zero gives -inf, as ln
 * does.  FDOCT_MANUALAVG_KEEP_ALL is an extension: it emits as soon as the m-th image is in, so nothing is dropped.
 *
 * Conventions are fdoct.h's: int return codes, the last-error text, the handle's device and stream, no exception across the
 * boundary.  No kernel, route or plan of the chain changes.  The accumulator is measurement state like the peak holds of
 * fdoct_roi.h: neither the state blob nor a clone of the handle carries it (a clone starts without one).
 *
 * Asynchrony, as in fdoct_roi.h.  With device memory on both sides a call only enqueues on the handle's stream, and the
 * handle's counter advances when the work is enqueued: process_async -> manualavg_add -> display needs no host
 * synchronisation in between.  Host memory on either side goes through device buffers the handle owns and the call
 * synchronises.  Pointers need the alignment of one float only (16-byte loads and stores are used where pointers and count
 * allow them, and give the same bits).
 * Every refusal -- bad arguments, an out_capacity below what the plan says, outputs that overlap the input or each other --
 * happens before anything is enqueued and leaves the accumulator, the counter and every output untouched.
 */
#ifndef FDOCT_MANUALAVG_H
#define FDOCT_MANUALAVG_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  FDOCT_MANUALAVG_REFERENCE = 0, /* period m + 1: the image that arrives when m are in is dropped (main:1416-1444) */
  FDOCT_MANUALAVG_KEEP_ALL = 1   /* period m: emit as soon as the m-th image is in; nothing dropped (extension) */
} fdoct_manualavg_mode;

/* Host arithmetic only, no handle, no GPU: from (manualaverages, mode, accumulated = manualaccumcount) and nbscans more images,
 * how many images are emitted (*emitted, may be NULL) and what the counter is afterwards (*accumulated_after, may be NULL).
 * FDOCT_ERR_INVALID for manualaverages < 1, a bad mode, accumulated outside 0..manualaverages and nbscans < 0. */
int fdoct_manualavg_plan(int manualaverages, int mode, int accumulated, int nbscans, int* emitted, int* accumulated_after);

/* manualaccum = Mat::zeros(...) and manualaccumcount = 0 (main:933, 567): allocates and zeroes the handle's accumulator of
 * `count` doubles in device memory, count = depths * ascans.  A second begin replaces the first; a begin that fails leaves the
 * handle without an accumulator. */
int fdoct_manualavg_begin(fdoct_handle h, int manualaverages, size_t count, int mode);

/* main:1399-1444 for nbscans linear B-scans of `count` floats each, packed, all in `mem`, taken in order.  Every emitted image
 * goes to slot e = 0, 1, .. of out_mean (count floats each: (float)(acc / m), what 1440 saves before its log) and of out_db
 * ((float)(20.0 * ln(acc / m) / 2.303), 1419-1423), both in out_mem; either may be NULL, both NULL only if the call emits
 * nothing.  out_capacity: slots the outputs hold; one below what the plan says for this call is FDOCT_ERR_INVALID.
 * *emitted (may be NULL) = slots written.  Slots past it, and anything behind the last image, are not touched. */
int fdoct_manualavg_add(fdoct_handle h, const float* bscans, fdoct_memspace mem, int nbscans, float* out_mean, float* out_db,
                        fdoct_memspace out_mem, int out_capacity, int* emitted);

/* Each out pointer may be NULL.  *accumulated = manualaccumcount; partial_host receives the running sums (manualaccum: count
 * doubles, host memory; the call then synchronises). */
int fdoct_manualavg_state(fdoct_handle h, int* manualaverages, size_t* count, int* mode, int* accumulated, double* partial_host);

/* Frees the accumulator (destroying the handle does so too); without one it does nothing.  The add and state calls without
 * begin, or after end: FDOCT_ERR_STATE. */
int fdoct_manualavg_end(fdoct_handle h);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_MANUALAVG_H */
