/*
 * fdoct_enface.h -- en-face projection of B-scan volumes: the C-scan of a volume of positions x A-scans x depths floats, one image
 * of positions x A-scans per depth slab -- the mean, the maximum and the depth of the maximum -- over slabs that are fixed or follow
 * the tissue surface, on the device, in one read of the slabs' depths.
 *
 * The add-on stages (fdoct_angio.h, fdoct_ssada.h, fdoct_cxavg.h, fdoct_doppler.h) and the chain itself end in volumes; this is the
 * stage that reduces a volume along depth to what is looked at.
 *
 * Input: V[p][r][b], positions x ascans x depths floats, row-major, 4-byte aligned -- what fdoct_angio, fdoct_ssada, fdoct_cxavg or
 * fdoct_process_async, row-major H x D, write.  An optional structure volume S of the same shape feeds the surface (S angiography's
 * out_power while V is its out_decorr, say); NULL means S = V.
 *
 * 1. Surface (surface != 0), per A-scan of S.  The search range is [s0, s1) = [search_first, search_first + search_count),
 *    search_count = 0 meaning up to depths; the candidates are b in [s0, s1 - smooth].  B[b] = sum_{j < smooth} S[b + j], in float,
 *    summed in increasing j and from scratch for every b (no running sums).  Mode 1 (absolute): thr = (float)threshold (float)smooth.
 *    Mode 2 (relative): thr = (float)threshold max_b B[b], threshold in (0, 1]; the maximum starts from -infinity and is replaced
 *    on B[b] > m.  z0[p][r] is the smallest candidate with B[b] >= thr, or -1 where there is none: a row of NaN gives -1.
 * 2. Lateral median.  z[p][r] is the lower median of the valid (>= 0) z0[p][r'], r' in [r - (median - 1) / 2, r + (median - 1) / 2]
 *    within [0, ascans): element (k - 1) / 2 of the k valid values in ascending order, and -1 where k = 0.  The median never crosses
 *    positions.  An A-scan without a crossing takes its neighbours' surface; this is intended.
 * 3. Slabs.  Slab s of an A-scan is [z + slab_first[s], z + slab_first[s] + slab_count[s]) within [0, depths), n depths remaining.
 *    With surface = 0, z = 0.  Slabs may overlap.
 * 4. Outputs, each optional (NULL), at least one required:
 *        out_mean    [nslabs][positions][ascans] floats   (sum of V over the slab) / (float)n
 *        out_max     [nslabs][positions][ascans] floats   the maximum: from the slab's first depth, replaced on V[b] > m
 *        out_argmax  [nslabs][positions][ascans] int32    the absolute depth of the first maximum
 *        out_surface [positions][ascans] int32            z; refused with surface = 0
 *    Where z = -1 or n = 0, mean and max are 0 and argmax is -1.  A NaN inside a slab makes that A-scan's results for that slab
 *    unspecified; it changes no other A-scan's bits and no other slab's.
 *    A requested subset of the outputs holds the same bits as all of them together; what nothing reads is not computed.
 *
 * Arithmetic.  All of it is float; no floating-point atomics.  A slab's sum is made of 64 partials: partial l sums, from 0 and in
 * increasing b, the slab's depths with (b mod 256) / 4 == l (integer division: depths 4 l .. 4 l + 3 of every 256).  The partials
 * are then combined by the butterfly p[l] += p[l + k], k = 32, 16, 8, 4, 2, 1, and p[0] is the sum.  The order is a function of the
 * clipped slab and the depth index alone: it depends neither on the grid, the workgroup or the pass that computes the A-scan, nor on
 * the volume's address, nor on which outputs the call asks for, which other slabs it names or what other positions hold.  A tie of the
 * maximum resolves to the smaller depth in every reduction step.  Two runs give the same bits.
 *
 * fdoct_enface_plan accepts or refuses a call and reports its geometry: pure, no handle.
 * fdoct_enface runs the stage on volumes in host or device memory; it reads nothing of the handle's geometry.
 * fdoct_process_enface is fdoct_process_async's chain, row-major, followed by the stage, for camera frames of the handle's geometry:
 * positions = nframes / averages, ascans = height, depths = numdisplaypoints, S = V; source 0 projects the linear B-scan, 1 its dB.
 * The volume stays in a workspace the handle owns.  Its kernel families and its refusals are the chain's (FDOCT_ERR_STATE without
 * a background; FDOCT_ERR_INVALID for dB with raw magnitudes on), it refuses nframes that is not a multiple of the handle's averages,
 * and FDOCT_ERR_UNSUPPORTED on a handle of the sim variant with averages above 1.  fdoct_last_kernel reports the chain's family.
 *
 * FDOCT_ERR_INVALID: a NULL vol or params, a bad memory space, positions outside 1 .. 65536, ascans or depths < 1, ascans depths
 * > 2^24, surface outside 0 .. 2, smooth outside 1 .. 16, median even or outside 1 .. 15, nslabs outside 1 .. 8, a slab_count < 1;
 * with surface = 0 a slab_first outside [0, depths), out_surface or structure given; with a surface |slab_first| >= depths, a search
 * range outside [0, depths) or shorter than smooth, a threshold that is not finite or, in mode 2, outside (0, 1]; all outputs NULL,
 * a pointer not aligned to 4 bytes, buffers that overlap, a byte count that does not fit size_t, a source other than 0 or 1.  Every
 * refusal and every reservation happens before anything is enqueued and leaves the outputs untouched.
 *
 * Conventions are fdoct_angio.h's: int return codes, fdoct_last_error, the handle's device and stream, no exception across the
 * boundary.  With device memory on both sides the call enqueues on the handle's stream and returns without a synchronisation;
 * host memory on either side goes through device buffers the handle owns and the call synchronises.  The calls change nothing
 * a later fdoct_process* reads.
 *
 * The entry points ship in libfdoct_enface.so, an add-on library over libfdoct_hip.so (link both).
 */
#ifndef FDOCT_ENFACE_H
#define FDOCT_ENFACE_H

#include "fdoct.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDOCT_ENFACE_MAX_SLABS 8
#define FDOCT_ENFACE_MAX_SMOOTH 16
#define FDOCT_ENFACE_MAX_MEDIAN 15

#define FDOCT_ENFACE_SURFACE_NONE 0
#define FDOCT_ENFACE_SURFACE_ABSOLUTE 1
#define FDOCT_ENFACE_SURFACE_RELATIVE 2

#define FDOCT_ENFACE_SOURCE_LINEAR 0
#define FDOCT_ENFACE_SOURCE_DB 1

typedef struct {
  int surface;        /* 0: none (z = 0); 1: absolute threshold; 2: threshold relative to the A-scan's own maximum */
  int search_first;   /* first depth of the surface search */
  int search_count;   /* depths of the surface search; 0: up to depths */
  int smooth;         /* 1 .. 16: depths summed per candidate */
  double threshold;   /* mode 1: per depth, finite; mode 2: in (0, 1] */
  int median;         /* odd, 1 .. 15: A-scans of the lateral median */
  int nslabs;         /* 1 .. 8 */
  int slab_first[FDOCT_ENFACE_MAX_SLABS];   /* relative to z */
  int slab_count[FDOCT_ENFACE_MAX_SLABS];   /* >= 1 */
} fdoct_enface_params;

typedef struct {
  long long ascans;         /* positions x ascans: one wavefront each */
  long long workgroups;     /* of the projection kernel on a card of 256 compute units: min(ceil(ascans / 4), 8 a compute unit); a call takes its own card's count */
  size_t workspace_bytes;   /* the raw surfaces z0 (0 with surface = 0) */
  int read_first;           /* surface = 0: the first depth of the slabs' union ... */
  int read_count;           /* ... and the depths from it to the union's last; of these the call reads the blocks of 256 depths that meet a slab.  0, 0 with a surface */
} fdoct_enface_info;

int fdoct_enface_plan(const fdoct_enface_params* params, int positions, int ascans, int depths, fdoct_enface_info* info);

int fdoct_enface(fdoct_handle h, const float* vol, const float* structure, fdoct_memspace space, int positions, int ascans, int depths,
                 const fdoct_enface_params* params, float* out_mean, float* out_max, int32_t* out_argmax, int32_t* out_surface,
                 fdoct_memspace out_space);

int fdoct_process_enface(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                         int source, const fdoct_enface_params* params, float* out_mean, float* out_max, int32_t* out_argmax,
                         int32_t* out_surface, fdoct_memspace out_space);

#ifdef __cplusplus
}
#endif

#endif /* FDOCT_ENFACE_H */
