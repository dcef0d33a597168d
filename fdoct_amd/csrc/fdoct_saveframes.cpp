// fdoct_saveframes.cpp -- the extern "C" entry points of include/fdoct_saveframes.h: the raw-magnitudes switch of the chain
// (fdoct_ctx::raw_mag, read by fdoct_route.cpp's kernel_eps and check_call) and the per-frame saves while averaging
// (BscanFFT.cpp:1197-1240, 1360-1377) over the kernels of fdoct_saveframes.hip.
#include "../../include/fdoct_saveframes.h"

#include "fdoct_ctx.h"
#include "fdoct_saveframes_kernels.h"

using namespace fdoct_impl;

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_set_raw_magnitudes(fdoct_handle h, int on) try {
  if (!h) return FDOCT_ERR_INVALID;
  h->raw_mag = on != 0;  // a kernel argument only: no table, plan or route depends on it
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_get_raw_magnitudes(fdoct_handle h) try { return h ? (h->raw_mag ? 1 : 0) : FDOCT_ERR_INVALID; } FDOCT_CATCH(h)

int fdoct_saveframes(fdoct_handle h, const float* frames, fdoct_memspace mem, fdoct_layout in_layout, int nframes, int depths,
                     int ascans, unsigned char* out_gray, int averages, float* out_bscan, float* out_db, fdoct_layout out_layout,
                     fdoct_memspace out_mem) try {
  // what needs no handle first: a bad call is refused the same way with and without a device
  if (!frames || !valid_mem(mem) || !valid_mem(out_mem) || !valid_layout(in_layout) || !valid_layout(out_layout) || nframes < 1 ||
      depths < 1 || ascans < 1 || averages < 0)
    return fail(h, FDOCT_ERR_INVALID, "fdoct_saveframes: bad arguments");
  const bool fold = out_bscan || out_db;
  if (!out_gray && !fold) return fail(h, FDOCT_ERR_INVALID, "fdoct_saveframes: no output requested");
  if (fold && averages == 0) return fail(h, FDOCT_ERR_INVALID, "fdoct_saveframes: averages = 0 means no fold: out_bscan and out_db must be NULL");
  if (averages && nframes % averages) return fail(h, FDOCT_ERR_INVALID, "fdoct_saveframes: nframes must be a multiple of averages");
  const size_t count = (size_t)depths * (size_t)ascans;
  if (count > ((size_t)1 << 40) || (size_t)nframes > ((size_t)1 << 40) / count)
    return fail(h, FDOCT_ERR_INVALID, "fdoct_saveframes: the batch is too large");
  if (!h) return FDOCT_ERR_INVALID;
  if (fold && h->cfg.variant == FDOCT_VARIANT_SIM)
    return fail(h, FDOCT_ERR_UNSUPPORTED, "fdoct_saveframes: the sim variant copies and does not accumulate (sim:936-947): no fold");
  const size_t groups = fold ? (size_t)(nframes / averages) : 0;
  const size_t in_bytes = count * nframes * sizeof(float), gray_bytes = count * nframes, fold_bytes = count * groups * sizeof(float);
  if (overlap(out_gray, gray_bytes, out_bscan, fold_bytes) || overlap(out_gray, gray_bytes, out_db, fold_bytes) ||
      overlap(out_bscan, fold_bytes, out_db, fold_bytes) ||
      (mem == out_mem && (overlap(frames, in_bytes, out_gray, gray_bytes) || overlap(frames, in_bytes, out_bscan, fold_bytes) ||
                          overlap(frames, in_bytes, out_db, fold_bytes))))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_saveframes: input and output buffers overlap");
  DEVICE_SCOPE(h);

  StagePlan sp;
  const int in = sp.in(frames, mem, in_bytes);
  const int gray = sp.out(out_gray, out_mem, gray_bytes);
  const int mag = sp.out(out_bscan, out_mem, fold_bytes), db = sp.out(out_db, out_mem, fold_bytes);
  if (int rc = stage_reserve(h, &sp)) return rc;
  fdoct::SaveFramesArgs a;
  a.in = sp.dev<const float>(in), a.gray = sp.dev<unsigned char>(gray), a.out_bscan = sp.dev<float>(mag), a.out_db = sp.dev<float>(db);
  a.count = (long long)count, a.nframes = nframes, a.depths = depths, a.ascans = ascans;
  a.group = fold ? averages : 1;
  a.in_transposed = in_layout == FDOCT_LAYOUT_TRANSPOSED_DxH, a.out_transposed = out_layout == FDOCT_LAYOUT_TRANSPOSED_DxH;
  a.dc_mask = h->cfg.dc_mask != 0;
  a.eps = 0.00001;  // main:1222, the double the reference adds (a sim handle has no fold)
  fdoct::saveframes_plan_launch(&a, h->num_cu);
  if (a.gray) {
    if (int rc = h->d_sf_part.reserve(h, fdoct::saveframes_part_doubles(a) * sizeof(double))) return rc;
    a.part = h->d_sf_part;
  }
  if (int rc = stage_upload(h, sp)) return rc;
  HIP_TRY(h, fdoct::launch_saveframes(a, h->stream));
  return stage_finish(h, sp);
} FDOCT_CATCH(h)

}  // extern "C"
