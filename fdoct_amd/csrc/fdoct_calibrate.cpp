// fdoct_calibrate.cpp -- the extern "C" entry points of include/fdoct_calibrate.h: BscanDark's calibration (BscanDark.cpp:996,
// 1005-1222) over the kernels of fdoct_calibrate.hip, the capture's accumulation (fdoct_capture.hip) and lpfilter
// (fdoct_lowpass.hip).  A capture is one sequence of launches on the handle's stream -- accumulate, row min / max and scale, plane
// min / max and scale or the division, lpfilter -- and its frame comes down only where the handle's host mirror (RefFrame) or the
// caller asks for it.  Frames are planned as fdoct_capture_reference plans them (fdoct_capture_plan.h).
#include "../../include/fdoct_calibrate.h"

#include "fdoct_calibrate_kernels.h"
#include "fdoct_capture_plan.h"

using namespace fdoct_impl;

namespace {

constexpr double kCapLo = 0.0001, kCapHi = 1.0;  // the limits of both normalisations of a capture (BscanDark.cpp:1056-1061)

int reserve_minmax(fdoct_ctx* h, int rows, int W, bool per_row) {
  return h->ws_cal_mm.reserve(h, fdoct::minmax_shape(rows, W, per_row, h->num_cu).ws_doubles * sizeof(double));
}

}  // namespace

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_normalize_rows_minmax(fdoct_handle h, const double* y, fdoct_memspace space, int rows, int width, size_t pitch_bytes,
                                double lo, double hi, int per_row, double* out, fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!y || !out || !valid_mem(space) || !valid_mem(out_space) || rows < 1 || width < 1)
    return fail(h, FDOCT_ERR_INVALID, "fdoct_normalize_rows_minmax: bad arguments");
  const size_t row = sizeof(double) * (size_t)width;
  const size_t pitch = pitch_bytes ? pitch_bytes : row;
  if (pitch < row) return fail(h, FDOCT_ERR_INVALID, "fdoct_normalize_rows_minmax: pitch smaller than a row");
  if (pitch % sizeof(double) || reinterpret_cast<uintptr_t>(y) % sizeof(double) || reinterpret_cast<uintptr_t>(out) % sizeof(double))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_normalize_rows_minmax: rows and pitch must be aligned to one double (8 bytes)");
  size_t span = 0;
  if (__builtin_mul_overflow(pitch, (size_t)rows - 1, &span) || __builtin_add_overflow(span, row, &span))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_normalize_rows_minmax: the rows' sizes do not fit size_t");
  if (y != out && overlap(y, span, out, span))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_normalize_rows_minmax: y and out overlap without being the same array");
  DEVICE_SCOPE(h);
  // host rows pass through a packed copy on the device (one, normalised in place, if both sides are host memory); device rows stay
  StagePlan sp;
  const int i = sp.in(y, space, row, (size_t)rows, pitch), o = sp.out_on(i, out, out_space, pitch);
  if (int rc = stage_reserve(h, &sp)) return rc;
  if (int rc = reserve_minmax(h, rows, width, per_row != 0)) return rc;
  if (int rc = stage_upload(h, sp)) return rc;
  fdoct::RowsF64 r;
  r.in = sp.dev<const double>(i), r.out = sp.dev<double>(o), r.in_pitch = sp.pitch(i), r.out_pitch = sp.pitch(o), r.rows = rows, r.W = width;
  HIP_TRY(h, fdoct::launch_normalize_minmax(r, per_row != 0, lo, hi, h->ws_cal_mm, h->num_cu, h->stream));
  return stage_finish(h, sp);
} FDOCT_CATCH(h)

int fdoct_calibrate_capture(fdoct_handle h, int slot, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes,
                            size_t pitch_bytes, double* out_host) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (slot < FDOCT_CAL_DARK || slot > FDOCT_CAL_SAMPLE) return fail(h, FDOCT_ERR_INVALID, "fdoct_calibrate_capture: bad slot");
  FramePlan p;
  if (int rc = plan_frames(h, "fdoct_calibrate_capture", frames, dtype, space, nframes, pitch_bytes, &p)) return rc;
  DEVICE_SCOPE(h);
  const bool rowwise = h->cfg.rowwisenormalize != 0, whole = !h->cfg.donotnormalize, lowpass = h->cap_lowpass != 0;
  const size_t count = (size_t)h->H * h->W, bytes = count * sizeof(double), row = sizeof(double) * (size_t)h->W;
  // every reservation before anything is enqueued: the staged frames, the front end's workspaces, the sums, the partials of both
  // normalisations, lpfilter's bins, the frame that becomes the slot, the host copy
  if (int rc = stage_reserve(h, &p.stage)) return rc;
  if (int rc = front_passes(h, p, nullptr)) return rc;
  if (int rc = h->ws_cap_acc.reserve(h, bytes)) return rc;
  if (int rc = rowwise ? reserve_minmax(h, h->H, h->W, true) : FDOCT_OK) return rc;
  if (int rc = whole ? reserve_minmax(h, h->H, h->W, false) : FDOCT_OK) return rc;
  if (int rc = lowpass ? enqueue_lowpass(h, nullptr, 0, nullptr, 0, h->H, h->W) : FDOCT_OK) return rc;
  DevBuf<double>& next = h->ws_cal_next;  // (a buffer of its own, so that a failure below leaves the slot's content where it is)
  if (int rc = next.reserve(h, bytes)) return rc;
  const bool download = out_host || slot == FDOCT_CAL_DARK;
  std::vector<double> v(download ? count : 0);
  if (int rc = stage_upload(h, p.stage)) return rc;
  if (int rc = front_passes(h, p, p.stage.dev<const void>(0))) return rc;
  // the recipe of fdoct_capture_reference's accumulating roles (main:1041-1057, BscanDark.cpp:1056-1074)
  const bool sim = h->cfg.variant == FDOCT_VARIANT_SIM;
  const int movavgn = (!sim && h->cfg.movavgn > 0 && !h->cap_raw) ? h->cfg.movavgn : 0;
  double* const acc = h->ws_cap_acc;
  HIP_TRY(h, fdoct::launch_capture_accumulate(p.cf, movavgn, true, acc, h->num_cu, h->stream));
  fdoct::RowsF64 r;
  r.in = acc, r.out = acc, r.in_pitch = r.out_pitch = row, r.rows = h->H, r.W = h->W;
  if (rowwise) HIP_TRY(h, fdoct::launch_normalize_minmax(r, true, kCapLo, kCapHi, h->ws_cal_mm, h->num_cu, h->stream));
  if (!lowpass) r.out = next;  // the last step writes the slot's frame
  if (whole)
    HIP_TRY(h, fdoct::launch_normalize_minmax(r, false, kCapLo, kCapHi, h->ws_cal_mm, h->num_cu, h->stream));
  else
    HIP_TRY(h, fdoct::launch_divide_rows(r, (double)nframes, h->num_cu, h->stream));
  if (lowpass)
    if (int rc = enqueue_lowpass(h, acc, row, next, row, h->H, h->W)) return rc;
  if (download) HIP_TRY(h, hipMemcpyAsync(v.data(), next, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  // the commit: nothing above changed the handle's state
  if (out_host) std::memcpy(out_host, v.data(), bytes);
  h->d_cal[slot].swap(next);  // (what the slot held is the next capture's buffer)
  h->cal_held[slot] = true;
  if (slot == FDOCT_CAL_DARK) {  // data_yd, as FDOCT_REF_DARK leaves it
    h->yd.v = std::move(v);
    h->yd.rows = h->H;
    invalidate(h);
  }
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_calibrate_compose(fdoct_handle h, double* out_host) try {
  if (!h) return FDOCT_ERR_INVALID;
  for (int s = FDOCT_CAL_DARK; s <= FDOCT_CAL_SAMPLE; s++)
    if (!h->cal_held[s])
      return fail(h, FDOCT_ERR_STATE, "fdoct_calibrate_compose: the dark, reference and sample captures must all be held (fdoct_calibrate_capture)");
  DEVICE_SCOPE(h);
  const size_t count = (size_t)h->H * h->W, bytes = count * sizeof(double);
  if (int rc = h->ws_cap_acc.reserve(h, bytes)) return rc;
  std::vector<double> v(count);
  HIP_TRY(h, fdoct::launch_compose(h->d_cal[FDOCT_CAL_REFERENCE], h->d_cal[FDOCT_CAL_SAMPLE], h->d_cal[FDOCT_CAL_DARK], h->ws_cap_acc, count,
                                   h->num_cu, h->stream));
  HIP_TRY(h, hipMemcpyAsync(v.data(), h->ws_cap_acc, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (out_host) std::memcpy(out_host, v.data(), bytes);
  h->yb.v = std::move(v);  // data_yb, as fdoct_set_background leaves it
  h->yb.rows = h->H;
  invalidate(h);
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_calibrate_state(fdoct_handle h, int held[3]) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!held) return fail(h, FDOCT_ERR_INVALID, "fdoct_calibrate_state: no output");
  for (int s = 0; s < 3; s++) held[s] = h->cal_held[s] ? 1 : 0;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_calibrate_clear(fdoct_handle h) try {
  if (!h) return FDOCT_ERR_INVALID;
  DEVICE_SCOPE(h);
  for (int s = 0; s < 3; s++) {
    h->d_cal[s].release();
    h->cal_held[s] = false;
  }
  h->ws_cal_next.release();
  return FDOCT_OK;
} FDOCT_CATCH(h)

}  // extern "C"
