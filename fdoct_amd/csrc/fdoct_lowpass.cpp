// fdoct_lowpass.cpp -- the extern "C" entry points of include/fdoct_lowpass.h: BscanDark's lpfilter (BscanDark.cpp:119-167) on
// rows of doubles over the kernel of fdoct_lowpass.hip, and the two switches fdoct_capture_reference reads (fdoct_capture.cpp).
#include "../../include/fdoct_lowpass.h"

#include "fdoct_capture_kernels.h"
#include "fdoct_ctx.h"

using namespace fdoct_impl;

namespace fdoct_impl {

int enqueue_lowpass(fdoct_ctx* h, const double* d_in, size_t in_pitch, double* d_out, size_t out_pitch, int rows, int W) {
  const fdoct::LowpassShape s = fdoct::lowpass_shape(rows, W, h->num_cu);
  if (s.ws_doubles)
    if (int rc = h->ws_lp_bins.reserve(h, s.ws_doubles * sizeof(double))) return rc;
  if (!d_in) return FDOCT_OK;
  HIP_TRY(h, fdoct::launch_lowpass_rows(d_in, in_pitch, d_out, out_pitch, rows, W, h->ws_lp_bins, h->num_cu, h->stream));
  return FDOCT_OK;
}

}  // namespace fdoct_impl

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_set_capture_options(fdoct_handle h, int lowpass, int raw_accumulate) try {
  if (!h) return FDOCT_ERR_INVALID;
  h->cap_lowpass = lowpass != 0;
  h->cap_raw = raw_accumulate != 0;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_get_capture_options(fdoct_handle h, int* lowpass, int* raw_accumulate) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!lowpass && !raw_accumulate) return fail(h, FDOCT_ERR_INVALID, "fdoct_get_capture_options: no output");
  if (lowpass) *lowpass = h->cap_lowpass;
  if (raw_accumulate) *raw_accumulate = h->cap_raw;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_lowpass_rows(fdoct_handle h, const double* in, fdoct_memspace in_space, int rows, int width, size_t pitch_bytes,
                       double* out, fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!in || !out || !valid_mem(in_space) || !valid_mem(out_space) || rows < 1 || width < 1)
    return fail(h, FDOCT_ERR_INVALID, "fdoct_lowpass_rows: bad arguments");
  const size_t row = sizeof(double) * (size_t)width;
  const size_t pitch = pitch_bytes ? pitch_bytes : row;
  if (pitch < row) return fail(h, FDOCT_ERR_INVALID, "fdoct_lowpass_rows: pitch smaller than a row");
  if (pitch % sizeof(double) || reinterpret_cast<uintptr_t>(in) % sizeof(double) || reinterpret_cast<uintptr_t>(out) % sizeof(double))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_lowpass_rows: rows and pitch must be aligned to one double");
  DEVICE_SCOPE(h);
  // host rows pass through a packed copy on the device (one, filtered in place, if both sides are host memory); device rows stay
  StagePlan sp;
  const int i = sp.in(in, in_space, row, (size_t)rows, pitch), o = sp.out_on(i, out, out_space, pitch);
  if (int rc = stage_reserve(h, &sp)) return rc;
  if (int rc = enqueue_lowpass(h, nullptr, 0, nullptr, 0, rows, width)) return rc;
  if (int rc = stage_upload(h, sp)) return rc;
  if (int rc = enqueue_lowpass(h, sp.dev<const double>(i), sp.pitch(i), sp.dev<double>(o), sp.pitch(o), rows, width)) return rc;
  return stage_finish(h, sp);
} FDOCT_CATCH(h)

}  // extern "C"
