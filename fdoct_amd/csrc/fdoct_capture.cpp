// fdoct_capture.cpp -- the extern "C" entry points of include/fdoct_capture.h: the handle's background / pi / dark frame
// captured from camera frames (the b / p key handlers, BscanFFT.cpp:1000-1099; BscanDark.cpp:1005-1190) and the per-frame
// min / max of the "Max intensity" line, over the kernels of fdoct_capture.hip.  The sums come back as H x W doubles -- the
// handle keeps its reference frames as host doubles (RefFrame) -- and the normalisations run on them here, in the arithmetic
// of fdoct_host.cpp::normalize_minmax.  With the handle's low-pass option on (include/fdoct_lowpass.h) the normalised doubles go
// back to the device once more, for lpfilter.
#include "../../include/fdoct_capture.h"

#include "fdoct_capture_plan.h"

using namespace fdoct_impl;

namespace {

bool has_frontend(const fdoct_ctx* h) { return h->fe_median > 0 || h->fe_binx > 1 || h->fe_biny > 1; }

}  // namespace

namespace fdoct_impl {  // (declared in fdoct_capture_plan.h: fdoct_calibrate.cpp plans its frames the same way)

int plan_frames(fdoct_ctx* h, const char* fn, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes,
                size_t pitch_bytes, FramePlan* p) {
  const std::string who = std::string(fn) + ": ";
  if (!frames || !valid_mem(space) || nframes < 1) return fail(h, FDOCT_ERR_INVALID, who + "bad arguments");
  if (h->colour >= 0) {
    if (int rc = colour_check(h, fn, h->colour, dtype, h->fe_median)) return rc;
    p->colour = true;
  }
  const size_t es = frame_pixel_bytes(h, dtype);
  if (!es) return fail(h, FDOCT_ERR_INVALID, who + "bad dtype");
  p->dtype = dtype, p->nframes = nframes, p->es = es;
  p->frontend = has_frontend(h);
  p->raw_w = h->W * (p->frontend ? h->fe_binx : 1);
  p->raw_h = h->H * (p->frontend ? h->fe_biny : 1);
  p->pitch = pitch_bytes ? pitch_bytes : es * (size_t)p->raw_w;
  if (p->pitch < es * (size_t)p->raw_w) return fail(h, FDOCT_ERR_INVALID, who + "pitch smaller than a row");
  if (!p->colour && (p->pitch % es || reinterpret_cast<uintptr_t>(frames) % es))
    return fail(h, FDOCT_ERR_INVALID, who + "frames and pitch must be aligned to one sample");
  if (p->frontend && !p->colour) {
    if (dtype != FDOCT_U8 && dtype != FDOCT_U16)
      return fail(h, FDOCT_ERR_UNSUPPORTED, who + "the front end (median / binning) takes the camera's 8- or 16-bit frames");
    if (h->fe_median == 7 && dtype == FDOCT_U16)
      return fail(h, FDOCT_ERR_INVALID, who + "a 7x7 median exists for 8-bit frames only (cv::medianBlur)");
  }
  p->stage.in(frames, space, es * p->raw_w, (size_t)p->raw_h * nframes, p->pitch);
  return FDOCT_OK;
}

// What stands between the frames on the device (the caller's, or the plan's item 0 after its upload) and the kernels: the colour
// stage or the front end.  src null: their checks and workspaces only, and p.cf gets its shape -- nothing is enqueued.
int front_passes(fdoct_ctx* h, FramePlan& p, const void* src) {
  size_t pitch = p.stage.pitch(0);
  fdoct_dtype dt = p.dtype;
  void* o = nullptr;
  if (p.colour) {  // webcam:1015-1038 ahead of everything, the median / binning with it
    if (int rc = run_colour(h, src, p.nframes, p.raw_w, p.raw_h, pitch, h->colour, h->fe_median, h->fe_binx, h->fe_biny, &o, &pitch)) return rc;
    if (h->colour == 3) dt = FDOCT_F64;
  } else if (p.frontend) {
    if (int rc = run_frontend(h, src, kernel_dtype(p.dtype), p.nframes, p.raw_w, p.raw_h, pitch, h->fe_median, h->fe_binx, h->fe_biny, &o, &pitch))
      return rc;
  }
  p.cf.frames = o ? o : src, p.cf.dt = dt, p.cf.pitch = pitch, p.cf.nframes = p.nframes, p.cf.H = h->H, p.cf.W = h->W;
  return FDOCT_OK;
}

}  // namespace fdoct_impl

namespace {

RefFrame* ref_of(fdoct_ctx* h, int role) {
  return role == FDOCT_REF_BACKGROUND ? &h->yb : role == FDOCT_REF_PI ? &h->yp : role == FDOCT_REF_DARK ? &h->yd : nullptr;
}

}  // namespace

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_capture_reference(fdoct_handle h, int role, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes,
                            size_t pitch_bytes, double* out_host) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (role < FDOCT_REF_BACKGROUND || role > FDOCT_REF_NONE) return fail(h, FDOCT_ERR_INVALID, "fdoct_capture_reference: bad role");
  FramePlan p;
  if (int rc = plan_frames(h, "fdoct_capture_reference", frames, dtype, space, nframes, pitch_bytes, &p)) return rc;
  const bool sim = h->cfg.variant == FDOCT_VARIANT_SIM;
  // sim:803-825: data_yb / data_yp are the binned frame itself
  const bool plain_copy = sim && (role == FDOCT_REF_BACKGROUND || role == FDOCT_REF_PI);
  if ((role == FDOCT_REF_PI || plain_copy) && nframes != 1)
    return fail(h, FDOCT_ERR_INVALID, "fdoct_capture_reference: this role takes exactly one frame (main:1081, sim:803-825)");
  DEVICE_SCOPE(h);
  const size_t count = (size_t)h->H * h->W;
  if (int rc = stage_reserve(h, &p.stage)) return rc;
  if (int rc = front_passes(h, p, nullptr)) return rc;
  if (int rc = h->ws_cap_acc.reserve(h, count * sizeof(double))) return rc;
  if (int rc = h->cap_lowpass ? enqueue_lowpass(h, nullptr, 0, nullptr, 0, h->H, h->W) : FDOCT_OK) return rc;
  if (int rc = stage_upload(h, p.stage)) return rc;  // (no stage_finish: no staged output, and the call synchronises itself)
  if (int rc = front_passes(h, p, p.stage.dev<const void>(0))) return rc;
  // saveinterferograms (fdoct_set_capture_options): the binned frames are accumulated as they are (main:1024)
  const int movavgn = (!sim && h->cfg.movavgn > 0 && !h->cap_raw) ? h->cfg.movavgn : 0;
  const bool accumulates = !(role == FDOCT_REF_PI || plain_copy);  // (the p key copies one data_y, main:1081)
  HIP_TRY(h, fdoct::launch_capture_accumulate(p.cf, movavgn, accumulates, h->ws_cap_acc, h->num_cu, h->stream));
  std::vector<double> v(count);
  HIP_TRY(h, hipMemcpyAsync(v.data(), h->ws_cap_acc, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (plain_copy) {
    // sim:803-825: the frame as it is
  } else if (role == FDOCT_REF_PI) {  // main:1093-1096
    if (h->cfg.rowwisenormalize) normalize_rows(v.data(), h->H, h->W, 0, 1);
    if (!h->cfg.donotnormalize) normalize_minmax(v.data(), count, 0, 1);
  } else {  // main:1050-1057, BscanDark.cpp:1056-1063
    if (h->cfg.rowwisenormalize) normalize_rows(v.data(), h->H, h->W, 0.0001, 1);
    if (!h->cfg.donotnormalize)
      normalize_minmax(v.data(), count, 0.0001, 1);
    else
      for (double& x : v) x = x / nframes;
    if (h->cap_lowpass) {  // lowpassfilter: lpfilter on the finished frame (BscanDark.cpp:1070-1074), in place on the device
      const size_t row = sizeof(double) * (size_t)h->W;
      HIP_TRY(h, hipMemcpyAsync(h->ws_cap_acc, v.data(), count * sizeof(double), hipMemcpyHostToDevice, h->stream));
      if (int rc = enqueue_lowpass(h, h->ws_cap_acc, row, h->ws_cap_acc, row, h->H, h->W)) return rc;
      HIP_TRY(h, hipMemcpyAsync(v.data(), h->ws_cap_acc, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
  }
  if (out_host) std::memcpy(out_host, v.data(), count * sizeof(double));
  if (RefFrame* dst = ref_of(h, role)) {  // the commit: nothing above changed the handle's state
    dst->v = std::move(v);
    dst->rows = h->H;
    invalidate(h);
  }
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_get_reference(fdoct_handle h, int role, double* out, size_t cap_doubles, int* rows) try {
  if (!h) return FDOCT_ERR_INVALID;
  const RefFrame* ref = ref_of(h, role);
  if (!ref) return fail(h, FDOCT_ERR_INVALID, "fdoct_get_reference: role must be background, pi or dark");
  if (!out && !rows) return fail(h, FDOCT_ERR_INVALID, "fdoct_get_reference: no output");
  if (rows) *rows = ref->rows;
  if (out) {
    if (cap_doubles < ref->v.size()) return fail(h, FDOCT_ERR_INVALID, "fdoct_get_reference: buffer smaller than rows * width doubles");
    if (!ref->v.empty()) std::memcpy(out, ref->v.data(), ref->v.size() * sizeof(double));
  }
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_frame_minmax(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes,
                       size_t pitch_bytes, double* out_min, double* out_max, fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!valid_mem(out_space) || (!out_min && !out_max)) return fail(h, FDOCT_ERR_INVALID, "fdoct_frame_minmax: no output");
  if (nframes > 65535) return fail(h, FDOCT_ERR_INVALID, "fdoct_frame_minmax: at most 65535 frames per call");
  FramePlan p;
  if (int rc = plan_frames(h, "fdoct_frame_minmax", frames, dtype, space, nframes, pitch_bytes, &p)) return rc;
  DEVICE_SCOPE(h);
  const size_t n = (size_t)nframes;
  const int lo = p.stage.out(out_min, out_space, n * sizeof(double)), hi = p.stage.out(out_max, out_space, n * sizeof(double));
  if (int rc = stage_reserve(h, &p.stage)) return rc;
  if (int rc = front_passes(h, p, nullptr)) return rc;  // (the partials follow from the frames' shape)
  if (int rc = h->ws_cap_mm.reserve(h, fdoct::frame_minmax_partials(p.cf, h->num_cu) * sizeof(double))) return rc;
  if (int rc = stage_upload(h, p.stage)) return rc;
  if (int rc = front_passes(h, p, p.stage.dev<const void>(0))) return rc;
  HIP_TRY(h, fdoct::launch_frame_minmax(p.cf, h->ws_cap_mm, p.stage.dev<double>(lo), p.stage.dev<double>(hi), h->num_cu, h->stream));
  return stage_finish(h, p.stage);
} FDOCT_CATCH(h)

int fdoct_normalize_minmax(double* y, size_t n, double lo, double hi) try {
  if (n > 0 && !y) return FDOCT_ERR_INVALID;
  normalize_minmax(y, n, lo, hi);
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

}  // extern "C"
