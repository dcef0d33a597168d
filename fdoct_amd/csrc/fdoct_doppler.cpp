// fdoct_doppler.cpp -- the extern "C" entry points of include/fdoct_doppler.h (libfdoct_doppler.so): phase-resolved Doppler from
// complex A-scans.  The kernels are fdoct_doppler.hip's; the chain in front of fdoct_process_doppler is the core library's
// (fdoct_route.cpp: enqueue_complex), called as fdoct_complex.cpp calls it.  What is this file's own is the calls' arguments: the
// parameters' refusals, and pairs, frames and outputs in host or device memory planned as fdoct_complex.cpp plans its.
#include "../../include/fdoct_doppler.h"

#include "fdoct_capture_plan.h"
#include "fdoct_doppler_kernels.h"

using namespace fdoct_impl;

namespace {

// What both entry points decide from the parameters and the images' shape: the refusals, then the kernels' arguments without
// their pointers.  h may be null (fdoct_doppler_size).
int plan_doppler(fdoct_ctx* h, const char* fn, const fdoct_doppler_params* p, int nframes, int ascans, int depths, fdoct::DopplerArgs* a) {
  const std::string f(fn);
  if (!p) return fail(h, FDOCT_ERR_INVALID, f + ": no parameters");
  if (nframes < 1 || ascans < 1 || depths < 1) return fail(h, FDOCT_ERR_INVALID, f + ": bad image size");
  if (p->axis != FDOCT_DOPPLER_ASCANS && p->axis != FDOCT_DOPPLER_FRAMES) return fail(h, FDOCT_ERR_INVALID, f + ": bad axis");
  if (p->win_ascans < 1 || p->win_ascans > fdoct::kDopMaxWin || p->win_depths < 1 || p->win_depths > fdoct::kDopMaxWin)
    return fail(h, FDOCT_ERR_INVALID, f + ": win_ascans and win_depths must be 1..32");
  if (p->lag < 1) return fail(h, FDOCT_ERR_INVALID, f + ": lag must be at least 1");
  if (!fdoct::doppler_pairs(p->axis, p->lag, nframes, ascans, &a->pair_images, &a->pair_rows))
    return fail(h, FDOCT_ERR_INVALID, f + ": the lag leaves no pair");
  if (p->bulk) {
    if (p->bulk_first < 0 || p->bulk_first >= depths || p->bulk_count < 0 || p->bulk_count > depths - p->bulk_first)
      return fail(h, FDOCT_ERR_INVALID, f + ": the bulk range must lie in [0, depths)");
  }
  if (!std::isfinite(p->scale) || !std::isfinite(p->min_power) || p->min_power < 0.0)
    return fail(h, FDOCT_ERR_INVALID, f + ": scale and min_power must be finite, min_power not negative");
  a->ascans = ascans, a->depths = depths;
  a->partner = (long long)p->lag * depths * (p->axis == FDOCT_DOPPLER_FRAMES ? (long long)ascans : 1LL);
  a->wa = p->win_ascans, a->wd = p->win_depths;
  a->use_bulk = p->bulk ? 1 : 0;
  a->bulk_first = p->bulk ? p->bulk_first : 0;
  a->bulk_count = !p->bulk ? 0 : p->bulk_count ? p->bulk_count : depths - p->bulk_first;
  a->scale = (float)p->scale, a->min_power = (float)p->min_power;
  return FDOCT_OK;
}

// The outputs' sizes and alignment; *floats is one float image batch (out_phase, out_power; out_corr is twice that).
int check_outputs(fdoct_ctx* h, const char* fn, const fdoct::DopplerArgs& a, const float* out_phase, const float* out_corr, const float* out_power,
                  size_t* bytes) {
  const std::string f(fn);
  if (!out_phase && !out_corr && !out_power) return fail(h, FDOCT_ERR_INVALID, f + ": no output");
  size_t bins = 0;
  if (__builtin_mul_overflow((size_t)a.pair_images * (size_t)a.pair_rows, (size_t)a.depths, &bins) || bins > ((size_t)1 << 40))
    return fail(h, FDOCT_ERR_INVALID, f + ": the batch is too large");
  *bytes = bins * sizeof(float);
  if (reinterpret_cast<uintptr_t>(out_corr) % sizeof(float2))
    return fail(h, FDOCT_ERR_INVALID, f + ": out_corr must be aligned to one (re, im) pair (8 bytes)");
  if (reinterpret_cast<uintptr_t>(out_phase) % sizeof(float) || reinterpret_cast<uintptr_t>(out_power) % sizeof(float))
    return fail(h, FDOCT_ERR_INVALID, f + ": out_phase and out_power must be aligned to 4 bytes");
  if (overlap(out_phase, *bytes, out_corr, 2 * *bytes) || overlap(out_phase, *bytes, out_power, *bytes) || overlap(out_corr, 2 * *bytes, out_power, *bytes))
    return fail(h, FDOCT_ERR_INVALID, f + ": the outputs overlap");
  return FDOCT_OK;
}

}  // namespace

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_doppler_size(const fdoct_doppler_params* params, int nframes, int ascans, int depths, int* pair_images, int* pair_rows) try {
  if (!pair_images || !pair_rows) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_doppler_size: no output");
  fdoct::DopplerArgs a;
  if (int rc = plan_doppler(nullptr, "fdoct_doppler_size", params, nframes, ascans, depths, &a)) return rc;
  *pair_images = a.pair_images, *pair_rows = a.pair_rows;
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_doppler(fdoct_handle h, const float* re_im, fdoct_memspace space, int nframes, int ascans, int depths,
                  const fdoct_doppler_params* params, float* out_phase, float* out_corr, float* out_power, fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!re_im || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_doppler: bad arguments");
  if (reinterpret_cast<uintptr_t>(re_im) % sizeof(float2))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_doppler: re_im must be aligned to one (re, im) pair (8 bytes)");
  fdoct::DopplerArgs a;
  if (int rc = plan_doppler(h, "fdoct_doppler", params, nframes, ascans, depths, &a)) return rc;
  size_t bytes = 0, pairs = 0, in_bytes = 0;
  if (int rc = check_outputs(h, "fdoct_doppler", a, out_phase, out_corr, out_power, &bytes)) return rc;
  if (__builtin_mul_overflow((size_t)nframes * (size_t)ascans, (size_t)depths, &pairs) || pairs > ((size_t)1 << 40))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_doppler: the batch is too large");
  in_bytes = pairs * sizeof(float2);
  if (space == out_space && (overlap(re_im, in_bytes, out_phase, bytes) || overlap(re_im, in_bytes, out_corr, 2 * bytes) || overlap(re_im, in_bytes, out_power, bytes)))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_doppler: input and output buffers overlap");
  DEVICE_SCOPE(h);
  // every reservation before anything is enqueued: the staged arguments, the bulk phasors
  StagePlan sp;
  const int in = sp.in(re_im, space, in_bytes);
  const int ph = sp.out(out_phase, out_space, bytes), co = sp.out(out_corr, out_space, 2 * bytes), pw = sp.out(out_power, out_space, bytes);
  if (int rc = stage_reserve(h, &sp)) return rc;
  if (a.use_bulk) {
    if (int rc = h->ws_dop_bulk.reserve(h, (size_t)a.pair_images * a.pair_rows * sizeof(float2))) return rc;
  }
  a.x = sp.dev<const float2>(in), a.bulk = h->ws_dop_bulk;
  a.out_phase = sp.dev<float>(ph), a.out_corr = sp.dev<float2>(co), a.out_power = sp.dev<float>(pw);
  fdoct::doppler_plan_launch(&a, h->num_cu);
  if (int rc = stage_upload(h, sp)) return rc;
  HIP_TRY(h, fdoct::launch_doppler(a, h->stream));
  return stage_finish(h, sp);
} FDOCT_CATCH(h)

int fdoct_process_doppler(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                          const fdoct_doppler_params* params, float* out_phase, float* out_corr, float* out_power, fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!frames || nframes < 1 || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_process_doppler: bad arguments");
  fdoct::DopplerArgs a;
  if (int rc = plan_doppler(h, "fdoct_process_doppler", params, nframes, h->H, h->D, &a)) return rc;
  size_t bytes = 0, pairs = 0, cx_bytes = 0, in_span = 0;
  if (int rc = check_outputs(h, "fdoct_process_doppler", a, out_phase, out_corr, out_power, &bytes)) return rc;
  FramePlan p;
  if (int rc = plan_frames(h, "fdoct_process_doppler", frames, dtype, space, nframes, pitch_bytes, &p)) return rc;
  if (__builtin_mul_overflow((size_t)nframes * (size_t)h->H, (size_t)h->D, &pairs) || __builtin_mul_overflow(pairs, sizeof(float2), &cx_bytes) ||
      __builtin_mul_overflow(p.pitch, (size_t)p.raw_h * (size_t)nframes, &in_span))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_process_doppler: the batch is too large");
  if (space == out_space && (overlap(frames, in_span, out_phase, bytes) || overlap(frames, in_span, out_corr, 2 * bytes) || overlap(frames, in_span, out_power, bytes)))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_process_doppler: frames and output buffers overlap");
  DEVICE_SCOPE(h);
  // every refusal and reservation before anything is enqueued: the staged arguments, the chain's pairs, the bulk phasors, then the
  // chain's own checks and its route on the frames where the kernels will read them (a run-time compile happens here)
  const int ph = p.stage.out(out_phase, out_space, bytes), co = p.stage.out(out_corr, out_space, 2 * bytes), pw = p.stage.out(out_power, out_space, bytes);
  if (int rc = stage_reserve(h, &p.stage)) return rc;
  if (int rc = h->ws_cx.reserve(h, cx_bytes)) return rc;
  if (a.use_bulk) {
    if (int rc = h->ws_dop_bulk.reserve(h, (size_t)a.pair_images * a.pair_rows * sizeof(float2))) return rc;
  }
  if (int rc = enqueue_complex(h, p.stage.dev<const void>(0), dtype, nframes, p.stage.pitch(0), nullptr)) return rc;
  a.x = h->ws_cx, a.bulk = h->ws_dop_bulk;
  a.out_phase = p.stage.dev<float>(ph), a.out_corr = p.stage.dev<float2>(co), a.out_power = p.stage.dev<float>(pw);
  fdoct::doppler_plan_launch(&a, h->num_cu);
  if (int rc = stage_upload(h, p.stage)) return rc;
  if (int rc = enqueue_complex(h, p.stage.dev<const void>(0), dtype, nframes, p.stage.pitch(0), h->ws_cx)) return rc;
  HIP_TRY(h, fdoct::launch_doppler(a, h->stream));
  return stage_finish(h, p.stage);
} FDOCT_CATCH(h)

}  // extern "C"
