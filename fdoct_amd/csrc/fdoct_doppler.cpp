// fdoct_doppler.cpp -- the extern "C" entry points of include/fdoct_doppler.h (libfdoct_doppler.so): phase-resolved Doppler from
// complex A-scans.  The kernels are fdoct_doppler.hip's; the chain in front of fdoct_process_doppler is the core library's
// (fdoct_route.cpp: enqueue_complex), called in the order fdoct_capture_plan.h's ComplexFront keeps.  What is this file's own is the
// calls' arguments: the parameters' refusals, and pairs, frames and outputs in host or device memory through the staging plan.
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
  int bulk_count = 0;
  if (p->bulk && !depth_range(p->bulk_first, p->bulk_count, depths, &bulk_count))
    return fail(h, FDOCT_ERR_INVALID, f + ": the bulk range must lie in [0, depths)");
  if (!std::isfinite(p->scale) || !std::isfinite(p->min_power) || p->min_power < 0.0)
    return fail(h, FDOCT_ERR_INVALID, f + ": scale and min_power must be finite, min_power not negative");
  a->ascans = ascans, a->depths = depths;
  a->partner = (long long)p->lag * depths * (p->axis == FDOCT_DOPPLER_FRAMES ? (long long)ascans : 1LL);
  a->wa = p->win_ascans, a->wd = p->win_depths;
  a->use_bulk = p->bulk ? 1 : 0;
  a->bulk_first = p->bulk ? p->bulk_first : 0;
  a->bulk_count = bulk_count;
  a->scale = (float)p->scale, a->min_power = (float)p->min_power;
  return FDOCT_OK;
}

// The outputs' presence, sizes, alignment and overlaps among themselves and with the input (`in_name` in the message: its first
// byte and size; null where the memory spaces differ); *floats is one float image batch (out_phase, out_power; out_corr is twice that).
int check_outputs(fdoct_ctx* h, const char* fn, const fdoct::DopplerArgs& a, const char* in_name, const void* in, size_t in_bytes, const float* out_phase,
                  const float* out_corr, const float* out_power, size_t* floats) {
  const std::string f(fn);
  if (!out_phase && !out_corr && !out_power) return fail(h, FDOCT_ERR_INVALID, f + ": no output");
  size_t bins = 0;
  if (__builtin_mul_overflow((size_t)a.pair_images * (size_t)a.pair_rows, (size_t)a.depths, &bins) || bins > ((size_t)1 << 40))
    return fail(h, FDOCT_ERR_INVALID, f + ": the batch is too large");
  *floats = bins * sizeof(float);
  if (reinterpret_cast<uintptr_t>(out_corr) % sizeof(float2))
    return fail(h, FDOCT_ERR_INVALID, f + ": out_corr must be aligned to one (re, im) pair (8 bytes)");
  if (reinterpret_cast<uintptr_t>(out_phase) % sizeof(float) || reinterpret_cast<uintptr_t>(out_power) % sizeof(float))
    return fail(h, FDOCT_ERR_INVALID, f + ": out_phase and out_power must be aligned to 4 bytes");
  const void* const p[3] = {out_phase, out_corr, out_power};
  const size_t nb[3] = {*floats, 2 * *floats, *floats};
  return refuse_overlaps(h, f, in_name, in, in_bytes, p, nb, 3);
}

// What both entry points end with.  sp's item 0 is the input (the pairs, or with `front` the frames of its chain, whose pairs are
// ws_cx's): the outputs join the plan, every reservation, then the copies up, the chain, the kernels, the copies down.
int run_stage(fdoct_ctx* h, StagePlan* sp, ComplexFront* front, fdoct::DopplerArgs a, size_t floats, float* out_phase, float* out_corr, float* out_power,
              fdoct_memspace out_space) {
  DEVICE_SCOPE(h);
  const int ph = sp->out(out_phase, out_space, floats), co = sp->out(out_corr, out_space, 2 * floats), pw = sp->out(out_power, out_space, floats);
  if (int rc = front ? reserve_complex_front(h, front) : stage_reserve(h, sp)) return rc;
  if (a.use_bulk) {
    if (int rc = h->ws_dop_bulk.reserve(h, (size_t)a.pair_images * a.pair_rows * sizeof(float2))) return rc;
  }
  a.x = front ? static_cast<const float2*>(h->ws_cx) : sp->dev<const float2>(0);
  a.bulk = h->ws_dop_bulk;
  a.out_phase = sp->dev<float>(ph), a.out_corr = sp->dev<float2>(co), a.out_power = sp->dev<float>(pw);
  fdoct::doppler_plan_launch(&a, h->num_cu);
  if (int rc = front ? run_complex_front(h, *front) : stage_upload(h, *sp)) return rc;
  HIP_TRY(h, fdoct::launch_doppler(a, h->stream));
  return stage_finish(h, *sp);
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
  size_t floats = 0, pairs = 0;
  if (__builtin_mul_overflow((size_t)nframes * (size_t)ascans, (size_t)depths, &pairs) || pairs > ((size_t)1 << 40))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_doppler: the batch is too large");
  const size_t in_bytes = pairs * sizeof(float2);
  if (int rc = check_outputs(h, "fdoct_doppler", a, "input", space == out_space ? re_im : nullptr, in_bytes, out_phase, out_corr, out_power, &floats)) return rc;
  StagePlan sp;
  sp.in(re_im, space, in_bytes);
  return run_stage(h, &sp, nullptr, a, floats, out_phase, out_corr, out_power, out_space);
} FDOCT_CATCH(h)

int fdoct_process_doppler(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                          const fdoct_doppler_params* params, float* out_phase, float* out_corr, float* out_power, fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!frames || nframes < 1 || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_process_doppler: bad arguments");
  fdoct::DopplerArgs a;
  if (int rc = plan_doppler(h, "fdoct_process_doppler", params, nframes, h->H, h->D, &a)) return rc;
  ComplexFront front;
  if (int rc = plan_complex_front(h, "fdoct_process_doppler", frames, dtype, space, nframes, pitch_bytes, &front)) return rc;
  size_t floats = 0;
  if (int rc = check_outputs(h, "fdoct_process_doppler", a, "frames", space == out_space ? frames : nullptr, front.in_span, out_phase, out_corr, out_power, &floats))
    return rc;
  return run_stage(h, &front.p.stage, &front, a, floats, out_phase, out_corr, out_power, out_space);
} FDOCT_CATCH(h)

}  // extern "C"
