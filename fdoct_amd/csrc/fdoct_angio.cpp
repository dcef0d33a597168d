// fdoct_angio.cpp -- the extern "C" entry points of include/fdoct_angio.h (libfdoct_angio.so): angiography from repeated complex
// B-scans.  The kernels are fdoct_angio.hip's; the chain in front of fdoct_process_angio is the core library's (fdoct_route.cpp:
// enqueue_complex), called in the order fdoct_capture_plan.h's ComplexFront keeps.  What is this file's own is the calls'
// arguments: the parameters' refusals and the groups (plan_angio; fdoct_angio_plan reports it), and pairs, frames and all four
// outputs in host or device memory through the staging plan.
#include "../../include/fdoct_angio.h"

#include <cmath>
#include <cstddef>

#include "fdoct_angio_kernels.h"
#include "fdoct_capture_plan.h"

using namespace fdoct_impl;

static_assert(FDOCT_ANGIO_MAX_WIN == fdoct::kAngMaxWin && FDOCT_ANGIO_MAX_REPEATS == fdoct::kAngMaxRepeats, "the kernels' registers are sized by them");

namespace {

// The buffers' sizes, in bytes.
struct AngBytes {
  size_t in = 0, floats = 0, bulk = 0;   // the pairs; one [groups][ascans][depths] float image batch; the bulk phasors
};

// What every entry point decides from the parameters and the images' shape: the refusals, then the kernels' arguments without
// their pointers, and the buffers' sizes.  h may be null (fdoct_angio_plan).
int plan_angio(fdoct_ctx* h, const char* fn, const fdoct_angio_params* p, int nframes, int ascans, int depths, fdoct::AngioArgs* a, AngBytes* b) {
  const std::string f(fn);
  if (!p) return fail(h, FDOCT_ERR_INVALID, f + ": no parameters");
  if (p->repeats < fdoct::kAngMinRepeats || p->repeats > fdoct::kAngMaxRepeats) return fail(h, FDOCT_ERR_INVALID, f + ": repeats must be 2..64");
  if (nframes < 1 || nframes > fdoct::kAngMaxFrames || nframes % p->repeats)
    return fail(h, FDOCT_ERR_INVALID, f + ": nframes must be a positive multiple of repeats, at most 65536");
  if (ascans < 1 || depths < 1 || (long long)ascans * depths > fdoct::kAngMaxPixels)
    return fail(h, FDOCT_ERR_INVALID, f + ": ascans and depths must be at least 1 and their product at most 2^24");
  if (p->win_ascans < 1 || p->win_ascans > fdoct::kAngMaxWin || p->win_depths < 1 || p->win_depths > fdoct::kAngMaxWin)
    return fail(h, FDOCT_ERR_INVALID, f + ": win_ascans and win_depths must be 1..16");
  if (p->bulk != 0 && p->bulk != 1) return fail(h, FDOCT_ERR_INVALID, f + ": bulk must be 0 or 1");
  int bulk_count = 0;
  if (p->bulk && !depth_range(p->bulk_first, p->bulk_count, depths, &bulk_count))
    return fail(h, FDOCT_ERR_INVALID, f + ": the bulk range must lie in [0, depths)");
  if (!std::isfinite(p->min_power) || p->min_power < 0.0) return fail(h, FDOCT_ERR_INVALID, f + ": min_power must be finite and not negative");
  a->groups = nframes / p->repeats, a->repeats = p->repeats, a->ascans = ascans, a->depths = depths;
  a->wa = p->win_ascans, a->wd = p->win_depths;
  a->use_bulk = p->bulk;
  a->bulk_first = p->bulk ? p->bulk_first : 0;
  a->bulk_count = bulk_count;
  a->min_power = (float)p->min_power;
  fdoct::angio_plan_launch(a, h ? h->num_cu : 0);
  const size_t pixels = (size_t)ascans * (size_t)depths;                // <= 2^24
  size_t pairs = 0;
  if (__builtin_mul_overflow((size_t)nframes, pixels, &pairs) || __builtin_mul_overflow(pairs, sizeof(float2), &b->in) ||
      __builtin_mul_overflow((size_t)a->groups * pixels, sizeof(float), &b->floats))
    return fail(h, FDOCT_ERR_INVALID, f + ": the batch's size does not fit size_t");
  b->bulk = p->bulk ? (size_t)a->groups * (size_t)(p->repeats - 1) * (size_t)ascans * sizeof(float2) : 0;   // < 2^16 2^24 8
  return FDOCT_OK;
}

// The outputs' presence, alignment and overlaps among themselves and with the input (in: its first byte and size; null where the
// memory spaces differ).
int check_outputs(fdoct_ctx* h, const char* fn, const AngBytes& b, const void* in, size_t in_bytes, const float* out_var, const float* out_decorr,
                  const float* out_cdecorr, const float* out_power) {
  const std::string f(fn);
  if (!out_var && !out_decorr && !out_cdecorr && !out_power) return fail(h, FDOCT_ERR_INVALID, f + ": no output");
  const void* const p[4] = {out_var, out_decorr, out_cdecorr, out_power};
  const size_t nb[4] = {b.floats, b.floats, b.floats, b.floats};
  for (int i = 0; i < 4; i++)
    if (reinterpret_cast<uintptr_t>(p[i]) % sizeof(float)) return fail(h, FDOCT_ERR_INVALID, f + ": every output must be aligned to 4 bytes");
  return refuse_overlaps(h, f, "input", in, in_bytes, p, nb, 4);
}

// Without out_cdecorr the bulk phasors have no reader: the bulk pass is skipped, and the other outputs' bits never depended on it.
// (What else nothing reads the kernel skips from the null pointers themselves.)
void drop_unread(fdoct::AngioArgs* a, AngBytes* b, const float* out_cdecorr) {
  if (out_cdecorr || !a->use_bulk) return;
  a->use_bulk = 0, a->bulk_first = a->bulk_count = 0, a->bulk_blocks = 0;
  b->bulk = 0;
}

// What both entry points end with.  sp's item 0 is the input (the pairs, or with `front` the frames of its chain, whose pairs are
// ws_cx's): the outputs join the plan (a null one is a null pointer the kernels skip), then every reservation, the copies up, the
// chain, the kernels, the copies down.
int run_stage(fdoct_ctx* h, StagePlan* sp, ComplexFront* front, fdoct::AngioArgs a, AngBytes b, float* out_var, float* out_decorr, float* out_cdecorr,
              float* out_power, fdoct_memspace out_space) {
  drop_unread(&a, &b, out_cdecorr);
  DEVICE_SCOPE(h);
  const int var = sp->out(out_var, out_space, b.floats), dec = sp->out(out_decorr, out_space, b.floats);
  const int cd = sp->out(out_cdecorr, out_space, b.floats), pw = sp->out(out_power, out_space, b.floats);
  if (int rc = front ? reserve_complex_front(h, front) : stage_reserve(h, sp)) return rc;
  if (a.use_bulk) {
    if (int rc = h->ws_ang_bulk.reserve(h, b.bulk)) return rc;
  }
  a.x = front ? static_cast<const float2*>(h->ws_cx) : sp->dev<const float2>(0);
  a.bulk = a.use_bulk ? static_cast<float2*>(h->ws_ang_bulk) : nullptr;
  a.out_var = sp->dev<float>(var), a.out_decorr = sp->dev<float>(dec), a.out_cdecorr = sp->dev<float>(cd), a.out_power = sp->dev<float>(pw);
  if (int rc = front ? run_complex_front(h, *front) : stage_upload(h, *sp)) return rc;
  HIP_TRY(h, fdoct::launch_angio(a, h->stream));
  return stage_finish(h, *sp);
}

}  // namespace

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_angio_plan(const fdoct_angio_params* params, int nframes, int ascans, int depths, fdoct_angio_info* info) try {
  if (!info) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_angio_plan: no output");
  fdoct::AngioArgs a;
  AngBytes b;
  if (int rc = plan_angio(nullptr, "fdoct_angio_plan", params, nframes, ascans, depths, &a, &b)) return rc;
  info->groups = a.groups, info->tiles = a.tiles, info->workgroups = a.blocks;
  info->workspace_bytes = b.bulk;
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_angio(fdoct_handle h, const float* re_im, fdoct_memspace space, int nframes, int ascans, int depths, const fdoct_angio_params* params,
                float* out_var, float* out_decorr, float* out_cdecorr, float* out_power, fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!re_im || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_angio: bad arguments");
  if (reinterpret_cast<uintptr_t>(re_im) % sizeof(float2))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_angio: re_im must be aligned to one (re, im) pair (8 bytes)");
  fdoct::AngioArgs a;
  AngBytes b;
  if (int rc = plan_angio(h, "fdoct_angio", params, nframes, ascans, depths, &a, &b)) return rc;
  if (int rc = check_outputs(h, "fdoct_angio", b, space == out_space ? re_im : nullptr, b.in, out_var, out_decorr, out_cdecorr, out_power)) return rc;
  StagePlan sp;
  sp.in(re_im, space, b.in);
  return run_stage(h, &sp, nullptr, a, b, out_var, out_decorr, out_cdecorr, out_power, out_space);
} FDOCT_CATCH(h)

int fdoct_process_angio(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                        const fdoct_angio_params* params, float* out_var, float* out_decorr, float* out_cdecorr, float* out_power,
                        fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!frames || nframes < 1 || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_process_angio: bad arguments");
  fdoct::AngioArgs a;
  AngBytes b;
  if (int rc = plan_angio(h, "fdoct_process_angio", params, nframes, h->H, h->D, &a, &b)) return rc;
  ComplexFront front;
  if (int rc = plan_complex_front(h, "fdoct_process_angio", frames, dtype, space, nframes, pitch_bytes, &front)) return rc;
  if (int rc = check_outputs(h, "fdoct_process_angio", b, space == out_space ? frames : nullptr, front.in_span, out_var, out_decorr, out_cdecorr, out_power))
    return rc;
  return run_stage(h, &front.p.stage, &front, a, b, out_var, out_decorr, out_cdecorr, out_power, out_space);
} FDOCT_CATCH(h)

}  // extern "C"
