// fdoct_cxavg.cpp -- the extern "C" entry points of include/fdoct_cxavg.h (libfdoct_cxavg.so): the coherent average of repeated
// complex B-scans.  The kernels are fdoct_cxavg.hip's; the chain in front of fdoct_process_cxavg is the core library's
// (fdoct_route.cpp: enqueue_complex), called in the order fdoct_capture_plan.h's ComplexFront keeps.  What is this file's own is
// the calls' arguments: the parameters' refusals and the groups (plan_cxavg; fdoct_cxavg_plan reports it), and pairs, frames and
// all four outputs in host or device memory through the staging plan.
#include "../../include/fdoct_cxavg.h"

#include <cstddef>

#include "fdoct_capture_plan.h"
#include "fdoct_cxavg_kernels.h"

using namespace fdoct_impl;

static_assert(FDOCT_CXAVG_MAX_REPEATS == fdoct::kCxaMaxRepeats && FDOCT_CXAVG_REG_PAIRS == fdoct::kCxaRegPairs, "the kernel's registers and LDS are sized by them");
static_assert(FDOCT_CXAVG_FORM_REGISTER == fdoct::kCxaFormRegister && FDOCT_CXAVG_FORM_STREAMING == fdoct::kCxaFormStreaming, "fdoct_cxavg_info.form");

namespace {

// The buffers' sizes, in bytes.
struct CxaBytes {
  size_t in = 0, floats = 0, pairs = 0, ws = 0;   // the input; one [groups][ascans][depths] float image batch; one of pairs; the workspace
  size_t phasors = 0;                             // pairs at the workspace's front that are the phasors; the per-row sums lie behind them
};

// What every entry point decides from the parameters and the images' shape: the refusals, then the kernels' arguments without
// their pointers, and the buffers' sizes.  h may be null (fdoct_cxavg_plan).
int plan_cxavg(fdoct_ctx* h, const char* fn, const fdoct_cxavg_params* p, int nframes, int ascans, int depths, fdoct::CxavgArgs* a, CxaBytes* b) {
  const std::string f(fn);
  if (!p) return fail(h, FDOCT_ERR_INVALID, f + ": no parameters");
  if (p->repeats < fdoct::kCxaMinRepeats || p->repeats > fdoct::kCxaMaxRepeats) return fail(h, FDOCT_ERR_INVALID, f + ": repeats must be 2..64");
  if (p->stride < 1 || p->stride > p->repeats) return fail(h, FDOCT_ERR_INVALID, f + ": stride must be 1..repeats");
  if (nframes < p->repeats || nframes > fdoct::kCxaMaxFrames || (nframes - p->repeats) % p->stride)
    return fail(h, FDOCT_ERR_INVALID, f + ": nframes must be repeats plus a multiple of stride, at most 65536");
  if (p->ref < 0 || p->ref >= p->repeats) return fail(h, FDOCT_ERR_INVALID, f + ": ref must be 0..repeats-1");
  if (ascans < 1 || depths < 1 || (long long)ascans * depths > fdoct::kCxaMaxPixels)
    return fail(h, FDOCT_ERR_INVALID, f + ": ascans and depths must be at least 1 and their product at most 2^24");
  if (p->align < fdoct::kCxaAlignNone || p->align > fdoct::kCxaAlignFrame) return fail(h, FDOCT_ERR_INVALID, f + ": align must be 0, 1 or 2");
  int count = 0;
  if (p->align && !depth_range(p->align_first, p->align_count, depths, &count))
    return fail(h, FDOCT_ERR_INVALID, f + ": the alignment range must lie in [0, depths)");
  a->groups = (nframes - p->repeats) / p->stride + 1, a->repeats = p->repeats, a->stride = p->stride, a->ref = p->ref;
  a->ascans = ascans, a->depths = depths;
  a->align = p->align, a->first = p->align ? p->align_first : 0, a->count = count;
  fdoct::cxavg_plan_launch(a, h ? h->num_cu : 0);
  const size_t pixels = (size_t)ascans * (size_t)depths;                // <= 2^24
  size_t in_pairs = 0;
  if (__builtin_mul_overflow((size_t)nframes, pixels, &in_pairs) || __builtin_mul_overflow(in_pairs, sizeof(float2), &b->in) ||
      __builtin_mul_overflow((size_t)a->groups * pixels, sizeof(float2), &b->pairs))
    return fail(h, FDOCT_ERR_INVALID, f + ": the batch's size does not fit size_t");
  b->floats = b->pairs / 2;
  b->phasors = (size_t)a->groups * (size_t)p->repeats;                  // < 2^16 2^6
  b->ws = p->align == fdoct::kCxaAlignFrame ? (b->phasors + b->phasors * (size_t)ascans) * sizeof(float2) : 0;   // < 2^22 2^25 8
  return FDOCT_OK;
}

// The outputs' presence, alignment and overlaps among themselves and with the input (in: its first byte and size; null where the
// memory spaces differ).
int check_outputs(fdoct_ctx* h, const char* fn, const CxaBytes& b, const void* in, size_t in_bytes, const float* out_mean, const float* out_mag,
                  const float* out_incoh, const float* out_coh) {
  const std::string f(fn);
  if (!out_mean && !out_mag && !out_incoh && !out_coh) return fail(h, FDOCT_ERR_INVALID, f + ": no output");
  const void* const p[4] = {out_mean, out_mag, out_incoh, out_coh};
  const size_t nb[4] = {b.pairs, b.floats, b.floats, b.floats};
  if (reinterpret_cast<uintptr_t>(out_mean) % sizeof(float2)) return fail(h, FDOCT_ERR_INVALID, f + ": out_mean must be aligned to one (re, im) pair (8 bytes)");
  for (int i = 1; i < 4; i++)
    if (reinterpret_cast<uintptr_t>(p[i]) % sizeof(float)) return fail(h, FDOCT_ERR_INVALID, f + ": every float output must be aligned to 4 bytes");
  return refuse_overlaps(h, f, "input", in, in_bytes, p, nb, 4);
}

// With out_incoh alone the phasors have no reader: the alignment is skipped, and out_incoh's bits never depended on it.
// (What else nothing reads the kernel skips from the null pointers themselves.)
void drop_unread(fdoct::CxavgArgs* a, CxaBytes* b, const float* out_mean, const float* out_mag, const float* out_coh) {
  if (out_mean || out_mag || out_coh || !a->align) return;
  a->align = fdoct::kCxaAlignNone, a->first = a->count = 0, a->row_blocks = a->phasor_blocks = 0;
  b->ws = 0;
}

// What both entry points end with.  sp's item 0 is the input (the pairs, or with `front` the frames of its chain, whose pairs are
// ws_cx's): the outputs join the plan (a null one is a null pointer the kernels skip), then every reservation, the copies up, the
// chain, the kernels, the copies down.
int run_stage(fdoct_ctx* h, StagePlan* sp, ComplexFront* front, fdoct::CxavgArgs a, CxaBytes b, float* out_mean, float* out_mag, float* out_incoh,
              float* out_coh, fdoct_memspace out_space) {
  drop_unread(&a, &b, out_mean, out_mag, out_coh);
  DEVICE_SCOPE(h);
  const int mean = sp->out(out_mean, out_space, b.pairs), mag = sp->out(out_mag, out_space, b.floats);
  const int inc = sp->out(out_incoh, out_space, b.floats), coh = sp->out(out_coh, out_space, b.floats);
  if (int rc = front ? reserve_complex_front(h, front) : stage_reserve(h, sp)) return rc;
  if (b.ws) {
    if (int rc = h->ws_cxa.reserve(h, b.ws)) return rc;
  }
  a.x = front ? static_cast<const float2*>(h->ws_cx) : sp->dev<const float2>(0);
  a.phasors = b.ws ? static_cast<float2*>(h->ws_cxa) : nullptr;
  a.rows = b.ws ? a.phasors + b.phasors : nullptr;
  a.out_mean = sp->dev<float2>(mean), a.out_mag = sp->dev<float>(mag), a.out_incoh = sp->dev<float>(inc), a.out_coh = sp->dev<float>(coh);
  if (int rc = front ? run_complex_front(h, *front) : stage_upload(h, *sp)) return rc;
  HIP_TRY(h, fdoct::launch_cxavg(a, h->stream));
  return stage_finish(h, *sp);
}

}  // namespace

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_cxavg_plan(const fdoct_cxavg_params* params, int nframes, int ascans, int depths, fdoct_cxavg_info* info) try {
  if (!info) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_cxavg_plan: no output");
  fdoct::CxavgArgs a;
  CxaBytes b;
  if (int rc = plan_cxavg(nullptr, "fdoct_cxavg_plan", params, nframes, ascans, depths, &a, &b)) return rc;
  info->groups = a.groups, info->form = a.form, info->workgroups = a.blocks;
  info->workspace_bytes = b.ws;
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_cxavg(fdoct_handle h, const float* re_im, fdoct_memspace space, int nframes, int ascans, int depths, const fdoct_cxavg_params* params,
                float* out_mean, float* out_mag, float* out_incoh, float* out_coh, fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!re_im || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_cxavg: bad arguments");
  if (reinterpret_cast<uintptr_t>(re_im) % sizeof(float2))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_cxavg: re_im must be aligned to one (re, im) pair (8 bytes)");
  fdoct::CxavgArgs a;
  CxaBytes b;
  if (int rc = plan_cxavg(h, "fdoct_cxavg", params, nframes, ascans, depths, &a, &b)) return rc;
  if (int rc = check_outputs(h, "fdoct_cxavg", b, space == out_space ? re_im : nullptr, b.in, out_mean, out_mag, out_incoh, out_coh)) return rc;
  StagePlan sp;
  sp.in(re_im, space, b.in);
  return run_stage(h, &sp, nullptr, a, b, out_mean, out_mag, out_incoh, out_coh, out_space);
} FDOCT_CATCH(h)

int fdoct_process_cxavg(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                        const fdoct_cxavg_params* params, float* out_mean, float* out_mag, float* out_incoh, float* out_coh,
                        fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!frames || nframes < 1 || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_process_cxavg: bad arguments");
  fdoct::CxavgArgs a;
  CxaBytes b;
  if (int rc = plan_cxavg(h, "fdoct_process_cxavg", params, nframes, h->H, h->D, &a, &b)) return rc;
  ComplexFront front;
  if (int rc = plan_complex_front(h, "fdoct_process_cxavg", frames, dtype, space, nframes, pitch_bytes, &front)) return rc;
  if (int rc = check_outputs(h, "fdoct_process_cxavg", b, space == out_space ? frames : nullptr, front.in_span, out_mean, out_mag, out_incoh, out_coh))
    return rc;
  return run_stage(h, &front.p.stage, &front, a, b, out_mean, out_mag, out_incoh, out_coh, out_space);
} FDOCT_CATCH(h)

}  // extern "C"
