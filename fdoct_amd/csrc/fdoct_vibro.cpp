// fdoct_vibro.cpp -- the extern "C" entry points of include/fdoct_vibro.h (libfdoct_vibro.so): phase-sensitive vibrometry from
// complex A-scans over time.  The kernels are fdoct_vibro.hip's; the chain in front of fdoct_process_vibro is the core library's
// (fdoct_route.cpp: enqueue_complex), called in the order fdoct_capture_plan.h's ComplexFront keeps.  What is this file's own is the
// calls' arguments: the parameters' refusals and the chunk rule (plan_vibro; fdoct_vibro_plan reports it), and pairs, frames and
// all four outputs in host or device memory through the staging plan.
#include "../../include/fdoct_vibro.h"

#include <cmath>
#include <cstddef>

#include "fdoct_capture_plan.h"
#include "fdoct_vibro_kernels.h"

using namespace fdoct_impl;

static_assert(FDOCT_VIBRO_MAX_FREQ == fdoct::kVibMaxFreq, "the kernels' accumulators are sized by it");

namespace {

// The workspaces' sizes, in bytes.
struct VibBytes {
  size_t ref = 0, part = 0, tab = 0, floats = 0, amp = 0;   // floats: one [ascans][depths] float image; amp: out_amp
  size_t tab_entries = 0, cst_entries = 0;                  // double2s of VibroArgs::tab and ::cst
};

// What every entry point decides from the parameters and the images' shape: the refusals, then the kernels' arguments without
// their pointers, and the workspaces' sizes.  h may be null (fdoct_vibro_plan).
int plan_vibro(fdoct_ctx* h, const char* fn, const fdoct_vibro_params* p, int nframes, int ascans, int depths, fdoct::VibroArgs* a, VibBytes* b) {
  const std::string f(fn);
  if (!p) return fail(h, FDOCT_ERR_INVALID, f + ": no parameters");
  if (nframes < 2 || nframes > fdoct::kVibMaxFrames) return fail(h, FDOCT_ERR_INVALID, f + ": nframes must be 2..65536");
  if (ascans < 1 || depths < 1 || (long long)ascans * depths > fdoct::kVibMaxPixels)
    return fail(h, FDOCT_ERR_INVALID, f + ": ascans and depths must be at least 1 and their product at most 2^24");
  if (p->nfreq < 0 || p->nfreq > fdoct::kVibMaxFreq) return fail(h, FDOCT_ERR_INVALID, f + ": nfreq must be 0..8");
  for (int j = 0; j < p->nfreq; j++)
    if (!std::isfinite(p->freq[j]) || !(p->freq[j] > 0.0) || p->freq[j] > 0.5)
      return fail(h, FDOCT_ERR_INVALID, f + ": every frequency must lie in (0, 0.5] cycles per frame");
  if (p->ref != 0 && p->ref != 1) return fail(h, FDOCT_ERR_INVALID, f + ": ref must be 0 or 1");
  int ref_count = 0;
  if (p->ref && !depth_range(p->ref_first, p->ref_count, depths, &ref_count))
    return fail(h, FDOCT_ERR_INVALID, f + ": the reference range must lie in [0, depths)");
  if (p->detrend != 0 && p->detrend != 1) return fail(h, FDOCT_ERR_INVALID, f + ": detrend must be 0 or 1");
  if (p->window != FDOCT_VIBRO_RECT && p->window != FDOCT_VIBRO_HANN) return fail(h, FDOCT_ERR_INVALID, f + ": bad window");
  if (!std::isfinite(p->scale) || !std::isfinite(p->min_power) || p->min_power < 0.0)
    return fail(h, FDOCT_ERR_INVALID, f + ": scale and min_power must be finite, min_power not negative");
  if (p->chunk_steps < 0) return fail(h, FDOCT_ERR_INVALID, f + ": chunk_steps must not be negative");
  a->T = nframes, a->ascans = ascans, a->depths = depths;
  a->use_ref = p->ref;
  a->ref_first = p->ref ? p->ref_first : 0;
  a->ref_count = ref_count;
  a->detrend = p->detrend, a->window = p->window, a->nfreq = p->nfreq;
  for (int j = 0; j < fdoct::kVibMaxFreq; j++) a->freq[j] = j < p->nfreq ? p->freq[j] : 0.0;
  a->scale = p->scale, a->min_power = p->min_power;
  a->chunk_steps = p->chunk_steps ? p->chunk_steps : fdoct::vibro_chunk_rule(nframes, (long long)ascans * depths);
  fdoct::vibro_plan_launch(a);
  const size_t pixels = (size_t)a->pixels, slots = (size_t)a->nfreq + 1;
  bool wraps = false;
  b->floats = pixels * sizeof(float);                                    // <= 2^26
  b->amp = (size_t)a->nfreq * pixels * sizeof(float2);                   // <= 2^30
  b->ref = a->use_ref ? (size_t)nframes * (size_t)ascans * sizeof(float2) : 0;   // <= 2^43
  b->tab_entries = a->nfreq ? (size_t)a->nfreq * (size_t)nframes : 0;
  b->cst_entries = a->nfreq ? (size_t)a->chunks * slots * 2 : 0;
  b->tab = a->nfreq ? (b->tab_entries + b->cst_entries + slots + 2 * slots) * sizeof(double2) : 0;
  if (a->chunks > 1) {
    size_t sums = 0;
    wraps = __builtin_mul_overflow((size_t)a->chunks * (size_t)fdoct::vibro_sums(a->nfreq), pixels, &sums) ||
            __builtin_mul_overflow(sums, sizeof(double), &b->part);
  }
  if (wraps) return fail(h, FDOCT_ERR_INVALID, f + ": the chunk partials' size does not fit size_t");
  return FDOCT_OK;
}

// The outputs' presence, alignment and overlaps among themselves and with the input (in: its first byte and size; null where the
// memory spaces differ).
int check_outputs(fdoct_ctx* h, const char* fn, const fdoct::VibroArgs& a, const VibBytes& b, const void* in, size_t in_bytes, const float* out_amp,
                  const float* out_rms, const float* out_drift, const float* out_power) {
  const std::string f(fn);
  if (!out_amp && !out_rms && !out_drift && !out_power) return fail(h, FDOCT_ERR_INVALID, f + ": no output");
  if (out_amp && a.nfreq == 0) return fail(h, FDOCT_ERR_INVALID, f + ": out_amp must be NULL with nfreq 0");
  if (reinterpret_cast<uintptr_t>(out_amp) % sizeof(float2)) return fail(h, FDOCT_ERR_INVALID, f + ": out_amp must be aligned to one (re, im) pair (8 bytes)");
  const void* const p[4] = {out_amp, out_rms, out_drift, out_power};
  const size_t nb[4] = {b.amp, b.floats, b.floats, b.floats};
  for (int i = 0; i < 4; i++)
    if (reinterpret_cast<uintptr_t>(p[i]) % sizeof(float)) return fail(h, FDOCT_ERR_INVALID, f + ": out_rms, out_drift and out_power must be aligned to 4 bytes");
  return refuse_overlaps(h, f, "input", in, in_bytes, p, nb, 4);
}

// Without out_amp the lock-in's sums have no reader: the kernels skip them, and the other outputs' bits do not depend on them.
void drop_unread(fdoct::VibroArgs* a, VibBytes* b, const float* out_amp) {
  if (out_amp || !a->nfreq) return;
  a->nfreq = 0;
  b->tab = b->tab_entries = b->cst_entries = 0;
  b->part = a->chunks > 1 ? (size_t)a->chunks * (size_t)fdoct::vibro_sums(0) * (size_t)a->pixels * sizeof(double) : 0;
}

// What both entry points end with.  sp's item 0 is the input (the pairs, or with `front` the frames of its chain, whose pairs are
// ws_cx's): the outputs join the plan (a null one is a null pointer the kernels skip), then every reservation -- the reference
// phasors, the tables, the chunk partials -- the copies up, the chain, the kernels, the copies down.
int run_stage(fdoct_ctx* h, StagePlan* sp, ComplexFront* front, fdoct::VibroArgs a, VibBytes b, float* out_amp, float* out_rms, float* out_drift,
              float* out_power, fdoct_memspace out_space) {
  drop_unread(&a, &b, out_amp);
  DEVICE_SCOPE(h);
  const int amp = sp->out(out_amp, out_space, b.amp), rms = sp->out(out_rms, out_space, b.floats);
  const int drift = sp->out(out_drift, out_space, b.floats), power = sp->out(out_power, out_space, b.floats);
  if (int rc = front ? reserve_complex_front(h, front) : stage_reserve(h, sp)) return rc;
  if (a.use_ref) {
    if (int rc = h->ws_vib_ref.reserve(h, b.ref)) return rc;
  }
  if (a.nfreq) {
    if (int rc = h->ws_vib_tab.reserve(h, b.tab)) return rc;
  }
  if (a.chunks > 1) {
    if (int rc = h->ws_vib_part.reserve(h, b.part)) return rc;
  }
  a.x = front ? static_cast<const float2*>(h->ws_cx) : sp->dev<const float2>(0);
  a.out_amp = sp->dev<float2>(amp), a.out_rms = sp->dev<float>(rms), a.out_drift = sp->dev<float>(drift), a.out_power = sp->dev<float>(power);
  a.refph = h->ws_vib_ref, a.part = h->ws_vib_part;
  if (a.nfreq) {
    const size_t slots = (size_t)a.nfreq + 1;
    a.tab = h->ws_vib_tab;
    a.cst = a.tab + b.tab_entries;
    a.head = a.cst + b.cst_entries;
    a.glob = a.head + slots;
  }
  if (int rc = front ? run_complex_front(h, *front) : stage_upload(h, *sp)) return rc;
  HIP_TRY(h, fdoct::launch_vibro(a, h->stream));
  return stage_finish(h, *sp);
}

}  // namespace

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_vibro_plan(const fdoct_vibro_params* params, int nframes, int ascans, int depths, fdoct_vibro_info* info) try {
  if (!info) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_vibro_plan: no output");
  fdoct::VibroArgs a;
  VibBytes b;
  if (int rc = plan_vibro(nullptr, "fdoct_vibro_plan", params, nframes, ascans, depths, &a, &b)) return rc;
  info->chunk_steps = a.chunk_steps, info->chunks = a.chunks, info->workgroups = a.items;
  info->workspace_bytes = b.ref + b.part + b.tab;
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_vibro(fdoct_handle h, const float* re_im, fdoct_memspace space, int nframes, int ascans, int depths, const fdoct_vibro_params* params,
                float* out_amp, float* out_rms, float* out_drift, float* out_power, fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!re_im || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_vibro: bad arguments");
  if (reinterpret_cast<uintptr_t>(re_im) % sizeof(float2))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_vibro: re_im must be aligned to one (re, im) pair (8 bytes)");
  fdoct::VibroArgs a;
  VibBytes b;
  if (int rc = plan_vibro(h, "fdoct_vibro", params, nframes, ascans, depths, &a, &b)) return rc;
  const size_t in_bytes = (size_t)nframes * (size_t)a.pixels * sizeof(float2);   // <= 2^16 2^24 8
  if (int rc = check_outputs(h, "fdoct_vibro", a, b, space == out_space ? re_im : nullptr, in_bytes, out_amp, out_rms, out_drift, out_power)) return rc;
  StagePlan sp;
  sp.in(re_im, space, in_bytes);
  return run_stage(h, &sp, nullptr, a, b, out_amp, out_rms, out_drift, out_power, out_space);
} FDOCT_CATCH(h)

int fdoct_process_vibro(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                        const fdoct_vibro_params* params, float* out_amp, float* out_rms, float* out_drift, float* out_power,
                        fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!frames || nframes < 1 || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_process_vibro: bad arguments");
  fdoct::VibroArgs a;
  VibBytes b;
  if (int rc = plan_vibro(h, "fdoct_process_vibro", params, nframes, h->H, h->D, &a, &b)) return rc;
  ComplexFront front;
  if (int rc = plan_complex_front(h, "fdoct_process_vibro", frames, dtype, space, nframes, pitch_bytes, &front)) return rc;
  if (int rc = check_outputs(h, "fdoct_process_vibro", a, b, space == out_space ? frames : nullptr, front.in_span, out_amp, out_rms, out_drift, out_power))
    return rc;
  return run_stage(h, &front.p.stage, &front, a, b, out_amp, out_rms, out_drift, out_power, out_space);
} FDOCT_CATCH(h)

}  // extern "C"
