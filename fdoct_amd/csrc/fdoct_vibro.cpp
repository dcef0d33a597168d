// fdoct_vibro.cpp -- the extern "C" entry points of include/fdoct_vibro.h (libfdoct_vibro.so): phase-sensitive vibrometry from
// complex A-scans over time.  The kernels are fdoct_vibro.hip's; the chain in front of fdoct_process_vibro is the core library's
// (fdoct_route.cpp: enqueue_complex), called as fdoct_dispersion.cpp calls it.  What is this file's own is the calls' arguments:
// the parameters' refusals and the chunk rule (plan_vibro; fdoct_vibro_plan reports it), and pairs, frames and outputs in host or
// device memory.  The pairs or frames go through the staging plan as fdoct_doppler.cpp's do.  A staging plan holds four items and
// this stage has four outputs beside its input, so outputs in host memory go through one workspace of the stage's own (ws_vib_out)
// and are copied down behind the kernels, as fdoct_dispersion.cpp copies its winner.
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
  if (p->ref) {
    if (p->ref_first < 0 || p->ref_first >= depths || p->ref_count < 0 || p->ref_count > depths - p->ref_first)
      return fail(h, FDOCT_ERR_INVALID, f + ": the reference range must lie in [0, depths)");
  }
  if (p->detrend != 0 && p->detrend != 1) return fail(h, FDOCT_ERR_INVALID, f + ": detrend must be 0 or 1");
  if (p->window != FDOCT_VIBRO_RECT && p->window != FDOCT_VIBRO_HANN) return fail(h, FDOCT_ERR_INVALID, f + ": bad window");
  if (!std::isfinite(p->scale) || !std::isfinite(p->min_power) || p->min_power < 0.0)
    return fail(h, FDOCT_ERR_INVALID, f + ": scale and min_power must be finite, min_power not negative");
  if (p->chunk_steps < 0) return fail(h, FDOCT_ERR_INVALID, f + ": chunk_steps must not be negative");
  a->T = nframes, a->ascans = ascans, a->depths = depths;
  a->use_ref = p->ref;
  a->ref_first = p->ref ? p->ref_first : 0;
  a->ref_count = !p->ref ? 0 : p->ref_count ? p->ref_count : depths - p->ref_first;
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
  const void* p[4] = {out_amp, out_rms, out_drift, out_power};
  const size_t nb[4] = {b.amp, b.floats, b.floats, b.floats};
  for (int i = 0; i < 4; i++) {
    if (reinterpret_cast<uintptr_t>(p[i]) % sizeof(float)) return fail(h, FDOCT_ERR_INVALID, f + ": out_rms, out_drift and out_power must be aligned to 4 bytes");
    if (overlap(in, in_bytes, p[i], nb[i])) return fail(h, FDOCT_ERR_INVALID, f + ": input and output buffers overlap");
    for (int j = 0; j < i; j++)
      if (overlap(p[i], nb[i], p[j], nb[j])) return fail(h, FDOCT_ERR_INVALID, f + ": the outputs overlap");
  }
  return FDOCT_OK;
}

// Where the kernels write: the caller's device memory, or a section of ws_vib_out on its way to the caller's host memory.
struct OutPlan {
  void* host[4] = {nullptr, nullptr, nullptr, nullptr};   // the caller's host pointers, or null
  size_t offset[4] = {0, 0, 0, 0}, bytes[4] = {0, 0, 0, 0};
  size_t total = 0;
};

// Every reservation of the stage: the outputs' workspace, the reference phasors, the tables, the chunk partials.
int reserve_stage(fdoct_ctx* h, StagePlan* sp, const fdoct::VibroArgs& a, const VibBytes& b, float* out_amp, float* out_rms, float* out_drift, float* out_power,
                  fdoct_memspace out_space, OutPlan* o) {
  if (out_space == FDOCT_MEM_HOST) {
    void* p[4] = {out_amp, out_rms, out_drift, out_power};
    const size_t nb[4] = {b.amp, b.floats, b.floats, b.floats};
    for (int i = 0; i < 4; i++) {
      if (!p[i]) continue;
      o->host[i] = p[i], o->offset[i] = o->total, o->bytes[i] = nb[i];
      o->total += (nb[i] + StagePlan::kAlign - 1) & ~(StagePlan::kAlign - 1);   // <= 2^30 + 3 2^26 + 4 kAlign
    }
    sp->sync = true;
    if (int rc = h->ws_vib_out.reserve(h, o->total)) return rc;
  }
  if (a.use_ref) {
    if (int rc = h->ws_vib_ref.reserve(h, b.ref)) return rc;
  }
  if (a.nfreq) {
    if (int rc = h->ws_vib_tab.reserve(h, b.tab)) return rc;
  }
  if (a.chunks > 1) {
    if (int rc = h->ws_vib_part.reserve(h, b.part)) return rc;
  }
  return FDOCT_OK;
}

void set_pointers(fdoct_ctx* h, const VibBytes& b, const OutPlan& o, float* out_amp, float* out_rms, float* out_drift, float* out_power, fdoct::VibroArgs* a) {
  unsigned char* const w = h->ws_vib_out;
  a->out_amp = reinterpret_cast<float2*>(o.host[0] ? w + o.offset[0] : reinterpret_cast<unsigned char*>(out_amp));
  a->out_rms = reinterpret_cast<float*>(o.host[1] ? w + o.offset[1] : reinterpret_cast<unsigned char*>(out_rms));
  a->out_drift = reinterpret_cast<float*>(o.host[2] ? w + o.offset[2] : reinterpret_cast<unsigned char*>(out_drift));
  a->out_power = reinterpret_cast<float*>(o.host[3] ? w + o.offset[3] : reinterpret_cast<unsigned char*>(out_power));
  a->refph = h->ws_vib_ref, a->part = h->ws_vib_part;
  if (a->nfreq) {
    const size_t slots = (size_t)a->nfreq + 1;
    a->tab = h->ws_vib_tab;
    a->cst = a->tab + b.tab_entries;
    a->head = a->cst + b.cst_entries;
    a->glob = a->head + slots;
  }
}

// The kernels, the outputs' copies to host memory, the staged copies and the synchronise host memory asks for.
int run_stage(fdoct_ctx* h, const StagePlan& sp, const OutPlan& o, const fdoct::VibroArgs& a) {
  HIP_TRY(h, fdoct::launch_vibro(a, h->stream));
  for (int i = 0; i < 4; i++)
    if (o.host[i]) HIP_TRY(h, hipMemcpyAsync(o.host[i], (unsigned char*)h->ws_vib_out + o.offset[i], o.bytes[i], hipMemcpyDeviceToHost, h->stream));
  return stage_finish(h, sp);
}

// Without out_amp the lock-in's sums have no reader: the kernels skip them, and the other outputs' bits do not depend on them.
void drop_unread(fdoct::VibroArgs* a, VibBytes* b, const float* out_amp) {
  if (out_amp || !a->nfreq) return;
  a->nfreq = 0;
  b->tab = b->tab_entries = b->cst_entries = 0;
  b->part = a->chunks > 1 ? (size_t)a->chunks * (size_t)fdoct::vibro_sums(0) * (size_t)a->pixels * sizeof(double) : 0;
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
  drop_unread(&a, &b, out_amp);
  DEVICE_SCOPE(h);
  // every reservation before anything is enqueued: the staged pairs, the outputs' workspace, the stage's own
  StagePlan sp;
  OutPlan o;
  const int in = sp.in(re_im, space, in_bytes);
  if (int rc = stage_reserve(h, &sp)) return rc;
  if (int rc = reserve_stage(h, &sp, a, b, out_amp, out_rms, out_drift, out_power, out_space, &o)) return rc;
  a.x = sp.dev<const float2>(in);
  set_pointers(h, b, o, out_amp, out_rms, out_drift, out_power, &a);
  if (int rc = stage_upload(h, sp)) return rc;
  return run_stage(h, sp, o, a);
} FDOCT_CATCH(h)

int fdoct_process_vibro(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                        const fdoct_vibro_params* params, float* out_amp, float* out_rms, float* out_drift, float* out_power,
                        fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!frames || nframes < 1 || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_process_vibro: bad arguments");
  fdoct::VibroArgs a;
  VibBytes b;
  if (int rc = plan_vibro(h, "fdoct_process_vibro", params, nframes, h->H, h->D, &a, &b)) return rc;
  FramePlan p;
  if (int rc = plan_frames(h, "fdoct_process_vibro", frames, dtype, space, nframes, pitch_bytes, &p)) return rc;
  size_t in_span = 0;
  if (__builtin_mul_overflow(p.pitch, (size_t)p.raw_h * (size_t)nframes, &in_span))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_process_vibro: the batch is too large");
  if (int rc = check_outputs(h, "fdoct_process_vibro", a, b, space == out_space ? frames : nullptr, in_span, out_amp, out_rms, out_drift, out_power))
    return rc;
  drop_unread(&a, &b, out_amp);
  DEVICE_SCOPE(h);
  // every refusal and reservation before anything is enqueued: the staged frames, the outputs' workspace, the stage's own, the
  // chain's pairs, then the chain's own checks and its route on the frames where the kernels will read them (a run-time compile
  // happens here)
  OutPlan o;
  if (int rc = stage_reserve(h, &p.stage)) return rc;
  if (int rc = reserve_stage(h, &p.stage, a, b, out_amp, out_rms, out_drift, out_power, out_space, &o)) return rc;
  if (int rc = h->ws_cx.reserve(h, (size_t)nframes * (size_t)a.pixels * sizeof(float2))) return rc;
  if (int rc = enqueue_complex(h, p.stage.dev<const void>(0), dtype, nframes, p.stage.pitch(0), nullptr)) return rc;
  a.x = h->ws_cx;
  set_pointers(h, b, o, out_amp, out_rms, out_drift, out_power, &a);
  if (int rc = stage_upload(h, p.stage)) return rc;
  if (int rc = enqueue_complex(h, p.stage.dev<const void>(0), dtype, nframes, p.stage.pitch(0), h->ws_cx)) return rc;
  return run_stage(h, p.stage, o, a);
} FDOCT_CATCH(h)

}  // extern "C"
