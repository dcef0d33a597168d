// fdoct_capture_plan.h -- how an entry point that takes camera frames plans them: what fdoct_capture.cpp (where the two functions
// are defined) and fdoct_calibrate.cpp share, so that both read frames, front end and colour input by one set of rules and refuse
// the same arguments.  Internal.
#pragma once
#include "fdoct_capture_kernels.h"
#include "fdoct_ctx.h"

namespace fdoct_impl {

// What a call does with its frames, decided (and refused) before anything is enqueued.
struct FramePlan {
  StagePlan stage;  // the frames are its item 0; a call adds its outputs
  fdoct::CaptureFrames cf;  // what the kernels read: front_passes fills it
  fdoct_dtype dtype = FDOCT_U16;
  bool frontend = false;
  bool colour = false;  // interleaved B,G,R frames (fdoct_set_colour_input): es is 3, the colour stage runs in the front end's place
  int nframes = 0, raw_w = 0, raw_h = 0;
  size_t es = 0, pitch = 0;
};

// Checks the frames' arguments against the handle (`fn` prefixes the message) and fills *p; enqueues nothing.
int plan_frames(fdoct_ctx* h, const char* fn, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes,
                size_t pitch_bytes, FramePlan* p);
// What stands between the frames on the device (the caller's, or the plan's item 0 after its upload) and the kernels: the colour
// stage or the front end.  src null: their checks and workspaces only, and p.cf gets its shape -- nothing is enqueued.
int front_passes(fdoct_ctx* h, FramePlan& p, const void* src);

// The complex chain in front of a stage (fdoct_route.cpp: enqueue_complex): camera frames in, the (re, im) pairs [nframes H D] in
// h->ws_cx out.  The three functions are the call's order, and its one rule is stated here: every refusal and reservation -- the
// staged arguments, the pairs, the chain's own checks and its route, which may compile at run time -- comes before the first
// enqueue.
//   plan_complex_front     the frames' refusals and sizes.  The caller then checks its outputs against [frames, in_span) and adds
//                          them to front.p.stage.
//   reserve_complex_front  the staging buffers, ws_cx, and the chain's dry run on the frames where the kernels will read them.  The
//                          caller then makes the stage's own reservations and fills its kernels' pointers (the pairs: h->ws_cx).
//   run_complex_front      the staged copies up and the chain.  The caller launches behind it and ends with
//                          stage_finish(h, front.p.stage).
struct ComplexFront {
  FramePlan p;
  size_t in_span = 0;   // bytes from the first frame's first to the last frame's last: what no output may lie on
  size_t cx_bytes = 0;  // the pairs in ws_cx
  bool reserved = false;
};

inline int plan_complex_front(fdoct_ctx* h, const char* fn, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes,
                              size_t pitch_bytes, ComplexFront* f) {
  if (int rc = plan_frames(h, fn, frames, dtype, space, nframes, pitch_bytes, &f->p)) return rc;
  size_t pairs = 0;
  if (__builtin_mul_overflow((size_t)nframes * (size_t)h->H, (size_t)h->D, &pairs) || __builtin_mul_overflow(pairs, sizeof(float2), &f->cx_bytes) ||
      __builtin_mul_overflow(f->p.pitch, (size_t)f->p.raw_h * (size_t)nframes, &f->in_span))
    return fail(h, FDOCT_ERR_INVALID, std::string(fn) + ": the batch is too large");
  return FDOCT_OK;
}
inline int reserve_complex_front(fdoct_ctx* h, ComplexFront* f) {
  StagePlan& s = f->p.stage;
  if (int rc = stage_reserve(h, &s)) return rc;
  if (int rc = h->ws_cx.reserve(h, f->cx_bytes)) return rc;
  if (int rc = enqueue_complex(h, s.dev<const void>(0), f->p.dtype, f->p.nframes, s.pitch(0), nullptr)) return rc;
  f->reserved = true;
  return FDOCT_OK;
}
inline int run_complex_front(fdoct_ctx* h, const ComplexFront& f) {
  const StagePlan& s = f.p.stage;
  if (!f.reserved) return fail(h, FDOCT_ERR_STATE, "the complex chain: a run before reserve");
  if (int rc = stage_upload(h, s)) return rc;
  return enqueue_complex(h, s.dev<const void>(0), f.p.dtype, f.p.nframes, s.pitch(0), h->ws_cx);
}

}  // namespace fdoct_impl
