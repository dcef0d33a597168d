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

}  // namespace fdoct_impl
