// fdoct_complex.cpp -- the extern "C" entry point of include/fdoct_complex.h (libfdoct_complex.so): the complex A-scan.  The chain is
// the core library's (fdoct_route.cpp: enqueue_complex, which routes the call to one of the two kernel families that write (re, im)
// pairs); what is this file's own is the call's arguments -- frames and pairs in host or device memory, planned as the capture
// entry points plan theirs (fdoct_capture_plan.h) -- and the D x H layout (fdoct_complex.hip).
#include "../../include/fdoct_complex.h"

#include "fdoct_capture_plan.h"
#include "fdoct_complex_kernels.h"

using namespace fdoct_impl;

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_process_complex(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                          float* out_re_im, fdoct_memspace out_space, fdoct_layout layout) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!frames || !out_re_im || nframes < 1 || !valid_mem(space) || !valid_mem(out_space) || !valid_layout(layout))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_process_complex: bad arguments");
  if (reinterpret_cast<uintptr_t>(out_re_im) % sizeof(float2))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_process_complex: out_re_im must be aligned to one (re, im) pair (8 bytes)");
  FramePlan p;
  if (int rc = plan_frames(h, "fdoct_process_complex", frames, dtype, space, nframes, pitch_bytes, &p)) return rc;
  size_t pairs = 0, out_bytes = 0, in_span = 0;
  if (__builtin_mul_overflow((size_t)nframes * (size_t)h->H, (size_t)h->D, &pairs) || __builtin_mul_overflow(pairs, sizeof(float2), &out_bytes) ||
      __builtin_mul_overflow(p.pitch, (size_t)p.raw_h * (size_t)nframes, &in_span))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_process_complex: the batch is too large");
  if (space == out_space && overlap(frames, in_span, out_re_im, out_bytes))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_process_complex: frames and out_re_im overlap");
  DEVICE_SCOPE(h);
  // every refusal and reservation before anything is enqueued: the staged arguments, the row-major intermediate of the D x H layout,
  // then the chain's own checks and its route on the frames where the kernels will read them (a run-time compile happens here)
  const bool transposed = layout == FDOCT_LAYOUT_TRANSPOSED_DxH;
  const int out = p.stage.out(out_re_im, out_space, out_bytes);
  if (int rc = stage_reserve(h, &p.stage)) return rc;
  if (transposed) {
    if (fdoct::cx_transpose_tiles(h->H, h->D, nframes) < 1) return fail(h, FDOCT_ERR_INVALID, "fdoct_process_complex: the batch is too large");
    if (int rc = h->ws_cx.reserve(h, out_bytes)) return rc;
  }
  if (int rc = enqueue_complex(h, p.stage.dev<const void>(0), dtype, nframes, p.stage.pitch(0), nullptr)) return rc;
  if (int rc = stage_upload(h, p.stage)) return rc;
  float2* const dst = p.stage.dev<float2>(out);
  if (int rc = enqueue_complex(h, p.stage.dev<const void>(0), dtype, nframes, p.stage.pitch(0), transposed ? static_cast<float2*>(h->ws_cx) : dst)) return rc;
  if (transposed) HIP_TRY(h, fdoct::launch_cx_transpose(h->ws_cx, dst, h->H, h->D, nframes, h->stream));
  return stage_finish(h, p.stage);
} FDOCT_CATCH(h)

}  // extern "C"
