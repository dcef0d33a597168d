// fdoct_colour.cpp -- the extern "C" entry points of include/fdoct_colour.h: the webcam's interleaved B,G,R frames
// (BscanFFTwebcam.cpp:1015-1038).  The handle's channelnum is read by the route (choose_route / run_passes_in_front,
// fdoct_route.cpp) and by the capture's plan / stage pair (fdoct_capture.cpp); the stage itself is run_colour over the kernels of
// fdoct_colour.hip.
#include "../../include/fdoct_colour.h"

#include "fdoct_colour_kernels.h"
#include "fdoct_ctx.h"

using namespace fdoct_impl;

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_set_colour_input(fdoct_handle h, int channelnum) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (channelnum < -1 || channelnum > 3)
    return fail(h, FDOCT_ERR_INVALID, "fdoct_set_colour_input: channelnum must be -1 (mono), 0, 1, 2 (B, G, R) or 3 (their sum)");
  h->colour = channelnum;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_get_colour_input(fdoct_handle h, int* channelnum) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!channelnum) return fail(h, FDOCT_ERR_INVALID, "fdoct_get_colour_input: no output");
  *channelnum = h->colour;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_colour_extract(fdoct_handle h, const void* bgr, fdoct_memspace space, int nframes, int raw_w, int raw_h, size_t pitch_bytes,
                         int channelnum, int mediann, int binx, int biny, void* out, fdoct_memspace out_space) try {
  // (the arguments first: their refusals need no handle, and fail() reports through fdoct_last_error(NULL) without one)
  if (!bgr || !out || !valid_mem(space) || !valid_mem(out_space) || nframes < 1 || raw_w < 1 || raw_h < 1)
    return fail(h, FDOCT_ERR_INVALID, "fdoct_colour_extract: bad arguments");
  if (int rc = colour_check(h, "fdoct_colour_extract", channelnum, FDOCT_U8, mediann)) return rc;
  if (binx < 1 || biny < 1 || raw_w % binx || raw_h % biny)
    return fail(h, FDOCT_ERR_INVALID, "fdoct_colour_extract: frame size must be a multiple of the bin factors");
  const size_t row = 3 * (size_t)raw_w;
  const size_t pitch = pitch_bytes ? pitch_bytes : row;
  if (pitch < row) return fail(h, FDOCT_ERR_INVALID, "fdoct_colour_extract: pitch smaller than a row of B,G,R pixels");
  if (!h) return FDOCT_ERR_INVALID;
  DEVICE_SCOPE(h);
  StagePlan sp;
  const int in = sp.in(bgr, space, row, (size_t)raw_h * nframes, pitch);  // host frames go up as packed, 16-byte-pitched rows
  sp.sync |= out_space == FDOCT_MEM_HOST;                                    // (out: copied from the stage's own workspace)
  if (int rc = stage_reserve(h, &sp)) return rc;
  if (int rc = run_colour(h, nullptr, nframes, raw_w, raw_h, sp.pitch(in), channelnum, mediann, binx, biny, nullptr, nullptr)) return rc;
  if (int rc = stage_upload(h, sp)) return rc;
  void* co = nullptr;
  size_t cp = 0;
  if (int rc = run_colour(h, sp.dev<const void>(in), nframes, raw_w, raw_h, sp.pitch(in), channelnum, mediann, binx, biny, &co, &cp)) return rc;
  const size_t out_row = (size_t)(raw_w / binx) * (channelnum == 3 ? sizeof(double) : 1);
  HIP_TRY(h, hipMemcpy2DAsync(out, out_row, co, cp, out_row, (size_t)(raw_h / biny) * nframes,
                              out_space == FDOCT_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
  return stage_finish(h, sp);
} FDOCT_CATCH(h)

double fdoct_colour_sum_scale(void) try { return fdoct::kColourSumScale; } FDOCT_CATCH_RETURN(nullptr, 0.0)

}  // extern "C"
