// fdoct_capi.cpp -- the extern "C" boundary (include/fdoct.h) over the HIP kernels.
//
// Replaces the processing block of the reference's main() loop
// (BscanFFT.cpp:1123-1240 / BscanFFTsim.cpp:842-955) plus its one-time set-up
// (BscanFFT.cpp:544-698, 936-944).  No CPU compute path exists here: every
// fdoct_process* call runs the gfx950 kernels or fails.
#include "fdoct_ctx.h"

using namespace fdoct_impl;

using HandlePtr = std::unique_ptr<fdoct_ctx, int (*)(fdoct_handle)>;  // (deleter: fdoct_destroy)

// (drain, caught and the FDOCT_CATCH macros: fdoct_ctx.h, shared with fdoct_roi.cpp)

// ------------------------------------------------------------------ C ABI --
extern "C" {

#define FDOCT_STR_(x) #x
#define FDOCT_STR(x) FDOCT_STR_(x)
const char* fdoct_version(void) try { return "fdoct-amd " FDOCT_STR(FDOCT_VERSION_MAJOR) "." FDOCT_STR(FDOCT_VERSION_MINOR) " (gfx950)"; } FDOCT_CATCH_RETURN(nullptr, "")

int fdoct_build_resample_table(int width, int multiplier, int numfftpoints, double lambdamin, double lambdamax,
                               int32_t* nearestkindex, double* fractionalk) try {
  if (width < 2 || multiplier < 1 || numfftpoints < 1 || !nearestkindex || !fractionalk) return FDOCT_ERR_INVALID;
  std::vector<int32_t> idx;
  std::vector<double> frac;
  build_resample_table(width, multiplier, numfftpoints, lambdamin, lambdamax, idx, frac);
  std::memcpy(nearestkindex, idx.data(), sizeof(int32_t) * idx.size());
  std::memcpy(fractionalk, frac.data(), sizeof(double) * frac.size());
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_build_colormap_jet(unsigned char* bgr256) try {
  if (!bgr256) return FDOCT_ERR_INVALID;
  build_opencv_jet(bgr256);
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_build_window(int width, double* win) try {
  if (width < 2 || !win) return FDOCT_ERR_INVALID;
  std::vector<double> w;
  build_barthann(width, w);
  std::memcpy(win, w.data(), sizeof(double) * w.size());
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

const char* fdoct_last_error(fdoct_handle h) try { return h ? h->err.c_str() : g_create_error.c_str(); } FDOCT_CATCH_RETURN(h, "")

int fdoct_create(const fdoct_config* cfg, fdoct_handle* out) try {
  if (!cfg || !out) return fail(nullptr, FDOCT_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(fdoct_config)) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_config.struct_size mismatch");
  if (cfg->width < 8 || cfg->height < 1 || cfg->numfftpoints < 8)
    return fail(nullptr, FDOCT_ERR_INVALID, "width/height/numfftpoints out of range");
  if (cfg->numdisplaypoints < 1 || cfg->numdisplaypoints > cfg->numfftpoints)
    return fail(nullptr, FDOCT_ERR_INVALID, "numdisplaypoints out of range");
  if (!(cfg->lambdamax > cfg->lambdamin) || !(cfg->lambdamin > 0))
    return fail(nullptr, FDOCT_ERR_INVALID, "lambda range");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, FDOCT_ERR_DEVICE, "no HIP device: this library has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, FDOCT_ERR_INVALID, "device ordinal out of range");

  HandlePtr owned(new fdoct_ctx(), fdoct_destroy);  // a half-built handle is destroyed on every early return
  fdoct_ctx* h = owned.get();
  h->cfg = *cfg;
  h->W = cfg->width;
  h->H = cfg->height;
  h->N = cfg->numfftpoints;
  h->D = cfg->numdisplaypoints;
  h->M = cfg->increasefftpointsmultiplier > 0 ? cfg->increasefftpointsmultiplier : 1;
  h->A = cfg->averages > 0 ? cfg->averages : 1;
  if (cfg->variant == FDOCT_VARIANT_SIM) {  // sim:936-947 copies, it never accumulates: the chain runs one frame per B-scan
    h->sim_group = h->A;
    h->A = 1;
  }
  h->device = cfg->device;
  DeviceScope scope(h->device);  // the caller's current device is restored on every return path
  if (scope.err != hipSuccess) return fail(nullptr, FDOCT_ERR_DEVICE, "hipSetDevice failed");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) return fail(nullptr, FDOCT_ERR_DEVICE, "hipGetDeviceProperties failed");
  h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return fail(nullptr, FDOCT_ERR_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
  if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess)
    return fail(nullptr, FDOCT_ERR_DEVICE, "hipStreamCreate failed");
  h->stream = h->own_stream;
  for (auto& ev : h->ev)
    if (hipEventCreate(&ev) != hipSuccess) return fail(nullptr, FDOCT_ERR_DEVICE, "hipEventCreate failed");
  if (hipEventCreateWithFlags(&h->ev_order, hipEventDisableTiming) != hipSuccess) return fail(nullptr, FDOCT_ERR_DEVICE, "hipEventCreate failed");

  build_resample_table(h->W, h->M, h->N, cfg->lambdamin, cfg->lambdamax, h->idx, h->frac);
  build_barthann(h->W, h->win);
  if (int rc = adopt_plan(h, plan_inputs(h))) return fail(nullptr, rc, h->err);
  builtin_jet(h->lut);
  if (const char* e = std::getenv("FDOCT_NO_TRO")) h->tro_enabled = std::atoi(e) == 0;
  if (const char* e = std::getenv("FDOCT_JIT")) h->jit = std::atoi(e) != 0;
  if (const char* e = std::getenv("FDOCT_PRECISE_DIVISION")) h->precise_div = std::atoi(e) != 0;
  if (const char* e = std::getenv("FDOCT_TR_CHUNK_MB")) {  // tuning aid (tools/layout_bench.py): 0 = one chunk
    const long long mb = std::atoll(e);
    h->tr_chunk_bytes = mb > 0 ? (size_t)mb << 20 : ~(size_t)0 >> 1;
  }
  *out = owned.release();
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_destroy(fdoct_handle h) try {
  if (!h) return FDOCT_OK;
  DeviceScope scope(h->device);
  if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
  if (h->stream && h->stream != h->own_stream) (void)hipStreamSynchronize(h->stream);  // work we enqueued on the caller's stream
  if (h->s_in) (void)hipStreamSynchronize(h->s_in);
  if (h->s_out) (void)hipStreamSynchronize(h->s_out);
  h->copy_pool.reset();  // (its threads stop before anything else goes)
  for (auto& ev : h->ev)
    if (ev) (void)hipEventDestroy(ev);
  if (h->ev_order) (void)hipEventDestroy(h->ev_order);
  for (int b = 0; b < 2; b++)
    for (hipEvent_t e : {h->pe_in[b], h->pe_k[b], h->pe_out[b]})
      if (e) (void)hipEventDestroy(e);
  if (h->s_in) (void)hipStreamDestroy(h->s_in);
  if (h->s_out) (void)hipStreamDestroy(h->s_out);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;  // the buffers go last, with the handle
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_set_stream(fdoct_handle h, void* hip_stream) try {
  if (!h) return FDOCT_ERR_INVALID;
  const hipStream_t next = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->own_stream;
  if (next == h->stream) return FDOCT_OK;
  // The handle carries device state from call to call (tables, workspaces, the manual-averaging accumulator, the peak holds):
  // what it enqueues on the new stream runs behind everything it has enqueued on the old one.  No host wait.
  DEVICE_SCOPE(h);
  HIP_TRY(h, hipEventRecord(h->ev_order, h->stream));
  HIP_TRY(h, hipStreamWaitEvent(next, h->ev_order, 0));
  h->stream = next;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_set_background(fdoct_handle h, const void* data, fdoct_dtype dtype, int rows, size_t pitch_bytes) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!data) return fail(h, FDOCT_ERR_INVALID, "background data is null");
  return copy_ref_frame(h, h->yb, data, dtype, rows, pitch_bytes);
} FDOCT_CATCH(h)
int fdoct_set_pi_frame(fdoct_handle h, const void* data, fdoct_dtype dtype, int rows, size_t pitch_bytes) try {
  if (!h) return FDOCT_ERR_INVALID;
  return copy_ref_frame(h, h->yp, data, dtype, rows, pitch_bytes);
} FDOCT_CATCH(h)
int fdoct_set_dark(fdoct_handle h, const void* data, fdoct_dtype dtype, int rows, size_t pitch_bytes) try {
  if (!h) return FDOCT_ERR_INVALID;
  return copy_ref_frame(h, h->yd, data, dtype, rows, pitch_bytes);
} FDOCT_CATCH(h)

int fdoct_set_window(fdoct_handle h, const double* win, int n) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!win) {
    build_barthann(h->W, h->win);
    h->custom_win = false;
  } else {
    // W entries whatever the zero-pad multiplier is: the window is applied before the upsampling (main:1142, 1146)
    if (n != h->W) return fail(h, FDOCT_ERR_INVALID, "window length must equal width");
    h->win.assign(win, win + n);
    h->custom_win = true;
  }
  invalidate(h);
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_set_resample_table(fdoct_handle h, const int32_t* nearestkindex, const double* fractionalk, int n) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!nearestkindex || !fractionalk || n != h->N) return fail(h, FDOCT_ERR_INVALID, "table length must equal numfftpoints");
  for (int i = 0; i < n; i++)
    if (nearestkindex[i] < 0 || nearestkindex[i] >= h->W * h->M)
      return fail(h, FDOCT_ERR_INVALID, "nearestkindex entry outside the row");
  h->idx.assign(nearestkindex, nearestkindex + n);
  h->frac.assign(fractionalk, fractionalk + n);
  h->custom_table = true;
  invalidate(h);
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_set_lambda_range(fdoct_handle h, double lambdamin, double lambdamax) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!(lambdamax > lambdamin) || !(lambdamin > 0)) return fail(h, FDOCT_ERR_INVALID, "lambda range");
  h->cfg.lambdamin = lambdamin;
  h->cfg.lambdamax = lambdamax;
  build_resample_table(h->W, h->M, h->N, lambdamin, lambdamax, h->idx, h->frac);
  h->custom_table = false;
  invalidate(h);
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_set_dispersion_phase(fdoct_handle h, const float* cos_sin_pairs, int n) try {
  if (!h) return FDOCT_ERR_INVALID;
  std::vector<float> phase;
  if (cos_sin_pairs) {
    if (n != h->N) return fail(h, FDOCT_ERR_INVALID, "phase length must equal numfftpoints");
    phase.assign(cos_sin_pairs, cos_sin_pairs + 2 * (size_t)n);
  }
  PlanInputs in = plan_inputs(h);
  in.phase = !phase.empty();
  if (int rc = adopt_plan(h, in)) return rc;  // no kernel for the complex path at this size: the previous state stays
  h->phase.swap(phase);
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_get_resample_table(fdoct_handle h, int32_t* nearestkindex, double* fractionalk, int n) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (n != h->N) return fail(h, FDOCT_ERR_INVALID, "table length must equal numfftpoints");
  if (nearestkindex) std::memcpy(nearestkindex, h->idx.data(), sizeof(int32_t) * n);
  if (fractionalk) std::memcpy(fractionalk, h->frac.data(), sizeof(double) * n);
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_get_window(fdoct_handle h, double* win, int n) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!win || n != (int)h->win.size()) return fail(h, FDOCT_ERR_INVALID, "window length must equal width");
  std::memcpy(win, h->win.data(), sizeof(double) * n);
  return FDOCT_OK;
} FDOCT_CATCH(h)

// The call as fdoct_hostcall.h sees it: the handle's geometry, the arguments, and -- for host memory on both sides, the only calls
// whose buffers the pipeline may take as they are -- whether each buffer is pinned.  FDOCT_HOST_CHUNK_MB is read per call.
static HostCall host_call(const fdoct_ctx* h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                          const float* out_bscan, const float* out_db, fdoct_memspace out_space) {
  HostCallInputs in;
  in.W = h->W, in.H = h->H, in.D = h->D, in.A = h->A, in.sim_group = h->sim_group, in.fe_binx = h->fe_binx, in.fe_biny = h->fe_biny;
  in.pixel_bytes = frame_pixel_bytes(h, dtype);  // a colour handle's rows hold 3 bytes per pixel: chunks, strides and staging follow
  in.pitch_bytes = pitch_bytes, in.frames = frames != nullptr, in.nframes = nframes, in.space = space, in.out_space = out_space;
  in.want_bscan = out_bscan != nullptr, in.want_db = out_db != nullptr;
  if (frames && space == FDOCT_MEM_HOST && out_space == FDOCT_MEM_HOST) {
    in.frames_pinned = host_pointer_is_pinned(frames);
    in.bscan_pinned = !out_bscan || host_pointer_is_pinned(out_bscan);
    in.db_pinned = !out_db || host_pointer_is_pinned(out_db);
  }
  if (const char* e = std::getenv("FDOCT_HOST_CHUNK_MB")) in.chunk_mb = std::atoll(e);  // tuning aid (tools/pcie_chunk.py)
  return make_host_call(in);
}

// SimFrames::Gather (fdoct_hostcall.h) carried out: one strided copy on the handle's stream, from host or device memory, packs the
// last frame of every group into ws_sim with the caller's row pitch and re-points the call at it, device-resident.  (The frame on
// which the reference EMITS, the (S + 1)-th of its loop, is computed and dropped there, sim:944-947: it never reaches an output,
// so it is the caller's to skip.)
static int sim_last_frames(fdoct_ctx* h, const HostCall& call, const void** frames, fdoct_memspace* space) {
  if (call.sim != SimFrames::Gather) return FDOCT_OK;
  const size_t frame_bytes = call.pitch * (size_t)call.rows_per_frame;  // raw camera rows when a front end is set
  DEVICE_SCOPE(h);
  if (int rc = h->ws_sim.reserve(h, frame_bytes * (size_t)call.nframes)) return rc;
  HIP_TRY(h, hipMemcpy2DAsync(h->ws_sim, frame_bytes, static_cast<const unsigned char*>(*frames) + call.first_byte, call.frame_stride, frame_bytes,
                              (size_t)call.nframes, *space == FDOCT_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->stream));
  *frames = h->ws_sim;
  *space = FDOCT_MEM_DEVICE;
  return FDOCT_OK;
}

int fdoct_process_async(fdoct_handle h, const void* d_frames, fdoct_dtype dtype, int nframes, size_t pitch_bytes,
                        float* d_out_bscan, float* d_out_db, fdoct_layout layout) try {
  if (!h) return FDOCT_ERR_INVALID;
  fdoct_memspace space = FDOCT_MEM_DEVICE;
  if (h->colour >= 0)
    if (int rc = colour_check(h, "colour input", h->colour, dtype, h->fe_median)) return rc;
  const HostCall call = host_call(h, d_frames, dtype, space, nframes, pitch_bytes, d_out_bscan, d_out_db, FDOCT_MEM_DEVICE);
  if (call.rc) return fail(h, call.rc, call.why);
  if (int rc = check_call(h, dtype, pitch_bytes, d_out_bscan, d_out_db)) return rc;
  if (int rc = sim_last_frames(h, call, &d_frames, &space)) return rc;
  h->record_now = h->async_timing;
  return enqueue(h, d_frames, dtype, call.nframes, pitch_bytes, d_out_bscan, d_out_db, layout);
} FDOCT_CATCH(h)

int fdoct_set_timing(fdoct_handle h, int on) try {
  if (!h) return FDOCT_ERR_INVALID;
  h->async_timing = on != 0;
  return FDOCT_OK;
} FDOCT_CATCH(h)

// Did a wave of a transposed-store launch give up waiting (FusedArgs::tr_fault)?  The word lives in pinned host memory, so
// this is a plain read: after a synchronisation point it is final for the work synchronised on, anywhere else (the next
// enqueue, fdoct_get_timing -- callers of the async API who wait on their own stream or event) it reports what has been
// raised so far.  The fault is reported once and cleared.
static int check_tro_fault(fdoct_ctx* h) {
  if (!h->d_tro_fault) return FDOCT_OK;
  volatile unsigned* w = h->d_tro_fault;
  if (*w) {
    *w = 0u;
    return fail(h, FDOCT_ERR_DEVICE, "transposed store: a wave timed out waiting for its tile buffer; results of the transposed-layout calls since the last check are invalid");
  }
  return FDOCT_OK;
}

int fdoct_synchronize(fdoct_handle h) try {
  if (!h) return FDOCT_ERR_INVALID;
  DEVICE_SCOPE(h);
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return check_tro_fault(h);
} FDOCT_CATCH(h)

int fdoct_get_host_staging(fdoct_handle h) try {
  if (!h) return FDOCT_ERR_INVALID;
  return copy_thread_count(h);
} FDOCT_CATCH(h)

int fdoct_set_host_staging(fdoct_handle h, int threads) try {
  if (!h) return FDOCT_ERR_INVALID;
  const int want = threads < 0 ? -1 : std::min(threads, 64);
  if (want != h->host_staging) {  // the pool is sized when it starts: a new count means a new pool (no batch is in flight here)
    h->copy_pool.reset();
  }
  h->host_staging = want;
  return FDOCT_OK;
} FDOCT_CATCH(h)

void* fdoct_host_alloc(size_t bytes) try {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
} FDOCT_CATCH_RETURN(nullptr, nullptr)

void fdoct_host_free(void* p) try {
  if (p) (void)hipHostFree(p);
} FDOCT_CATCH_VOID(nullptr)

int fdoct_process(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes,
                  size_t pitch_bytes, float* out_bscan, float* out_db, fdoct_memspace out_space,
                  fdoct_layout layout) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!frames || nframes <= 0) return fail(h, FDOCT_ERR_INVALID, "no frames");
  if (h->colour >= 0)
    if (int rc = colour_check(h, "colour input", h->colour, dtype, h->fe_median)) return rc;
  DEVICE_SCOPE(h);
  const HostCall call = host_call(h, frames, dtype, space, nframes, pitch_bytes, out_bscan, out_db, out_space);
  if (call.rc) return fail(h, call.rc, call.why);
  if (int rc = check_call(h, dtype, pitch_bytes, out_bscan, out_db)) return rc;
  // ---- nothing has been enqueued up to here: everything that can refuse the call without a route has
  int rc;
  if (call.path == HostPath::Pipelined) {
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = process_pipelined(h, call, frames, dtype, out_bscan, out_db, layout))) return rc;
    if ((rc = check_tro_fault(h))) return rc;
    h->timing_pending = false;  // no per-call device events here: report the wall time of the whole pipeline
    h->timing.last_process_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    h->timing.last_kernel_ms = h->timing.resample_stage_ms = h->timing.fft_stage_ms = 0.0;
    h->timing.ascans = (uint64_t)call.in_rows;
    h->record_now = true;
    return FDOCT_OK;
  }
  if ((rc = sim_last_frames(h, call, &frames, &space))) return rc;
  StagePlan sp;  // host frames go up packed and aligned, host outputs come down (the PCIe-inclusive path)
  const int in = sp.in(frames, space, call.row_bytes, (size_t)call.in_rows, call.pitch);
  const int mag = sp.out(out_bscan, out_space, call.out_elems * 4), db = sp.out(out_db, out_space, call.out_elems * 4);
  sp.sync = true;  // (device-resident arguments too: this is the synchronous call)
  if ((rc = stage_begin(h, &sp))) return rc;
  h->record_now = true;
  if ((rc = enqueue(h, sp.dev<const void>(in), dtype, call.nframes, sp.pitch(in), sp.dev<float>(mag), sp.dev<float>(db), layout))) return rc;
  if ((rc = stage_finish(h, sp))) return rc;
  return check_tro_fault(h);
} FDOCT_CATCH(h)

int fdoct_get_timing(fdoct_handle h, fdoct_timing* t) try {
  if (!h || !t) return FDOCT_ERR_INVALID;
  if (h->timing_pending) {
    DEVICE_SCOPE(h);
    HIP_TRY(h, hipEventSynchronize(h->ev[3]));
    float ms = 0.f;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[3]));
    h->timing.last_process_ms = ms;
    HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
    h->timing.last_kernel_ms = ms;
    h->timing.resample_stage_ms = h->timing.fft_stage_ms = 0.0;
    if (h->timing_staged) {
      HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[1], h->ev[4]));
      h->timing.resample_stage_ms = ms;
      HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[4], h->ev[2]));
      h->timing.fft_stage_ms = ms;
    }
    h->timing_pending = false;
    if (int frc = check_tro_fault(h)) return frc;
  } else if (!h->record_now) {
    h->timing.last_process_ms = h->timing.last_kernel_ms = h->timing.resample_stage_ms = h->timing.fft_stage_ms = 0.0;
  }
  *t = h->timing;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_set_launch(fdoct_handle h, int threads_per_block, int blocks) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (threads_per_block < 0 || threads_per_block % 64 || threads_per_block > FDOCT_MAX_BLOCK || blocks < 0)
    return fail(h, FDOCT_ERR_INVALID, "threads_per_block must be a multiple of 64 up to the build's block limit");
  h->block_override = threads_per_block;
  h->grid_override = blocks;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_set_plan(fdoct_handle h, int plan_id, int force_general_kernel) try {
  if (!h) return FDOCT_ERR_INVALID;
  FusedPlan q{};
  if (plan_id >= 0 && !fused_plan_get(plan_id, &q)) return fail(h, FDOCT_ERR_INVALID, "unknown plan id");
  if (plan_id < -3) return fail(h, FDOCT_ERR_INVALID, "plan id: -1 automatic, -2 the workgroup-per-row kernel, -3 the long-row path");
  PlanInputs in = plan_inputs(h);
  in.plan_override = plan_id;
  in.force_general = force_general_kernel != 0;
  if (int rc = adopt_plan(h, in)) return rc;
  h->plan_override = in.plan_override;
  h->force_general = in.force_general;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_set_frontend(fdoct_handle h, int mediann, int binx, int biny) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (binx < 1 || biny < 1 || (mediann != 0 && mediann != 3 && mediann != 5 && mediann != 7))
    return fail(h, FDOCT_ERR_INVALID, "mediann must be 0/3/5/7 and the bin factors >= 1");
  h->fe_median = mediann;
  h->fe_binx = binx;
  h->fe_biny = biny;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_frontend(fdoct_handle h, const void* raw, fdoct_dtype dtype, int nframes, int raw_w, int raw_h, size_t pitch_bytes,
                   int mediann, int binx, int biny, void* out) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!raw || !out || nframes <= 0 || raw_w <= 0 || raw_h <= 0) return fail(h, FDOCT_ERR_INVALID, "fdoct_frontend: bad arguments");
  if (dtype != FDOCT_U8 && dtype != FDOCT_U16)
    return fail(h, FDOCT_ERR_UNSUPPORTED, "the front end takes 8- or 16-bit camera frames");
  const int kdt = kernel_dtype(dtype);
  const size_t es = dtype_size(dtype);
  if (pitch_bytes == 0) pitch_bytes = es * raw_w;
  if (pitch_bytes < es * raw_w) return fail(h, FDOCT_ERR_INVALID, "pitch smaller than a raw camera row");
  DEVICE_SCOPE(h);
  int rc;
  StagePlan sp;
  const int in = sp.in(raw, FDOCT_MEM_HOST, es * raw_w, (size_t)raw_h * nframes, pitch_bytes);
  sp.sync = true;  // (out is host memory: copied from the front end's own workspace)
  if ((rc = stage_reserve(h, &sp))) return rc;
  if ((rc = run_frontend(h, nullptr, kdt, nframes, raw_w, raw_h, 0, mediann, binx, biny, nullptr, nullptr))) return rc;
  if ((rc = stage_upload(h, sp))) return rc;
  void* fo = nullptr;
  size_t fp = 0;
  if ((rc = run_frontend(h, sp.dev<void>(in), kdt, nframes, raw_w, raw_h, sp.pitch(in), mediann, binx, biny, &fo, &fp))) return rc;
  const int ow = raw_w / binx, oh = raw_h / biny;
  HIP_TRY(h, hipMemcpy2DAsync(out, es * ow, fo, fp, es * ow, (size_t)oh * nframes, hipMemcpyDeviceToHost, h->stream));
  return stage_finish(h, sp);
} FDOCT_CATCH(h)

int fdoct_set_colormap(fdoct_handle h, const unsigned char* bgr256) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (bgr256)
    std::memcpy(h->lut, bgr256, 768);
  else
    builtin_jet(h->lut);
  h->lut_dirty = true;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_get_colormap(fdoct_handle h, unsigned char* bgr256) try {
  if (!h || !bgr256) return FDOCT_ERR_INVALID;
  std::memcpy(bgr256, h->lut, 768);
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_display(fdoct_handle h, const float* bscandb, fdoct_memspace in_mem, int nbscans, int rows, int cols,
                  double bscanthreshold, int clampupper, unsigned char* out_gray, unsigned char* out_bgr,
                  fdoct_memspace out_mem) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!bscandb || nbscans <= 0 || rows <= 0 || cols <= 0) return fail(h, FDOCT_ERR_INVALID, "fdoct_display: bad arguments");
  if (!out_gray && !out_bgr) return fail(h, FDOCT_ERR_INVALID, "fdoct_display: no output requested");
  if (clampupper && (rows <= 5 || cols <= 5)) return fail(h, FDOCT_ERR_INVALID, "clampupper needs a B-scan larger than 5x5");
  DEVICE_SCOPE(h);
  int rc;
  const long long count = (long long)rows * cols;
  const size_t total = (size_t)count * nbscans;
  StagePlan sp;
  const int in = sp.in(bscandb, in_mem, total * sizeof(float)), gray = sp.out(out_gray, out_mem, total), bgr = sp.out(out_bgr, out_mem, 3 * total);
  if ((rc = stage_reserve(h, &sp))) return rc;
  if (!h->d_lut && (rc = h->d_lut.assign(h, 768))) return rc;
  if ((rc = h->d_disp_part.reserve(h, (size_t)nbscans * display_parts(count) * 2 * sizeof(double)))) return rc;
  if ((rc = stage_upload(h, sp))) return rc;
  if (h->lut_dirty) {  // (true until an upload has succeeded: a d_lut just made is covered)
    HIP_TRY(h, hipMemcpyAsync(h->d_lut, h->lut, 768, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // h->lut may change right after we return
    h->lut_dirty = false;
  }
  const long long clamp_at = clampupper ? 5LL * cols + 5 : -1;  // bscandisp.at<double>(5, 5), main:1252
  HIP_TRY(h, launch_display(sp.dev<const float>(in), count, nbscans, bscanthreshold, clamp_at, h->d_disp_part, h->d_lut,
                            sp.dev<unsigned char>(gray), sp.dev<unsigned char>(bgr), h->stream));
  return stage_finish(h, sp);
} FDOCT_CATCH(h)

int fdoct_lockin_db(fdoct_handle h, const float* bscan, const float* jscan, fdoct_memspace mem, int nbscans, size_t count,
                    float* out_db) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!bscan || !jscan || !out_db || nbscans <= 0 || count == 0) return fail(h, FDOCT_ERR_INVALID, "fdoct_lockin_db: bad arguments");
  DEVICE_SCOPE(h);
  const size_t total = count * (size_t)nbscans;
  if (mem != FDOCT_MEM_DEVICE) mem = FDOCT_MEM_HOST;  // (every other value has always read as host memory here)
  StagePlan sp;
  const int b = sp.in(bscan, mem, total * sizeof(float)), j = sp.in(jscan, mem, count * sizeof(float));
  const int o = sp.out(out_db, mem, total * sizeof(float));
  if (int rc = stage_begin(h, &sp)) return rc;
  HIP_TRY(h, launch_lockin_db(sp.dev<const float>(b), sp.dev<const float>(j), (long long)total, (long long)count, sp.dev<float>(o), h->stream));
  return stage_finish(h, sp);
} FDOCT_CATCH(h)

int fdoct_set_averages(fdoct_handle h, int averages) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (averages < 1) return fail(h, FDOCT_ERR_INVALID, "averages must be >= 1");
  if (h->cfg.variant == FDOCT_VARIANT_SIM)
    h->sim_group = averages;  // (fdoct_hostcall.h: the last frame of every group is what the reference emits)
  else
    h->A = averages;  // a launch parameter only: no table depends on it
  h->cfg.averages = averages;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_set_bandpass(fdoct_handle h, int on) try {
  if (!h) return FDOCT_ERR_INVALID;
  h->bandpass = on != 0;  // takes effect inside the zero-pad stage (increasefftpointsmultiplier > 1), as in the reference
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_set_staged(fdoct_handle h, int on) try {
  if (!h) return FDOCT_ERR_INVALID;
  h->staged = on != 0;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_prepare(fdoct_handle h, fdoct_dtype dtype, fdoct_layout layout) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!h->yb.rows) return fail(h, FDOCT_ERR_STATE, "no background set (fdoct_set_background)");
  const size_t es = frame_pixel_bytes(h, dtype);
  if (!es) return fail(h, FDOCT_ERR_INVALID, "bad dtype");
  DEVICE_SCOPE(h);
  // the call fdoct_process* will see: aligned device frames, packed rows, one averaging group, both images asked for
  Route r;
  RouteInputs in = route_inputs(h, dtype, 0, es * (size_t)h->W * h->fe_binx, h->A);
  in.layout = layout;
  if (int rc = choose_route(h, in, &r)) return rc;
  return r.family;
} FDOCT_CATCH(h)

int fdoct_set_precise_division(fdoct_handle h, int on) try {
  if (!h) return FDOCT_ERR_INVALID;
  h->precise_div = on != 0;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_set_jit(fdoct_handle h, int on) try {
  if (!h) return FDOCT_ERR_INVALID;
  h->jit = on != 0;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_last_kernel(fdoct_handle h) try { return h ? h->last_kernel : FDOCT_KERNEL_NONE; } FDOCT_CATCH(h)

const char* fdoct_jit_note(fdoct_handle h) try { return h ? h->jit_note.c_str() : ""; } FDOCT_CATCH_RETURN(h, "")

long long fdoct_jit_compile_check(int width, int multiplier, int numfftpoints, int numdisplaypoints, fdoct_dtype dtype, const char* gcn_arch,
                                  char* why, int why_len) try {
  std::string reason;
  long long n = -1;
  const int kdt = kernel_dtype(dtype);
  // (FDOCT_JIT_CHECK_OPT: the kernel's option mask -- fdoct_wave.h, FDOCT_WAVE_OPT_* -- for build checks of the optional stages; the
  // shape is judged with it, as a call's route judges it: a display beyond numfftpoints / 2 needs the mirror option or complex rows)
  const char* eo = std::getenv("FDOCT_JIT_CHECK_OPT");
  const int opt = eo ? std::atoi(eo) : 0;
  if (!gcn_arch || !*gcn_arch)
    reason = "no architecture named";
  else if (!wave_jit_shape_ok(width, multiplier, numfftpoints, numdisplaypoints, opt))
    reason = "the wave-per-row kernel cannot take this shape";
  else
    n = wave_jit_compile_only(width, multiplier, numfftpoints, kdt, numdisplaypoints, opt, gcn_arch, &reason);
  if (why && why_len > 0) std::snprintf(why, (size_t)why_len, "%s", reason.c_str());
  return n;
} FDOCT_CATCH_RETURN(nullptr, -1)

int fdoct_device_count(void) try {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess) return 0;
  return ndev > 0 ? ndev : 0;
} FDOCT_CATCH(nullptr)

int fdoct_shard_frames(int nframes_total, int averages, int part, int nparts, int* first, int* count) try {
  if (nframes_total < 0 || averages < 1 || nparts < 1 || part < 0 || part >= nparts || !first || !count) return FDOCT_ERR_INVALID;
  const int groups = nframes_total / averages, base = groups / nparts, extra = groups % nparts;
  const int g0 = part * base + (part < extra ? part : extra);
  const int g1 = g0 + base + (part < extra ? 1 : 0);
  *first = g0 * averages;
  *count = (g1 - g0) * averages;
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_clone_to_device(fdoct_handle h, int device, fdoct_handle* out) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!out) return fail(h, FDOCT_ERR_INVALID, "fdoct_clone_to_device: null output");
  *out = nullptr;
  fdoct_config cfg = h->cfg;
  cfg.device = device;
  cfg.averages = h->cfg.variant == FDOCT_VARIANT_SIM ? h->sim_group : h->A;
  fdoct_handle c = nullptr;
  int rc = fdoct_create(&cfg, &c);
  if (rc) return fail(h, rc, std::string("fdoct_clone_to_device: ") + fdoct_last_error(nullptr));
  HandlePtr owned(c, fdoct_destroy);  // destroyed on every return but the last
  // constant state: the same blob the multi-process set-up broadcasts (host memory; the device tables of the clone are
  // built on ITS device at the first call, like any handle's)
  size_t used = 0;
  rc = fdoct_export_state(h, nullptr, 0, &used);
  std::vector<unsigned char> blob(used);
  if (!rc) rc = fdoct_export_state(h, blob.data(), blob.size(), &used);
  if (!rc) rc = fdoct_import_state(c, blob.data(), blob.size());
  if (rc) {
    return fail(h, rc, "fdoct_clone_to_device: " + (rc == FDOCT_ERR_INVALID ? c->err : h->err));
  }
  // run-time settings
  c->fe_median = h->fe_median;
  c->fe_binx = h->fe_binx;
  c->fe_biny = h->fe_biny;
  c->cap_lowpass = h->cap_lowpass;
  c->cap_raw = h->cap_raw;
  c->colour = h->colour;
  c->bandpass = h->bandpass;
  c->jit = h->jit;
  c->precise_div = h->precise_div;
  c->raw_mag = h->raw_mag;
  c->staged = h->staged;
  c->async_timing = h->async_timing;
  c->host_staging = h->host_staging;  // (the setting: the clone starts its own copy threads)
  c->force_general = h->force_general;
  c->plan_override = h->plan_override;
  c->block_override = h->block_override;
  c->grid_override = h->grid_override;
  std::memcpy(c->lut, h->lut, sizeof c->lut);
  c->lut_dirty = true;
  if ((rc = adopt_plan(c, plan_inputs(c)))) return fail(h, rc, "fdoct_clone_to_device: " + c->err);
  *out = owned.release();
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_get_ylin(fdoct_handle h, long long row0, int nrows, double* out) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!out || nrows <= 0 || row0 < 0) return fail(h, FDOCT_ERR_INVALID, "fdoct_get_ylin: bad arguments");
  if (!h->ylin_rows || !h->ws_ylin) return fail(h, FDOCT_ERR_STATE, "fdoct_get_ylin: the last run was not a staged one (fdoct_set_staged)");
  if (row0 + nrows > h->ylin_rows) return fail(h, FDOCT_ERR_INVALID, "fdoct_get_ylin: rows past the end of the last batch");
  DEVICE_SCOPE(h);
  const int NC = h->plan.NC, N = h->N;
  std::vector<float2> z((size_t)nrows * NC);
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(z.data(), h->ws_ylin + (size_t)row0 * NC, z.size() * sizeof(float2), hipMemcpyDeviceToHost));
  for (int r = 0; r < nrows; r++) {
    const float2* zr = z.data() + (size_t)r * NC;
    double* o = out + (size_t)r * N;
    if (h->plan.cplx) {
      // complex path: the stage stores data_ylin[q] * (cos, sin)[q]; the phasors have unit modulus
      for (int q = 0; q < N; q++) o[q] = (double)zr[q].x * h->phase[2 * q] + (double)zr[q].y * h->phase[2 * q + 1];
    } else {
      // real path: FFT point n packs (data_ylin[2n], data_ylin[2n+1]), with the untangle's 1/2 folded into the window
      for (int n = 0; n < NC; n++) {
        o[2 * n] = 2.0 * (double)zr[n].x;
        o[2 * n + 1] = 2.0 * (double)zr[n].y;
      }
    }
  }
  return FDOCT_OK;
} FDOCT_CATCH(h)

// ---- state blob (format 2): 12 x int32 header {magic, version, W, H, N, M, yb_rows, yp_rows, yd_rows, nphase floats,
// window length, flags (bit 0 custom window, bit 1 custom resample table)}, then yb, yp, yd, window, fractionalk as
// doubles, nearestkindex as int32, the phase as floats.  The window has W entries whatever the zero-pad multiplier is:
// it is applied before the upsampling (main:1142 precedes main:1146).
static const int32_t kStateMagic = 0x46444f43;  // 'FDOC'
static const int32_t kStateVersion = 2;
static const size_t kStateHeader = 12 * sizeof(int32_t);

// The set-up broadcast of the multi-GPU arrangement with one process per GPU, for a C / C++ host that has an RCCL
// communicator: rank `root` exports its constant state, the blob's size and bytes travel as two ncclBroadcast calls over
// device buffers on the handle's stream, the other ranks import it.  librccl is looked up at run time (dlopen: a host that
// never calls this does not need it); the communicator and its lifetime are the caller's.  A one-rank communicator is a plain
// export / import round trip.
int fdoct_broadcast_state_rccl(fdoct_handle h, void* nccl_comm, int root) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!nccl_comm) return fail(h, FDOCT_ERR_INVALID, "fdoct_broadcast_state_rccl: null communicator");
  // (the entry points used, by their documented C signatures: ncclResult_t is an int with 0 = success, ncclUint8 = 1,
  // ncclUint64 = 5 in every NCCL / RCCL 2.x header -- ncclGetVersion is asked before those values are relied on)
  typedef int (*bcast_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
  typedef int (*rank_fn)(const void*, int*);
  typedef int (*version_fn)(int*);
  typedef const char* (*err_fn)(int);
  static void* lib = nullptr;
  static bcast_fn nccl_broadcast = nullptr;
  static rank_fn nccl_rank = nullptr, nccl_count = nullptr;
  static err_fn nccl_err = nullptr;
  static int nccl_major = 0;
  static std::once_flag once;  // (handles on several devices may call this from several host threads)
  std::call_once(once, [] {
    for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so", "libnccl.so.2"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (lib) break;
    }
    if (!lib) return;
    nccl_broadcast = reinterpret_cast<bcast_fn>(dlsym(lib, "ncclBroadcast"));
    nccl_rank = reinterpret_cast<rank_fn>(dlsym(lib, "ncclCommUserRank"));
    nccl_count = reinterpret_cast<rank_fn>(dlsym(lib, "ncclCommCount"));
    nccl_err = reinterpret_cast<err_fn>(dlsym(lib, "ncclGetErrorString"));
    if (version_fn getv = reinterpret_cast<version_fn>(dlsym(lib, "ncclGetVersion"))) {
      int v = 0;   // 2.x.y: 2000 + 100 x + y up to 2.8, 20000 + 100 x + y from 2.9
      if (getv(&v) == 0) nccl_major = v >= 10000 ? v / 10000 : v / 1000;
    }
  });
  if (!lib) return fail(h, FDOCT_ERR_UNSUPPORTED, "fdoct_broadcast_state_rccl: librccl.so not found");
  if (!nccl_broadcast || !nccl_rank || !nccl_count) return fail(h, FDOCT_ERR_UNSUPPORTED, "fdoct_broadcast_state_rccl: librccl.so lacks ncclBroadcast / ncclCommUserRank / ncclCommCount");
  if (nccl_major != 2) return fail(h, FDOCT_ERR_UNSUPPORTED, "fdoct_broadcast_state_rccl: the collective library does not report a 2.x version (ncclGetVersion); its datatype codes are not known here");
  auto nccl_try = [&](int r, const char* what) -> int {
    if (r == 0) return FDOCT_OK;
    return fail(h, FDOCT_ERR_DEVICE, std::string(what) + ": " + (nccl_err ? nccl_err(r) : "RCCL error"));
  };
  DEVICE_SCOPE(h);
  int rank = -1, count = 0, rc;
  if ((rc = nccl_try(nccl_rank(nccl_comm, &rank), "ncclCommUserRank"))) return rc;
  if ((rc = nccl_try(nccl_count(nccl_comm, &count), "ncclCommCount"))) return rc;
  if (root < 0 || root >= count) return fail(h, FDOCT_ERR_INVALID, "fdoct_broadcast_state_rccl: root outside the communicator");
  // Everything that can fail on ONE rank alone happens before the first collective: the export on the root, the
  // device buffers -- a size word and one fixed-size chunk the blob travels through, so that nothing is allocated between the
  // collectives.  A root that cannot export still takes part in the size broadcast, with 0, and every rank returns an error; a
  // rank that fails HERE returns without having entered a collective -- the others then wait in theirs, and the caller must
  // ncclCommAbort the communicator (include/fdoct.h says so).
  const size_t kChunk = (size_t)4 << 20;
  std::vector<unsigned char> blob;
  unsigned long long nbytes = 0;
  int root_rc = FDOCT_OK;
  if (rank == root) {
    size_t used = 0;
    root_rc = fdoct_export_state(h, nullptr, 0, &used);
    if (!root_rc) {
      try {
        blob.resize(used);
      } catch (...) {   // (caught here, not at the boundary: the root still takes part in the size broadcast, with 0, and every rank returns an error)
        blob.clear();
        root_rc = fail(h, FDOCT_ERR_NOMEM, "fdoct_broadcast_state_rccl: no host memory for the state blob on the root");
      }
    }
    if (!root_rc) root_rc = fdoct_export_state(h, blob.data(), blob.size(), &used);
    nbytes = root_rc ? 0 : used;
  }
  hipStream_t st = h->stream;
  DevBuf<unsigned long long> d_n;
  DevBuf<unsigned char> d_chunk;
  if (d_n.assign(h, 1) || d_chunk.assign(h, kChunk))
    return fail(h, FDOCT_ERR_NOMEM, "fdoct_broadcast_state_rccl: no device memory for the staging buffers (no collective was entered: abort the communicator)");
  if (hipMemcpyAsync(d_n, &nbytes, sizeof nbytes, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return fail(h, FDOCT_ERR_DEVICE, "fdoct_broadcast_state_rccl: copy of the blob size failed (no collective was entered: abort the communicator)");
  // ---- collective 1: the size
  if ((rc = nccl_try(nccl_broadcast(d_n, d_n, 1, /*ncclUint64*/ 5, root, nccl_comm, st), "ncclBroadcast (size)"))) return rc;
  if (hipMemcpyAsync(&nbytes, d_n, sizeof nbytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess ||
      nbytes > (1ull << 34)) {
    // (this rank cannot know how many chunk broadcasts follow, so it cannot stay in step with the others: include/fdoct.h
    // documents this exit next to the pre-collective ones)
    return fail(h, FDOCT_ERR_DEVICE, "fdoct_broadcast_state_rccl: the broadcast blob size could not be read back or is implausible (this rank leaves "
                                     "before the chunk broadcasts: abort the communicator)");
  }
  if (nbytes == 0)  // the root had nothing to send: every rank returns an error, nobody is left in a later broadcast
    return root_rc ? root_rc : fail(h, FDOCT_ERR_INVALID, "fdoct_broadcast_state_rccl: the root rank could not export its state");
  // ---- collectives 2 ...: the blob, chunk by chunk through the staging buffer.  A copy that fails from here on does not
  // take this rank out of the remaining broadcasts (the others would wait in them): the error is returned at the end.
  if (rank != root) {
    try {
      blob.resize(nbytes);
    } catch (...) {   // (caught here, not at the boundary: a rank without host memory must still take part in the chunk broadcasts)
      blob.clear();   // (no host memory: keep taking part, report afterwards)
    }
  }
  int late = FDOCT_OK;
  for (unsigned long long off = 0; off < nbytes; off += kChunk) {
    const size_t n = (size_t)std::min<unsigned long long>(kChunk, nbytes - off);
    if (rank == root && hipMemcpyAsync(d_chunk, blob.data() + off, n, hipMemcpyHostToDevice, st) != hipSuccess && !late)
      late = fail(h, FDOCT_ERR_DEVICE, "fdoct_broadcast_state_rccl: upload of the blob failed");
    if ((rc = nccl_try(nccl_broadcast(d_chunk, d_chunk, n, /*ncclUint8*/ 1, root, nccl_comm, st), "ncclBroadcast (blob)")))
      return rc;   // (the collective itself failed: the communicator is in error for every rank)
    if (rank != root && !blob.empty()) {
      if ((hipMemcpyAsync(blob.data() + off, d_chunk, n, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) && !late)
        late = fail(h, FDOCT_ERR_DEVICE, "fdoct_broadcast_state_rccl: download of the blob failed");
    } else if (hipStreamSynchronize(st) != hipSuccess && !late) {  // the chunk buffer is reused by the next round
      late = fail(h, FDOCT_ERR_DEVICE, "fdoct_broadcast_state_rccl: stream error during the blob broadcast");
    }
  }
  if (late) return late;
  if (blob.size() != nbytes) return fail(h, FDOCT_ERR_NOMEM, "fdoct_broadcast_state_rccl: no host memory for the blob");
  // (the root imports its own blob too: every rank ends in the state the blob describes, validated the same way)
  return fdoct_import_state(h, blob.data(), blob.size());
} FDOCT_CATCH(h)

int fdoct_export_state(fdoct_handle h, void* buf, size_t cap, size_t* used) try {
  if (!h || !used) return FDOCT_ERR_INVALID;
  const size_t need = kStateHeader + (h->yb.v.size() + h->yp.v.size() + h->yd.v.size() + h->win.size() + h->frac.size()) * 8 +
                      h->idx.size() * 4 + h->phase.size() * 4;
  *used = need;
  if (!buf) return FDOCT_OK;
  if (cap < need) return fail(h, FDOCT_ERR_INVALID, "state buffer too small");
  unsigned char* p = static_cast<unsigned char*>(buf);
  const int32_t hdr[12] = {kStateMagic, kStateVersion, h->W, h->H, h->N, h->M, h->yb.rows, h->yp.rows, h->yd.rows,
                           (int32_t)h->phase.size(), (int32_t)h->win.size(), (h->custom_win ? 1 : 0) | (h->custom_table ? 2 : 0)};
  std::memcpy(p, hdr, sizeof hdr);
  p += sizeof hdr;
  auto put = [&](const void* src, size_t bytes) {
    if (bytes) std::memcpy(p, src, bytes);
    p += bytes;
  };
  put(h->yb.v.data(), h->yb.v.size() * 8);
  put(h->yp.v.data(), h->yp.v.size() * 8);
  put(h->yd.v.data(), h->yd.v.size() * 8);
  put(h->win.data(), h->win.size() * 8);
  put(h->frac.data(), h->frac.size() * 8);
  put(h->idx.data(), h->idx.size() * 4);
  put(h->phase.data(), h->phase.size() * 4);
  return FDOCT_OK;
} FDOCT_CATCH(h)

// Everything is parsed and checked into temporaries first: a blob that fails any check leaves the handle untouched.
int fdoct_import_state(fdoct_handle h, const void* buf, size_t len) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!buf || len < kStateHeader) return fail(h, FDOCT_ERR_INVALID, "state blob too short");
  const unsigned char* p = static_cast<const unsigned char*>(buf);
  int32_t hdr[12];
  std::memcpy(hdr, p, sizeof hdr);
  p += sizeof hdr;
  if (hdr[0] != kStateMagic) return fail(h, FDOCT_ERR_INVALID, "not a state blob");
  if (hdr[1] != kStateVersion) return fail(h, FDOCT_ERR_INVALID, "state blob of another format version");
  if (hdr[2] != h->W || hdr[3] != h->H || hdr[4] != h->N || hdr[5] != h->M)
    return fail(h, FDOCT_ERR_INVALID, "state blob does not match this handle's geometry (width, height, numfftpoints, multiplier)");
  auto rows_ok = [&](int r) { return r == 0 || r == 1 || r == h->H; };
  if (!rows_ok(hdr[6]) || !rows_ok(hdr[7]) || !rows_ok(hdr[8])) return fail(h, FDOCT_ERR_INVALID, "corrupt state blob: reference frame rows");
  if (hdr[9] != 0 && hdr[9] != 2 * h->N) return fail(h, FDOCT_ERR_INVALID, "corrupt state blob: phase length must be 0 or 2 x numfftpoints");
  if (hdr[10] != h->W) return fail(h, FDOCT_ERR_INVALID, "corrupt state blob: window length must equal width");
  const size_t nyb = (size_t)hdr[6] * h->W, nyp = (size_t)hdr[7] * h->W, nyd = (size_t)hdr[8] * h->W;
  const size_t nwin = (size_t)hdr[10], nph = (size_t)hdr[9];
  const size_t need = kStateHeader + (nyb + nyp + nyd + nwin + (size_t)h->N) * 8 + (size_t)h->N * 4 + nph * 4;
  if (len < need) return fail(h, FDOCT_ERR_INVALID, "state blob truncated");
  auto get = [&](void* dst, size_t bytes) {
    if (bytes) std::memcpy(dst, p, bytes);
    p += bytes;
  };
  RefFrame yb, yp, yd;
  std::vector<double> win(nwin), frac(h->N);
  std::vector<int32_t> idx(h->N);
  std::vector<float> phase(nph);
  yb.v.resize(nyb); yb.rows = hdr[6]; get(yb.v.data(), nyb * 8);
  yp.v.resize(nyp); yp.rows = hdr[7]; get(yp.v.data(), nyp * 8);
  yd.v.resize(nyd); yd.rows = hdr[8]; get(yd.v.data(), nyd * 8);
  get(win.data(), nwin * 8);
  get(frac.data(), (size_t)h->N * 8);
  get(idx.data(), (size_t)h->N * 4);
  get(phase.data(), nph * 4);
  for (int32_t v : idx)
    if (v < 0 || v >= h->W * h->M)  // the kernels index LDS with these
      return fail(h, FDOCT_ERR_INVALID, "corrupt state blob: nearestkindex entry outside the row");
  // the complex path must have a kernel at this size before anything is committed (as fdoct_set_dispersion_phase checks); the
  // new plan leaves every device table to be rebuilt
  PlanInputs in = plan_inputs(h);
  in.phase = !phase.empty();
  if (int rc = adopt_plan(h, in)) return rc;
  h->phase.swap(phase);
  h->yb = std::move(yb);
  h->yp = std::move(yp);
  h->yd = std::move(yd);
  h->win.swap(win);
  h->frac.swap(frac);
  h->idx.swap(idx);
  h->custom_win = (hdr[11] & 1) != 0;
  h->custom_table = (hdr[11] & 2) != 0;
  return FDOCT_OK;
} FDOCT_CATCH(h)

}  // extern "C"
