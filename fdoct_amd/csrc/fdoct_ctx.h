// fdoct_ctx.h -- what the translation units of the C-ABI layer share: the handle (fdoct_ctx), the error / device-scope /
// device-memory helpers, and the declarations of
//   fdoct_state.cpp   the handle's plan (fdoct_plan.h) and everything a handle uploads to its device (tables, planes, twiddles)
//   fdoct_route.cpp   the dispatch: choose_route (which carries out fdoct_route_value.h's route value), the passes in front of the
//                     chain, one launcher per kernel family, enqueue
//   fdoct_route_value.cpp the route of a call as a value, decided before anything is enqueued (make_route; plain C++ like the planner)
//   fdoct_big_host.cpp the long-row path's host side: the plans and tables of its transforms, their grouped launches, run_big
//   fdoct_capi.cpp    the extern "C" entry points of include/fdoct.h
//   fdoct_hostcall.h  what fdoct_process* decide on the host before anything is enqueued, as a value (make_host_call)
//   fdoct_pipeline.cpp fdoct_process's three-stream pipeline for host buffers on both sides, and its copy threads
//   fdoct_roi.cpp     those of include/fdoct_roi.h (the B-scan readouts)
//   fdoct_capture.cpp those of include/fdoct_capture.h (reference frames captured from camera frames)
//   fdoct_lowpass.cpp those of include/fdoct_lowpass.h (BscanDark's lpfilter, the capture's options)
//   fdoct_bscanbin.cpp those of include/fdoct_bscanbin.h (spinjnt's output binning between the linear B-scan and its dB)
//   fdoct_colour.cpp  those of include/fdoct_colour.h (the webcam's interleaved B,G,R frames: channelnum)
//   fdoct_manualavg.cpp those of include/fdoct_manualavg.h (manual averaging of B-scans: manualaccum and its counter)
//   fdoct_saveframes.cpp those of include/fdoct_saveframes.h (per-frame saves while averaging; the raw-magnitudes switch)
//   fdoct_calibrate.cpp those of include/fdoct_calibrate.h (BscanDark's calibration: device-side normalisations, held captures, composition)
//   fdoct_complex.cpp that of include/fdoct_complex.h (the complex A-scan: the chain through fdoct_route.cpp's enqueue_complex, the D x H layout)
//   fdoct_doppler.cpp those of include/fdoct_doppler.h (phase-resolved Doppler from complex A-scans: the stage alone, and behind enqueue_complex)
//   fdoct_dispersion.cpp those of include/fdoct_dispersion.h (the dispersion search over (a2, a3): the stage alone, and behind enqueue_complex)
//   fdoct_vibro.cpp   those of include/fdoct_vibro.h (vibrometry from the phase over time: the stage alone, and behind enqueue_complex)
//   fdoct_ssada.cpp   those of include/fdoct_ssada.h (split-spectrum amplitude decorrelation: the stage alone, and behind enqueue_complex)
//   fdoct_enface.cpp  those of include/fdoct_enface.h (en-face projection of a volume over depth slabs: the stage alone, and behind enqueue)
//   fdoct_stage.h     the staging plan of host-memory arguments: the side entry points', fdoct_process's single shot (stage_reserve / stage_upload / stage_finish, below, commit it)
// (round 5: one 2900-line file until then; the seams are DESIGN.md 3.5's).  Internal: nothing outside fdoct_amd/csrc includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/fdoct.h"
#include "fdoct_big.h"
#include "fdoct_host.h"
#include "fdoct_kernels.h"
#include "fdoct_launch.h"
#include "fdoct_route_value.h"
#include "fdoct_hostcall.h"
#include "fdoct_stage.h"
#include "fdoct_wave.h"
#include "fdoct_jit.h"
#include "fdoct_hostcopy.h"

using namespace fdoct;

namespace fdoct_impl {

inline const double kPi = 3.141592653589793;  // BscanFFT.cpp:609
inline thread_local std::string g_create_error;  // fdoct_create has no handle to report through

struct RefFrame {  // a caller-supplied reference frame (background / pi / dark), as doubles
  std::vector<double> v;
  int rows = 0;  // 0 = unset, 1 = one spectrum for all rows, H = full frame
};

inline int fail(fdoct_ctx* h, int code, const std::string& msg);
inline void drain(fdoct_ctx* h);

// Memory a handle owns: device memory (hipMalloc) or, Pinned, page-locked host memory (hipHostMalloc with the given flags).
// Freed when the buffer dies; reads as the T* it holds, so that launch code fills its argument blocks from it directly.
// Move-only (a BigPlan moves into the handle's map).
// Stream order: reserve and assign replace a buffer that calls still in flight may read or write, so they drain the handle's streams
// before they let go of it (retire) -- the wait hipFree happens to make, stated here so that it stays when the free does not.
template <typename T, bool Pinned>
class Buffer {
 public:
  Buffer() = default;
  explicit Buffer(unsigned flags) : flags_(flags) {}
  Buffer(Buffer&& o) noexcept : p_(o.p_), bytes_(o.bytes_), flags_(o.flags_) { o.p_ = nullptr, o.bytes_ = 0; }
  ~Buffer() { release(); }
  operator T*() const { return p_; }

  void release() {
    if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr;
    bytes_ = 0;
  }
  void swap(Buffer& o) noexcept { std::swap(p_, o.p_), std::swap(bytes_, o.bytes_), std::swap(flags_, o.flags_); }
  // at least `bytes`, grown only (the old contents are not kept)
  int reserve(fdoct_ctx* h, size_t bytes) {
    if (bytes_ >= bytes && p_) return FDOCT_OK;
    retire(h);
    void* q = nullptr;
    const hipError_t e = Pinned ? hipHostMalloc(&q, bytes, flags_) : hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(h, FDOCT_ERR_NOMEM, std::string(Pinned ? "hipHostMalloc: " : "hipMalloc: ") + hipGetErrorString(e));
    p_ = static_cast<T*>(q);
    bytes_ = bytes;
    return FDOCT_OK;
  }
  // exactly `count` elements; 0 releases the buffer
  // (drained: the caller has waited for the handle's streams itself -- a table rebuild does so once for all its tables)
  int assign(fdoct_ctx* h, size_t count, bool drained = false) {
    if (drained)
      release();
    else
      retire(h);
    return count ? reserve(h, count * sizeof(T)) : FDOCT_OK;
  }

 private:
  // release() once nothing the handle has enqueued can still use the memory
  void retire(fdoct_ctx* h) {
    if (p_ && h) drain(h);
    release();
  }
  T* p_ = nullptr;
  size_t bytes_ = 0;
  unsigned flags_ = hipHostMallocDefault;
};
template <typename T> using DevBuf = Buffer<T, false>;
template <typename T> using PinnedBuf = Buffer<T, true>;

}  // namespace fdoct_impl
using fdoct_impl::DevBuf;
using fdoct_impl::PinnedBuf;
using fdoct_impl::RefFrame;

struct fdoct_ctx {
  fdoct_config cfg{};
  int W = 0, H = 0, N = 0, D = 0, M = 1, A = 1;
  int device = 0, num_cu = 256;
  hipStream_t own_stream = nullptr, stream = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  std::string err;

  // host state
  std::vector<double> win;
  std::vector<int32_t> idx;
  std::vector<double> frac;
  RefFrame yb, yp, yd;
  std::vector<float> phase;  // N (cos,sin) pairs or empty
  bool custom_win = false, custom_table = false, force_general = false, staged = false, bandpass = false;
  int block_override = 0, grid_override = 0, plan_override = -1;  // plan_override == -2: force the generic path

  Plan plan;               // made for plan_inputs(this); replaced only by a plan made in full (adopt_plan)
  unsigned tables_ok = 0;  // TABLES_* whose device tables match the host state (invalidate clears them all)

  DevBuf<unsigned> d_gen_tickets;   // kGenTickets row counters of generic_kernel launches, used round-robin (one per launch in flight)
  unsigned gen_ticket_seq = 0;
  struct GenericDftTables {
    DevBuf<float2> tw, chirp, bhat;
  };
  GenericDftTables d_gzf, d_gzi;  // of plan.gen.gzf / gzi: the zero-pad stage at full length inside generic_kernel
  DevBuf<float2> d_blu_chirp, d_blu_bhat, d_twg_blu;

  // device state
  DevBuf<float> d_ib, d_ib2d, d_ib2d_f, d_yp, d_yd, d_yp_lo, d_yd_lo, d_win, d_g;
  DevBuf<float> d_il, d_il2d, d_il2d_f, d_il_p;  // d_il_p: d_il in the order of the fused kernels' LDS planes  // low words of the reciprocal background, laid out like d_ib / d_ib2d / d_ib2d_f
  DevBuf<uint32_t> d_il16, d_il16_2d;  // the second word as the fast path reads it: il / ib * 2^38 as half-float pairs (fdoct_fused_rules.h: fused_il_half)
  // fdoct_set_precise_division.  ON by default (round 5): main:1132 divides in double, and one f32 reciprocal leaves a fixed
  // pattern of 6e-8 of the DC level -- 8 x the tolerance on fringes of 1e-3 of it.  Off (or FDOCT_PRECISE_DIVISION=0) is the
  // opt-out for callers who know their fringes exceed ~1 % of the DC level.
  bool precise_div = true;
  // BscanFFTsim.cpp with averages > 1 (sim:936-947): every frame's magnitudes are COPIED over the last one's (the accumulate
  // is commented out) and what is emitted, undivided, is the last copy -- frame averages - 1 of every group.  The chain then
  // runs with A = 1 on those frames only (fdoct_hostcall.h: read where they lie, or gathered into ws_sim); sim_group is the group
  // length the caller counts in.
  int sim_group = 1;
  DevBuf<unsigned char> ws_sim;
  DevBuf<uint32_t> d_gidx;
  DevBuf<float2> d_tw, d_utw, d_phase, d_minmax;
  // generic path
  DevBuf<float> d_win_g, d_win_lo_g, d_g_g;
  DevBuf<int32_t> d_idx_g;
  // wave-per-row kernels (fdoct_wave.hip)
  DevBuf<uint32_t> d_wave_gidx;
  DevBuf<float2> d_wave_tw;
  DevBuf<float2> d_twg_n, d_twg_nh, d_twg_w, d_twg_mw, d_twg_wh, d_twg_mwh;
  // long-row path (fdoct_big.hip): rows in HBM, one DFT plan per length
  using BigGroupPlan = fdoct::BigGroupPlan;  // one launch: a group of the transform's passes with the data in LDS (fdoct_big_plan.h)
  struct BigPlan {
    std::vector<int> rad;      // Stockham radices of the length itself, or (Bluestein) of mb: the one-launch-per-pass form
    std::vector<BigGroupPlan> groups;  // the same transform as a few launches of several passes each (empty: not available)
    int mb = 0;                // > 0: the length has a prime factor above 5 and runs as Bluestein around two mb-point DFTs
    DevBuf<float2> d_tw, d_chirp, d_bhat;  // exp(+2 pi i j / (mb ? mb : n)); e^(+i pi m^2/n); DFT(conj chirp)/mb
  };
  bool use_big = false;
  std::map<int, BigPlan> big_plans;
  DevBuf<float> ws_big_y;
  DevBuf<float2> ws_big_a, ws_big_b;
  // workspaces
  DevBuf<float> ws_f32, ws_f32_lo;   // f64 frames as two f32 planes (launch_f64_split)
  DevBuf<float> ws_mov_lo;           // ... and the moving average of the low plane
  DevBuf<float> ws_tr;
  DevBuf<float2> ws_ylin;
  long long ylin_rows = 0;  // A-scans the last staged run left in ws_ylin (0: none)
  DevBuf<float> ws_mov;
  DevBuf<unsigned char> ws_front, ws_med;
  DevBuf<unsigned char> stage_in, stage_out;  // host-memory arguments on their way up and down (stage_reserve): fdoct_process's single shot, the side entry points
  int fe_median = 0, fe_binx = 1, fe_biny = 1;
  // host-pointer pipeline (fdoct_process with host buffers): copy-in / kernels / copy-out on three streams
  hipStream_t s_in = nullptr, s_out = nullptr;
  hipEvent_t pe_in[2] = {nullptr, nullptr}, pe_k[2] = {nullptr, nullptr}, pe_out[2] = {nullptr, nullptr};
  DevBuf<unsigned char> pl_in[2];
  DevBuf<float> pl_mag[2], pl_db[2];
  // the same pipeline fed from / drained to PAGEABLE caller memory (fdoct_hostcopy.h): pinned staging slots the handle owns
  // and the threads that move a chunk between them and the caller's buffers
  PinnedBuf<unsigned char> pin_in[2];
  PinnedBuf<float> pin_mag[2], pin_db[2];
  std::unique_ptr<fdoct_impl::HostCopyPool> copy_pool;
  int host_staging = -1;  // fdoct_set_host_staging: -1 = the library decides per buffer (pageable: staged), 0 = never, > 0 = that many copy threads
  unsigned char lut[768];
  bool lut_dirty = true;
  DevBuf<unsigned char> d_lut;
  DevBuf<double> d_disp_part;
  // B-scan readouts (fdoct_roi.cpp): measurement state, not set-up state, so neither fdoct_export_state nor
  // fdoct_clone_to_device carries it
  struct PeakHoldRoi {
    int x = 0, y = 0, w = 0, h = 0, ascanat = 0;  // x, w: A-scans; y, h: depths
    bool set = false;
  };
  PeakHoldRoi roi;
  DevBuf<uint32_t> d_hold_cols;    // 4 slots x roi.w column holds, as roi_encode words (fdoct_roi_kernels.h)
  DevBuf<uint32_t> d_hold_scalar;  // 4 scalar holds of A-scan roi.ascanat, likewise
  long long hold_count[4] = {0, 0, 0, 0};
  // reference-frame capture (fdoct_capture.cpp): the front end goes through ws_med / ws_front
  DevBuf<double> ws_cap_acc;       // the H x W sums on their way to the host
  DevBuf<double> ws_cap_mm;        // per-frame min / max: the per-block partials
  // fdoct_set_capture_options (fdoct_lowpass.cpp): BscanDark.ini's lowpassfilter and the ini's saveinterferograms.  Run-time
  // settings like the front end's: fdoct_clone_to_device carries them, the state blob does not.
  int cap_lowpass = 0, cap_raw = 0;
  DevBuf<double> ws_lp_bins;       // rows too long for LDS: their bins (LowpassShape::ws_doubles)
  // spinjnt's output binning (fdoct_bscanbin.cpp)
  DevBuf<double> d_bin_taps;       // the cubic's phases for bin_taps_upx / bin_taps_upy (fdoct_bscanbin_kernels.h), uploaded when they change
  int bin_taps_upx = 0, bin_taps_upy = 0;
  // fdoct_set_colour_input (fdoct_colour.cpp): BscanFFTwebcam.ini's channelnum.  -1: mono frames; 0 / 1 / 2: 8-bit frames are
  // interleaved B,G,R and that channel is taken; 3: their scaled sum, a frame of doubles.  A run-time setting like the front
  // end's: fdoct_clone_to_device carries it, the state blob does not.
  int colour = -1;
  DevBuf<unsigned char> ws_col;    // the full-resolution channel on its way to the median (run_colour)
  DevBuf<double> ws_col_sum;       // the (binned) sum frames
  // manual averaging (fdoct_manualavg.cpp): measurement state like the peak holds, so neither fdoct_export_state nor
  // fdoct_clone_to_device carries it
  DevBuf<double> d_mavg;           // manualaccum (BscanFFT.cpp:933): mavg_count running sums
  size_t mavg_count = 0;
  int mavg_m = 0, mavg_mode = 0, mavg_accumulated = 0;  // manualaverages (0: no accumulator), fdoct_manualavg_mode, manualaccumcount
  // per-frame saves (fdoct_saveframes.cpp).  fdoct_set_raw_magnitudes: the chain's kernels get 0 for their epsilon
  // (kernel_eps) and write no dB.  A run-time setting like `averages`: fdoct_clone_to_device carries it, the state blob does not.
  bool raw_mag = false;
  DevBuf<double> d_sf_part;        // partial (min, max) pairs of the pictures' dB values, per image (fdoct_saveframes_kernels.h)
  // BscanDark's calibration (fdoct_calibrate.cpp): the dark / reference / sample captures held on the device.  Measurement state
  // like the peak holds, so neither fdoct_export_state nor fdoct_clone_to_device carries it
  DevBuf<double> d_cal[3];         // H x W doubles each, indexed by fdoct_cal_slot
  bool cal_held[3] = {false, false, false};
  DevBuf<double> ws_cal_next;      // the frame a capture is writing: swapped with its slot when the capture has succeeded
  DevBuf<double> ws_cal_mm;        // min / max partials and the (scale, shift) pairs made from them (MinMaxShape::ws_doubles)
  // the complex A-scan (fdoct_complex.cpp): the chain's row-major pairs on their way to the D x H layout
  DevBuf<float2> ws_cx;
  // phase-resolved Doppler (fdoct_doppler.cpp): fdoct_process_doppler's pairs go through ws_cx; the bulk-motion phasors, one per pair row
  DevBuf<float2> ws_dop_bulk;
  // the dispersion search (fdoct_dispersion.cpp): fdoct_process_dispersion_search's pairs go through ws_cx; the transform's twiddles
  // and the two phasor tables (DispersionArgs::tab).  The outputs, the winner included, go through the staging plan
  DevBuf<float2> ws_disp_tab;
  // vibrometry (fdoct_vibro.cpp): fdoct_process_vibro's pairs go through ws_cx; the reference phasors, one per frame and A-scan; the
  // chunk partials; the lock-in's tables and their sums (VibroArgs::tab, cst, head, glob).  The outputs go through the staging plan
  DevBuf<float2> ws_vib_ref;
  DevBuf<double> ws_vib_part;
  DevBuf<double2> ws_vib_tab;
  // angiography (fdoct_angio.cpp): fdoct_process_angio's pairs go through ws_cx; the bulk-motion phasors, one per group, pair and
  // A-scan.  State like ws_dop_bulk: neither fdoct_clone_to_device nor the state blob carries it
  DevBuf<float2> ws_ang_bulk;
  // coherent averaging (fdoct_cxavg.cpp): fdoct_process_cxavg's pairs go through ws_cx; with align 2 the phasors, one per group and
  // repeat, and behind them the per-row sums they are made from.  State like ws_ang_bulk
  DevBuf<float2> ws_cxa;
  // split-spectrum decorrelation (fdoct_ssada.cpp): fdoct_process_ssada's pairs go through ws_cx; one pass's band pairs with the
  // per-band decorrelation and power behind them, and the transform's twiddles with the bands' table.  State like ws_ang_bulk
  DevBuf<unsigned char> ws_ssa, ws_ssa_tab;
  // en-face projection (fdoct_enface.cpp): the raw surfaces, one per position and A-scan, between its two kernels; the row-major
  // volume fdoct_process_enface's chain writes.  State like ws_ang_bulk
  DevBuf<int32_t> ws_enf_surf;
  DevBuf<float> ws_enf_vol;

  fdoct_timing timing{};
  bool timing_pending = false, timing_staged = false;
  bool async_timing = false, record_now = false;  // event records cost stream time: async calls opt in
  bool rec_first = true, rec_last = true;         // chunked calls: the first chunk records the start events, the last one the end events
  // see FusedArgs::tr_fault: one word of pinned, device-visible HOST memory, so that any entry point can look at it without a
  // copy or a synchronisation of its own (coherent: fdoct_route.cpp, launch_family_fused)
  PinnedBuf<unsigned> d_tro_fault{hipHostMallocCoherent | hipHostMallocMapped};
  bool tro_used = false;                          // a TRO launch has run on this handle
  bool tro_enabled = true;                        // FDOCT_NO_TRO=1 (tuning / tests): always the two-pass path
  size_t tr_chunk_bytes = (size_t)2 << 30;        // transposed layout, two-pass path: row-major intermediate per chunk (bounds the workspace)
  bool jit = true;                                // fdoct_set_jit / FDOCT_JIT=0: compile the wave-per-row kernel for shapes off the built-in list
  std::string jit_note;                           // why the last run-time compile was refused (the call itself fell back and succeeded)
  int last_kernel = FDOCT_KERNEL_NONE;            // fdoct_last_kernel
  hipEvent_t ev_order = nullptr;                  // fdoct_set_stream: recorded on the stream the handle leaves, waited for on the one it moves to
};

namespace fdoct_impl {

inline int fail(fdoct_ctx* h, int code, const std::string& msg) {
  if (h)
    h->err = msg;
  else
    g_create_error = msg;
  return code;
}

#define HIP_TRY(h, expr)                                                                       \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return fail(h, FDOCT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

// Every entry point works on the handle's device and leaves the calling thread's current device as it found it: a host
// that drives other GPUs through HIP (or torch) on the same thread is not re-pointed behind its back.
struct DeviceScope {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceScope(int device) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != device) {
      err = hipSetDevice(device);
      switched = (err == hipSuccess);
    }
  }
  ~DeviceScope() {
    if (switched) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};
#define DEVICE_SCOPE(h)                                                                                     \
  DeviceScope device_scope_((h)->device);                                                                   \
  if (device_scope_.err != hipSuccess)                                                                      \
  return fail(h, FDOCT_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(device_scope_.err))

// A device table built from host state.  Stream order: a rebuild waits for the handle's streams ONCE, at its head, before any of its
// tables goes (fdoct_state.cpp: upload_shared, ensure_wave_tables), so a call enqueued before the setter that caused the rebuild has
// finished with them; the tables of a new long-row plan go into buffers nothing has used.  The copy is synchronous, so the call
// that follows finds the new table whichever stream it runs on.
template <typename T>
int upload(fdoct_ctx* h, DevBuf<T>& d, const std::vector<T>& v) {
  if (int rc = d.assign(h, v.size(), /*drained=*/true)) return rc;
  if (!v.empty()) HIP_TRY(h, hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return FDOCT_OK;
}

// The commit of a staging plan (fdoct_stage.h).  stage_reserve grows the handle's two staging buffers and sets the items' device
// pointers; every other reservation and refusal of the call follows it, then stage_upload enqueues the host-to-device copies on
// h->stream (stage_begin: both at once), and stage_finish the device-to-host copies and the synchronise host memory asks for.
inline int stage_reserve(fdoct_ctx* h, StagePlan* p) {
  if (p->rc) return fail(h, p->rc, "staging: the arguments' sizes do not fit size_t");
  if (int rc = p->in_bytes ? h->stage_in.reserve(h, p->in_bytes) : FDOCT_OK) return rc;
  if (int rc = p->out_bytes ? h->stage_out.reserve(h, p->out_bytes) : FDOCT_OK) return rc;
  for (StageItem& it : p->item) it.dev = !it.staged ? it.ptr : (it.output && !it.on_input ? h->stage_out : h->stage_in) + it.offset;
  return FDOCT_OK;
}
inline int stage_copy(fdoct_ctx* h, const StagePlan& p, bool down) {  // the staged inputs up, or the staged outputs down
  for (const StageItem& it : p.item) {
    if (!it.staged || !it.ptr || it.output != down) continue;
    if (!it.dev) return fail(h, FDOCT_ERR_STATE, "staging: a copy before reserve");
    void *const dst = down ? it.ptr : it.dev, *const src = down ? it.dev : it.ptr;
    const size_t dp = down ? it.pitch : it.dev_pitch, sp = down ? it.dev_pitch : it.pitch;
    const hipMemcpyKind kind = down ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
    HIP_TRY(h, it.rows == 1 ? hipMemcpyAsync(dst, src, it.row, kind, h->stream) : hipMemcpy2DAsync(dst, dp, src, sp, it.row, it.rows, kind, h->stream));
  }
  return FDOCT_OK;
}
inline int stage_upload(fdoct_ctx* h, const StagePlan& p) { return stage_copy(h, p, false); }
inline int stage_begin(fdoct_ctx* h, StagePlan* p) { const int rc = stage_reserve(h, p); return rc ? rc : stage_upload(h, *p); }
inline int stage_finish(fdoct_ctx* h, const StagePlan& p) {
  if (int rc = stage_copy(h, p, true)) return rc;
  if (p.sync) HIP_TRY(h, hipStreamSynchronize(h->stream));
  return FDOCT_OK;
}
// The refusal of fdoct_stage.h's overlaps(), in the words of the side entry points; `in_name` is what the message calls the input.
inline int refuse_overlaps(fdoct_ctx* h, const std::string& fn, const char* in_name, const void* in, size_t in_bytes, const void* const* out,
                           const size_t* bytes, int n) {
  switch (overlaps(in, in_bytes, out, bytes, n)) {
    case OVERLAP_INPUT: return fail(h, FDOCT_ERR_INVALID, fn + ": " + in_name + " and output buffers overlap");
    case OVERLAP_OUTPUTS: return fail(h, FDOCT_ERR_INVALID, fn + ": the outputs overlap");
    default: return FDOCT_OK;
  }
}

// COLORMAP_JET as OpenCV builds it (fdoct_host.cpp::build_opencv_jet): dark blue (128,0,0 in B,G,R) at 0 through cyan and
// yellow to dark red (0,0,128) at 255.
inline void builtin_jet(unsigned char* bgr) { build_opencv_jet(bgr); }

// ---- fdoct_state.cpp ------------------------------------------------------------------------------------------------------
// Each family's device tables (TABLES_*, fdoct_route_value.h), built by its ensure_*_tables when they do not match the host state.
inline void invalidate(fdoct_ctx* h) { h->tables_ok = 0; }

// Waits for everything the handle has enqueued: nothing is left in flight that still points at the caller's buffers or the
// chunk slots.
inline void drain(fdoct_ctx* h) {
  if (h->s_in) (void)hipStreamSynchronize(h->s_in);
  (void)hipStreamSynchronize(h->stream);
  if (h->s_out) (void)hipStreamSynchronize(h->s_out);
}

// The one handler of every entry point (include/fdoct.h, include/fdoct_roi.h: nothing throws across the boundary).  Out of
// host memory is FDOCT_ERR_NOMEM, any other exception FDOCT_ERR_DEVICE, and the text goes where fdoct_last_error finds it.  A
// handle's device state is rebuilt by its next call (an exception may have cut an upload short) and its streams are drained.
inline int caught(fdoct_ctx* h) noexcept {
  int code = FDOCT_ERR_DEVICE;
  const char* what = "unknown exception";
  try {
    throw;
  } catch (const std::bad_alloc&) {
    code = FDOCT_ERR_NOMEM;
    what = "out of host memory";
  } catch (const std::exception& e) {
    what = e.what();
  } catch (...) {
  }
  std::string& err = h ? h->err : g_create_error;
  try {
    err = what;
  } catch (...) {
    err.clear();
  }
  if (h) {
    invalidate(h);
    drain(h);
  }
  return code;
}
#define FDOCT_CATCH(h) catch (...) { return caught(h); }
#define FDOCT_CATCH_RETURN(h, value) catch (...) { (void)caught(h); return value; }
#define FDOCT_CATCH_VOID(h) catch (...) { (void)caught(h); }

int copy_ref_frame(fdoct_ctx* h, RefFrame& dst, const void* data, fdoct_dtype dtype, int rows, size_t pitch);
PlanInputs plan_inputs(const fdoct_ctx* h);
int adopt_plan(fdoct_ctx* h, const PlanInputs& in);
void reciprocal_words(const std::vector<double>& yb, std::vector<float>& ib, std::vector<float>& il);
struct PlaneScales { double yb, yp, yd; };
PlaneScales plane_scales(const fdoct_ctx* h);
std::vector<double> scaled_copy(const std::vector<double>& v, double s);
void build_bluestein_tables(int n, int Mb, std::vector<float2>& chirp, std::vector<float2>& bhat);
int ensure_fused_tables(fdoct_ctx* h);
int ensure_generic_tables(fdoct_ctx* h);  // (fails where the plan's generic path does: GenericPlan::rc)
int ensure_wave_tables(fdoct_ctx* h);

// ---- fdoct_route.cpp ------------------------------------------------------------------------------------------------------
// ---- dispatch ----------------------------------------------------------------------------------------------------------
// Everything a call decides before it enqueues anything: which passes run in front of the chain, which kernel family takes it
// and that family's launch -- instantiation, block, LDS, grid.  A function of the handle's state and of the call's geometry only
// (pointers enter through their alignment), so that fdoct_prepare makes the same decisions -- pays for a run-time compile, meets
// the same refusals -- without frames.  The launchers fill argument blocks from handle and route and launch; they decide nothing.
// The decision is a value made without HIP (make_route, fdoct_route_value.h); a Route is that value with what choose_route adds.
struct Route : RouteDecision {
  hipFunction_t jit_fn = nullptr;   // FDOCT_KERNEL_WAVE_JIT: the kernel compiled for this handle
};

// Quantities of one call that every family's launch needs.
struct Call {
  const void* kframes = nullptr;    // what the chain's kernel reads (the caller's frames, or the last pre-pass's output)
  const float* kframes_lo = nullptr;  // f64 frames: the low words of kframes (same pitch), else null
  int nframes = 0, G = 0;
  long long in_rows = 0, out_rows = 0;
  size_t es = 0;                    // bytes per sample of the CALLER's frames (the algorithmic-bytes figure)
  float *k_mag = nullptr, *k_db = nullptr;          // where the chain's kernel writes (the caller's arrays, or the transpose pass's input)
  float2* k_cx = nullptr;           // the complex call (enqueue_complex): (re, im) pairs go here and k_mag / k_db stay null
  float *d_out_bscan = nullptr, *d_out_db = nullptr;
  hipStream_t st = nullptr;
};

// Bytes per pixel of the frames a call takes: the sample's size, or 3 for the 8-bit frames of a colour handle.
inline size_t frame_pixel_bytes(const fdoct_ctx* h, int dtype) { return h->colour >= 0 && dtype == FDOCT_U8 ? 3 : dtype_size(dtype); }
// What a colour stage can do, checked before anything is enqueued (`who` prefixes the message): 8-bit frames only, no median in
// front of the sum (cv::medianBlur rejects CV_64F: there is no reference behaviour to match).
int colour_check(fdoct_ctx* h, const char* who, int channelnum, fdoct_dtype dtype, int mediann);
// The colour stage on device-resident interleaved frames (fdoct_colour.hip), with the median / binning behind it: leaves packed,
// 16-byte-pitched bytes (channelnum 0-2) or doubles (3) in a library workspace, *out / *out_pitch.  Enqueues only.  With null
// frames, both: their checks and workspaces alone, nothing enqueued (a call that uploads host frames does that first).
int run_colour(fdoct_ctx* h, const void* d_bgr, int nframes, int raw_w, int raw_h, size_t pitch, int channelnum, int mediann, int binx,
               int biny, void** out, size_t* out_pitch);
int run_frontend(fdoct_ctx* h, const void* d_raw, int kdt, int nframes, int raw_w, int raw_h, size_t raw_pitch, int mediann,
                 int binx, int biny, void** out, size_t* out_pitch);
float chain_eps(const fdoct_ctx* h);  // the epsilon under the chain's log (sim:949 / main:1222)
float kernel_eps(const fdoct_ctx* h);  // what the chain's kernels are handed for it: chain_eps, or 0 with fdoct_set_raw_magnitudes
// The inputs of make_route: the handle's part, and a row-major call of `nframes` frames without outputs; the caller adds the rest.
RouteInputs route_inputs(const fdoct_ctx* h, fdoct_dtype dtype, uintptr_t frames_addr, size_t pitch_bytes, int nframes);
int choose_route(fdoct_ctx* h, const RouteInputs& in, Route* r);
// What refuses a call without a route and without its frames: no background, no output, a bad dtype, a pitch below a row.  First in
// enqueue_one; fdoct_process* make it ahead of their own copies.
int check_call(fdoct_ctx* h, fdoct_dtype dtype, size_t pitch_bytes, const float* out_bscan, const float* out_db);
int enqueue(fdoct_ctx* h, const void* d_frames, fdoct_dtype dtype, int nframes, size_t pitch_bytes,
            float* d_out_bscan, float* d_out_db, fdoct_layout layout);
// The complex A-scan of device-resident frames, row-major [nframes H D] (re, im) pairs (include/fdoct_complex.h: the add-on library's
// entry point calls it).  d_out null: the checks and the route only -- nothing is enqueued.
int enqueue_complex(fdoct_ctx* h, const void* d_frames, fdoct_dtype dtype, int nframes, size_t pitch_bytes, float2* d_out);

// ---- fdoct_big_host.cpp ---------------------------------------------------------------------------------------------------
// The whole chain for device-resident frames on the long-row path (fdoct_big.hip), chunk by chunk of whole averaging groups.
int run_big(fdoct_ctx* h, const void* kframes, const float* kframes_lo, int kdt, size_t kpitch, int nframes, bool need_minmax, float* k_mag, float* k_db,
            hipStream_t st);

// ---- fdoct_pipeline.cpp ---------------------------------------------------------------------------------------------------
bool host_pointer_is_pinned(const void* p);
int copy_thread_count(const fdoct_ctx* h);  // 0: pageable buffers are not staged
// HostPath::Pipelined carried out on `batch`, the caller's frames pointer; synchronous.  Drains the handle if it fails.
int process_pipelined(fdoct_ctx* h, const HostCall& call, const void* batch, fdoct_dtype dtype, float* out_bscan, float* out_db,
                      fdoct_layout layout);

// ---- fdoct_lowpass.cpp ----------------------------------------------------------------------------------------------------
// Enqueues lpfilter (BscanDark.cpp:119-167) on device rows of W doubles (d_in == d_out: in place) and reserves the workspace a
// long row needs -- with d_in null that alone, like run_frontend.  The arguments are the caller's to check.
int enqueue_lowpass(fdoct_ctx* h, const double* d_in, size_t in_pitch, double* d_out, size_t out_pitch, int rows, int W);

}  // namespace fdoct_impl
