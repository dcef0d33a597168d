// fdoct_route.cpp -- the dispatch of a call: choose_route decides everything before anything is enqueued -- the
// passes in front of the chain, the kernel family and its launch (the fused family's from fdoct_launch.h) --, the passes run, one
// launcher per kernel family fills its argument block from handle and route, finish_launch is the one epilogue; plus the front end.
// The decision itself is a value (make_route, fdoct_route_value.h): choose_route builds its inputs and carries it out.  The long-row
// path's host side is fdoct_big_host.cpp.  Part of the C-ABI layer (fdoct_ctx.h).
#include "fdoct_ctx.h"
#include "fdoct_colour_kernels.h"

namespace fdoct_impl {

// medianBlur + INTER_AREA binning of device-resident raw frames into a packed, 16-byte-pitched buffer.
// Returns the binned frames in *out / *out_pitch (library workspace).  d_raw null: the checks and the workspaces only.
int run_frontend(fdoct_ctx* h, const void* d_raw, int kdt, int nframes, int raw_w, int raw_h, size_t raw_pitch, int mediann,
                 int binx, int biny, void** out, size_t* out_pitch) {
  if (kdt != FDOCT_K_U8 && kdt != FDOCT_K_U16) return fail(h, FDOCT_ERR_UNSUPPORTED, "the front end takes 8- or 16-bit camera frames");
  if (binx < 1 || biny < 1 || raw_w % binx || raw_h % biny) return fail(h, FDOCT_ERR_INVALID, "frame size must be a multiple of the bin factors");
  if (mediann != 0 && mediann != 3 && mediann != 5 && mediann != 7) return fail(h, FDOCT_ERR_INVALID, "mediann must be 0, 3, 5 or 7");
  // cv::medianBlur takes ksize 3 or 5 only for CV_16U (main:955 would throw): there is no reference behaviour to match
  if (mediann == 7 && kdt == FDOCT_K_U16) return fail(h, FDOCT_ERR_INVALID, "a 7x7 median exists for 8-bit frames only (cv::medianBlur)");
  const size_t es = kdt == FDOCT_K_U8 ? 1 : 2;
  int rc;
  hipStream_t st = h->stream;
  const void* src = d_raw;
  size_t src_pitch = raw_pitch;
  const size_t mp = frontend_pitch(raw_w, es);
  const int ow = raw_w / binx, oh = raw_h / biny;
  const size_t op = frontend_pitch(ow, es);
  if (mediann > 0 && (rc = h->ws_med.reserve(h, mp * (size_t)raw_h * nframes))) return rc;
  if ((rc = h->ws_front.reserve(h, op * (size_t)oh * nframes))) return rc;
  if (!d_raw) return FDOCT_OK;
  if (mediann > 0) {
    HIP_TRY(h, launch_median(src, (long long)src_pitch, h->ws_med, (long long)mp, kdt, raw_w, raw_h, mediann, nframes, st));
    src = h->ws_med;
    src_pitch = mp;
  }
  HIP_TRY(h, launch_bin(src, (long long)src_pitch, h->ws_front, (long long)op, kdt, ow, oh, binx, biny, nframes, st));
  *out = h->ws_front;
  *out_pitch = op;
  return FDOCT_OK;
}

int colour_check(fdoct_ctx* h, const char* who, int channelnum, fdoct_dtype dtype, int mediann) {
  std::string why;
  const int rc = colour_refusal(who, channelnum, dtype, mediann, &why);
  return rc ? fail(h, rc, why) : FDOCT_OK;
}

// webcam:1015-1038 and the block behind it.  Sum: one kernel, the binning in it.  Select without a median: likewise, into the
// front end's output buffer.  Select with a median: the full-resolution channel goes to ws_col and from there through the mono
// front end as it is (launch_median, launch_bin).  d_bgr null: the checks and the workspaces only, like run_frontend.
int run_colour(fdoct_ctx* h, const void* d_bgr, int nframes, int raw_w, int raw_h, size_t pitch, int channelnum, int mediann, int binx,
               int biny, void** out, size_t* out_pitch) {
  if (int rc = colour_check(h, "colour stage", channelnum, FDOCT_U8, mediann)) return rc;
  if (nframes < 1 || raw_w < 1 || raw_h < 1) return fail(h, FDOCT_ERR_INVALID, "colour stage: no frames");
  if (binx < 1 || biny < 1 || raw_w % binx || raw_h % biny) return fail(h, FDOCT_ERR_INVALID, "frame size must be a multiple of the bin factors");
  if (pitch < 3 * (size_t)raw_w) return fail(h, FDOCT_ERR_INVALID, "pitch smaller than a row of B,G,R pixels");
  const bool via_median = mediann > 0;
  ColourArgs a;
  a.bgr = static_cast<const unsigned char*>(d_bgr);
  a.pitch = (long long)pitch;
  a.channelnum = channelnum;
  a.binx = via_median ? 1 : binx;
  a.biny = via_median ? 1 : biny;
  a.ow = raw_w / a.binx;
  a.out_rows = (long long)nframes * (raw_h / a.biny);
  a.out_pitch = (long long)frontend_pitch(a.ow, channelnum == 3 ? 8 : 1);
  const size_t bytes = (size_t)a.out_pitch * (size_t)a.out_rows;
  int rc;
  if (channelnum == 3) {
    if ((rc = h->ws_col_sum.reserve(h, bytes))) return rc;
    a.out = h->ws_col_sum;
  } else {
    DevBuf<unsigned char>& ws = via_median ? h->ws_col : h->ws_front;
    if ((rc = ws.reserve(h, bytes))) return rc;
    a.out = ws;
  }
  if (via_median && (rc = run_frontend(h, nullptr, FDOCT_K_U8, nframes, raw_w, raw_h, 0, mediann, binx, biny, nullptr, nullptr))) return rc;
  if (!d_bgr) return FDOCT_OK;
  HIP_TRY(h, launch_colour(a, h->stream));
  if (via_median) return run_frontend(h, a.out, FDOCT_K_U8, nframes, raw_w, raw_h, (size_t)a.out_pitch, mediann, binx, biny, out, out_pitch);
  *out = a.out;
  *out_pitch = (size_t)a.out_pitch;
  return FDOCT_OK;
}

// What make_route reads: the handle's part, and a row-major call of `nframes` frames without outputs (fdoct_prepare: an aligned,
// packed set-up); the entry points add their outputs, layout and whether the call is the complex one.
RouteInputs route_inputs(const fdoct_ctx* h, fdoct_dtype dtype, uintptr_t frames_addr, size_t pitch_bytes, int nframes) {
  static const unsigned ring_cap = [] { const char* e = std::getenv("FDOCT_TRO_RING"); return e ? (unsigned)std::atoi(e) : 0u; }();  // measurement: at most this many slots
  RouteInputs in;
  in.W = h->W; in.H = h->H; in.N = h->N; in.D = h->D; in.M = h->M; in.A = h->A;
  in.plan = &h->plan;
  in.bg_rows = h->yb.rows; in.pi = h->yp.rows > 0; in.dark = h->yd.rows > 0;
  in.bandpass = h->bandpass; in.rowwisenormalize = h->cfg.rowwisenormalize != 0;
  in.normalize = (h->cfg.variant == FDOCT_VARIANT_SIM) || !h->cfg.donotnormalize;
  in.phase = !h->phase.empty(); in.movavgn = h->cfg.movavgn;
  in.fe_median = h->fe_median; in.fe_binx = h->fe_binx; in.fe_biny = h->fe_biny; in.colour = h->colour;
  in.jit = h->jit; in.staged = h->staged;
  in.plan_override = h->plan_override; in.block_override = h->block_override; in.grid_override = h->grid_override; in.num_cu = h->num_cu;
  in.precise_div = h->precise_div; in.force_general = h->force_general; in.tro_enabled = h->tro_enabled; in.ring_cap = ring_cap;
  in.dtype = dtype; in.frames_addr = frames_addr; in.pitch_bytes = pitch_bytes; in.nframes = nframes;
  return in;
}

// make_route's question to the run-time compiler, and what the compiler's last answer left: the kernel and the reason.
struct JitAsk {
  const fdoct_ctx* h;
  bool asked = false;
  hipFunction_t fn = nullptr;
  std::string why;
  static bool can_compile(void* p, int kdt, int wave_opt) {
    JitAsk& a = *static_cast<JitAsk*>(p);
    a.asked = true;
    a.fn = nullptr;
    return wave_jit_get(a.h->W, a.h->M, a.h->N, kdt, a.h->D, wave_opt, a.h->device, &a.fn, &a.why) == hipSuccess;
  }
};

// Decides the route of a call (make_route) and carries out what the decision asks of the handle: the device tables it names, and
// fdoct_jit_note -- the reason of the route's last compile attempt (empty after a successful one), or the decision's own note.  May
// compile (hipRTC) and rebuild device tables -- never launches.  Reads the handle's adopted plan and changes none of it.
int choose_route(fdoct_ctx* h, const RouteInputs& in, Route* r) {
  JitAsk jit{h};
  RouteDecision d;
  std::string why;
  if (int rc = route_precheck(in, &why)) return fail(h, rc, why);   // (no route: the note stays the last route's)
  int rc = make_route(in, JitAsk::can_compile, &jit, &d, &why);
  if (rc) fail(h, rc, why);
  if (!rc && (d.tables & TABLES_FUSED)) rc = ensure_fused_tables(h);
  if (!rc && (d.tables & (TABLES_GENERIC | TABLES_WAVE))) rc = (d.tables & TABLES_WAVE) ? ensure_wave_tables(h) : ensure_generic_tables(h);
  if (d.note)
    h->jit_note = d.note;
  else if (jit.asked)
    h->jit_note = jit.why;
  else
    h->jit_note.clear();
  if (rc) return rc;
  *r = Route{d, d.family == FDOCT_KERNEL_WAVE_JIT ? jit.fn : nullptr};
  return FDOCT_OK;
}

// After the chain's kernel(s) of any family: end-of-kernel event, the transpose pass where the chain did not write D x H itself,
// end-of-call event, and the call's figures for fdoct_get_timing.
int finish_launch(fdoct_ctx* h, const Route& r, const Call& c, bool staged_timing) {
  hipStream_t st = c.st;
  if (h->record_now && h->rec_last) HIP_TRY(h, hipEventRecord(h->ev[2], st));
  if (r.transpose_pass) {
    if (c.d_out_bscan) HIP_TRY(h, launch_transpose(c.k_mag, c.d_out_bscan, h->H, h->D, c.G, st));
    if (c.d_out_db) HIP_TRY(h, launch_transpose(c.k_db, c.d_out_db, h->H, h->D, c.G, st));
  }
  if (h->record_now && h->rec_last) HIP_TRY(h, hipEventRecord(h->ev[3], st));
  h->last_kernel = r.family;
  h->timing.ascans = (uint64_t)c.in_rows;
  h->timing.bytes_in = (uint64_t)c.in_rows * h->W * c.es;
  h->timing.bytes_out = (uint64_t)c.out_rows * h->D * 4 * ((c.d_out_bscan ? 1 : 0) + (c.d_out_db ? 1 : 0) + (c.k_cx ? 2 : 0));
  h->timing_pending = h->record_now;
  h->timing_staged = staged_timing;
  return FDOCT_OK;
}

float chain_eps(const fdoct_ctx* h) { return (h->cfg.variant == FDOCT_VARIANT_SIM) ? 1e-6f : 1e-5f; }  // sim:949 / main:1222
float kernel_eps(const fdoct_ctx* h) { return h->raw_mag ? 0.0f : chain_eps(h); }                     // fdoct_set_raw_magnitudes
constexpr float kDbScale = (float)(20.0 / 2.303 * 0.6931471805599453);                                // main:1236, times ln 2 (the kernels use log2)

int launch_family_wave(fdoct_ctx* h, const Route& r, const Call& c) {
  const int W = h->W, H = h->H, D = h->D, A = h->A;
  WaveArgs wa{};
  wa.frames = c.kframes;
  wa.pitch_bytes = (long long)r.kpitch;
  wa.total_out_rows = c.out_rows;
  wa.dtype = r.kdt;
  wa.H = H; wa.D = D; wa.A = A;
  wa.ib = h->yb.rows == 1 ? h->d_ib : h->d_ib2d;
  wa.il = h->yb.rows == 1 ? h->d_il : h->d_il2d;
  wa.ib_2d = h->yb.rows > 1;
  wa.win = h->d_win_g;
  wa.win_lo = h->d_win_lo_g;
  wa.yp_lo = h->d_yp_lo; wa.yd_lo = h->d_yd_lo;
  wa.g = h->d_g_g;
  wa.gidx = h->d_wave_gidx;
  wa.tw = h->d_wave_tw;
  wa.tw_count = h->plan.wave_tw.count;
  wa.off_nc = h->plan.wave_tw.off[0]; wa.off_lh = h->plan.wave_tw.off[1]; wa.off_wh = h->plan.wave_tw.off[2];
  wa.off_tww = h->plan.wave_tw.off[3]; wa.off_twmw = h->plan.wave_tw.off[4]; wa.off_twn = h->plan.wave_tw.off[5];
  wa.dcmask = h->cfg.dc_mask;
  wa.inv_A = (float)(1.0 / (double)A);
  wa.eps = kernel_eps(h);
  wa.db_scale = kDbScale;
  wa.out_mag = c.k_mag;
  wa.out_db = c.k_db;
  wa.yp = h->d_yp; wa.yp_2d = h->yp.rows > 1;
  wa.yd = h->d_yd; wa.yd_2d = h->yd.rows > 1;
  wa.minmax = r.need_minmax ? h->d_minmax : nullptr;
  wa.phase = h->d_phase;
  wa.out_cx = c.k_cx;
#ifdef FDOCT_WAVE_PROBE  // measurement build: per-phase cycles of the first workgroups' waves, printed every 50 calls
  {
    static unsigned long long* d_probe = nullptr;
    const size_t pbytes = 4 * 16 * 12 * 8;
    if (!d_probe) {
      (void)hipMalloc(reinterpret_cast<void**>(&d_probe), pbytes);
      (void)hipMemset(d_probe, 0, pbytes);
    }
    wa.probe = d_probe;
    static int calls = 0;
    if (++calls % 50 == 0) {
      std::vector<unsigned long long> v(4 * 16 * 12);
      (void)hipStreamSynchronize(c.st);
      (void)hipMemcpy(v.data(), d_probe, pbytes, hipMemcpyDeviceToHost);
      static const char* names[9] = {"load+A2/A3", "fwd W/2", "re-pack", "inv MW/2", "slope", "gather", "final N/2", "untangle", "epilogue"};
      double tot = 0;
      double sum[9] = {};
      int nw = 0;
      for (int w = 0; w < 64; w++) {
        if (!v[w * 12 + 6]) continue;
        nw++;
        for (int i = 0; i < 9; i++) sum[i] += (double)v[w * 12 + i];
      }
      for (int i = 0; i < 9; i++) tot += sum[i];
      std::fprintf(stderr, "[wave probe] %d waves:", nw);
      for (int i = 0; i < 9; i++) std::fprintf(stderr, " %s %.1f%%", names[i], 100.0 * sum[i] / (tot > 0 ? tot : 1));
      std::fprintf(stderr, "\n");
    }
  }
#endif
  if (h->record_now && h->rec_first) HIP_TRY(h, hipEventRecord(h->ev[1], c.st));
  if (r.jit_fn)
    HIP_TRY(h, wave_jit_launch(r.jit_fn, wa, (int)r.grid, r.waves, r.lds, c.st));
  else
    HIP_TRY(h, launch_wave(W, h->M, h->N, wa, (int)r.grid, r.waves, r.lds, c.st));
  return finish_launch(h, r, c, false);
}

int launch_family_long_rows(fdoct_ctx* h, const Route& r, const Call& c) {
  int rc;
  if (h->record_now && h->rec_first) HIP_TRY(h, hipEventRecord(h->ev[1], c.st));
  if ((rc = run_big(h, c.kframes, c.kframes_lo, r.kdt, r.kpitch, c.nframes, r.need_minmax, c.k_mag, c.k_db, c.st))) return rc;
  return finish_launch(h, r, c, false);
}

int launch_family_generic(fdoct_ctx* h, const Route& r, const Call& c) {
  const int W = h->W, H = h->H, D = h->D, A = h->A;
  const PlanInputs in = plan_inputs(h);
  const GenericPlan& gp = h->plan.gen;
  GenericArgs ga{};
  ga.frames = c.kframes;
  ga.frames_lo = c.kframes_lo;
  ga.pitch_bytes = (long long)r.kpitch;
  ga.total_out_rows = c.out_rows;
  ga.dtype = r.kdt;
  ga.W = W; ga.H = H; ga.N = h->N; ga.D = D; ga.M = h->M; ga.A = A;
  ga.L = generic_buffer_len(in, gp);
  ga.real_half = generic_real_half(in) ? 1 : 0;
  ga.ybuf_len = (W + 3) & ~3;
  ga.ib = h->yb.rows == 1 ? h->d_ib : h->d_ib2d;
  ga.il = h->yb.rows == 1 ? h->d_il : h->d_il2d;
  ga.ib_2d = h->yb.rows > 1;
  ga.yp = h->d_yp; ga.yp_2d = h->yp.rows > 1;
  ga.yd = h->d_yd; ga.yd_2d = h->yd.rows > 1;
  ga.win = h->d_win_g;
  ga.win_lo = h->d_win_lo_g;
  ga.yp_lo = h->d_yp_lo; ga.yd_lo = h->d_yd_lo;
  ga.g = h->d_g_g;
  ga.idx = h->d_idx_g;
  ga.phase = h->d_phase;
  ga.minmax = r.need_minmax ? h->d_minmax : nullptr;
  ga.tw_n = h->d_twg_n; ga.tw_nh = h->d_twg_nh; ga.tw_w = h->d_twg_w; ga.tw_mw = h->d_twg_mw;
  ga.tw_wh = h->d_twg_wh; ga.tw_mwh = h->d_twg_mwh;
  auto put_plan = [](const std::vector<int>& rad, int* rr, unsigned* mag) {
    unsigned long long ns = 1;
    for (size_t i = 0; i < rad.size(); i++) {
      rr[i] = rad[i];
      mag[i] = (unsigned)(((1ull << 32) + ns - 1) / ns);  // ceil(2^32 / Ns); unused for Ns == 1
      ns *= (unsigned)rad[i];
    }
  };
  put_plan(gp.rad_n, ga.rad_n, ga.mag_n);
  if (ga.real_half) put_plan(gp.rad_nh, ga.rad_nh, ga.mag_nh);
  ga.npass_nh = (int)gp.rad_nh.size();
  put_plan(gp.rad_wh, ga.rad_wh, ga.mag_wh);
  put_plan(gp.rad_mwh, ga.rad_mwh, ga.mag_mwh);
  ga.npass_n = (int)gp.rad_n.size(); ga.npass_wh = (int)gp.rad_wh.size(); ga.npass_mwh = (int)gp.rad_mwh.size();
  ga.blu_m = gp.blu_m;
  if (gp.blu_m) {
    put_plan(gp.rad_blu, ga.rad_blu, ga.mag_blu);
    ga.npass_blu = (int)gp.rad_blu.size();
    ga.blu_chirp = h->d_blu_chirp;
    ga.blu_bhat = h->d_blu_bhat;
    ga.tw_blu = h->d_twg_blu;
  }
  ga.zp_full = (h->M > 1 && gp.zp_full) ? 1 : 0;
  ga.zn = gp.zn;
  if (ga.zp_full) {
    auto put_dft = [&](const GenericDftPlan& p, const fdoct_ctx::GenericDftTables& t, GenericDft& d) {
      d.n = p.n;
      d.blu_m = p.blu_m;
      d.npass = (int)p.rad.size();
      put_plan(p.rad, d.rad, d.mag);
      d.tw = t.tw;
      d.chirp = t.chirp;
      d.bhat = t.bhat;
    };
    put_dft(gp.gzf, h->d_gzf, ga.zf);
    put_dft(gp.gzi, h->d_gzi, ga.zi);
  }
  ga.bandpass = h->bandpass ? 1 : 0;
  ga.inplace = gp.inplace ? 1 : 0;
  ga.radix16 = gp.radix16 ? 1 : 0;
  ga.rowwisenormalize = h->cfg.rowwisenormalize;
  ga.dcmask = h->cfg.dc_mask;
  ga.inv_A = (float)(1.0 / (double)A);
  ga.eps = kernel_eps(h);
  ga.db_scale = kDbScale;
  ga.out_mag = c.k_mag;
  ga.out_db = c.k_db;
  ga.out_cx = c.k_cx;
  {
    // the launch's row counter: one of 64 words used in turn, zeroed on the stream in front of the launch (no host
    // synchronisation).  A word comes round again after 64 launches, with any number of them still queued: what keeps it safe is
    // stream order alone -- a handle's launches run one after the other on its stream (fdoct_set_stream puts the new stream behind
    // the old), so the memset that re-zeroes a word runs after the launch that used it last has finished
    // (tests/test_gpu_stream_order.py: 130 launches behind a stalled stream)
    constexpr unsigned kGenTickets = 64;
    static const bool no_tickets = [] { const char* e = std::getenv("FDOCT_GENERIC_TICKETS"); return e && std::atoi(e) == 0; }();  // measurement: the static stride
    if (h->d_gen_tickets && !no_tickets) {   // (allocated with the kernel's tables: ensure_generic_tables)
      unsigned* t = h->d_gen_tickets + (h->gen_ticket_seq++ % kGenTickets);
      HIP_TRY(h, hipMemsetAsync(t, 0, sizeof(unsigned), c.st));
      ga.row_ticket = t;
    }
  }
  if (h->record_now && h->rec_first) HIP_TRY(h, hipEventRecord(h->ev[1], c.st));
  HIP_TRY(h, launch_generic(ga, (int)r.grid, r.lds, c.st));
  return finish_launch(h, r, c, false);
}

#if defined(FDOCT_RUNTIME_ABLATE) || defined(FDOCT_CLOCKPROBE) || defined(FDOCT_FUSED_PROBE)
#define FDOCT_DEV_BUILD 1
// Measurement builds only (tools/ablate.sh, tools/mkvariant.sh probe): the stage-skipping mask and the in-kernel clock probes.
void dev_build_hooks(FusedArgs& a, hipStream_t st) {
#ifdef FDOCT_RUNTIME_ABLATE
  static const int ablate = [] { const char* ab = std::getenv("FDOCT_ABLATE"); return ab ? std::atoi(ab) : 0; }();
  a.ablate = ablate;
#endif
#ifdef FDOCT_FUSED_PROBE
  {  // share of a wave's cycles per phase of the row loop, first workgroups' waves, printed every 50 launches
    static unsigned long long* d_ph = nullptr;
    const size_t n = 4 * 16 * FUSED_PROBE_PHASES;
    if (!d_ph) {
      (void)hipMalloc(reinterpret_cast<void**>(&d_ph), n * 8);
      (void)hipMemset(d_ph, 0, n * 8);
    }
    a.phase_probe = d_ph;
    static int calls = 0;
    if (++calls % 50 == 0) {
      std::vector<unsigned long long> v(n);
      (void)hipStreamSynchronize(st);
      (void)hipMemcpy(v.data(), d_ph, n * 8, hipMemcpyDeviceToHost);
      static const char* names[10] = {"loads' tail + A2/A3", "window + slope + staging", "prefetch issue + gather", "FFT step 1 (registers)", "row swap",
                                      "twiddle + radix 4 + LDS writes", "LDS read-back", "step-5 twiddles + radix 16", "untangle + magnitude", "epilogue + stores"};
      double sum[10] = {}, tot = 0;
      int nw = 0;
      for (int w = 0; w < 64; w++) {
        if (!v[w * FUSED_PROBE_PHASES + 3]) continue;
        nw++;
        for (int i = 0; i < 10; i++) sum[i] += (double)v[w * FUSED_PROBE_PHASES + i];
      }
      for (int i = 0; i < 10; i++) tot += sum[i];
      std::fprintf(stderr, "[fused probe] %d waves, %.0f cycles per wave:", nw, nw ? tot / nw : 0.0);
      for (int i = 0; i < 10; i++) std::fprintf(stderr, " | %s %.1f%%", names[i], 100.0 * sum[i] / (tot > 0 ? tot : 1));
      std::fprintf(stderr, "\n");
    }
  }
#endif
#ifdef FDOCT_CLOCKPROBE
  static unsigned long long* d_probe = nullptr;
  const size_t pbytes = (32 + 1024) * 8;
  if (!d_probe) {
    (void)hipMalloc(reinterpret_cast<void**>(&d_probe), pbytes);
    (void)hipMemset(d_probe, 0, pbytes);
  }
  a.probe = d_probe;
  static int calls = 0;
  if (++calls % 64 == 0) {
    std::vector<unsigned long long> v(32 + 1024);
    (void)hipStreamSynchronize(st);
    (void)hipMemcpy(v.data(), d_probe, pbytes, hipMemcpyDeviceToHost);
    std::fprintf(stderr, "[probe]");
    for (int w = 0; w < 16; w++)
      if (v[2 * w + 1]) std::fprintf(stderr, " w%d %.0fus@%.2fGHz", w, v[2 * w + 1] / 100.0, v[2 * w] / (v[2 * w + 1] * 10.0));
    unsigned long long t0 = ~0ull;
    std::vector<double> stv, en;
    for (int b = 0; b < 512; b++)
      if (v[32 + 2 * b]) t0 = std::min(t0, v[32 + 2 * b]);
    for (int b = 0; b < 512; b++)
      if (v[32 + 2 * b]) {
        stv.push_back((v[32 + 2 * b] - t0) / 100.0);
        en.push_back((v[32 + 2 * b + 1] - t0) / 100.0);
      }
    if (!stv.empty()) {
      std::sort(stv.begin(), stv.end());
      std::sort(en.begin(), en.end());
      std::fprintf(stderr, "\n[probe] %zu blocks: start max %.1f us; end min %.1f p10 %.1f p50 %.1f p90 %.1f max %.1f us", stv.size(),
                   stv.back(), en.front(), en[en.size() / 10], en[en.size() / 2], en[en.size() * 9 / 10], en.back());
    }
    std::fprintf(stderr, "\n");
  }
#else
  (void)st;
#endif
}
#endif

int launch_family_fused(fdoct_ctx* h, const Route& r, const Call& c) {
  const int W = h->W, H = h->H, D = h->D, A = h->A;
  int rc;
  hipStream_t st = c.st;
  FusedArgs a{};
  a.frames = c.kframes;
  a.frames_lo = c.kframes_lo;
  a.pitch_bytes = (long long)r.kpitch;
  a.total_out_rows = c.out_rows;
  a.W = W;
  a.H = H;
  a.D = D;
  a.A = A;
  a.split = h->plan.split;
  a.scratch_bytes = h->plan.scratch_bytes;
  a.tw_count = h->plan.tw_count;
  a.ib = h->d_ib;
  a.ib2d = h->d_ib2d_f;
  a.il = h->d_il;
  a.il2d = h->d_il2d_f;
  a.ilp = h->d_il_p;
  a.il16 = h->d_il16;
  a.il16_2d = h->d_il16_2d;
  a.yp = h->d_yp;
  a.yp_2d = h->yp.rows > 1;
  a.yd = h->d_yd;
  a.yd_2d = h->yd.rows > 1;
  a.win = h->d_win;
  a.g = h->d_g;
  a.gidx = h->d_gidx;
  a.tw = h->d_tw;
  a.utw = h->d_utw;
  a.phase = h->d_phase;
  a.minmax = r.need_minmax ? h->d_minmax : nullptr;
  a.rowwisenormalize = h->cfg.rowwisenormalize;
  a.dcmask = h->cfg.dc_mask;
  a.need_rc = (a.ib2d || a.yp_2d || a.yd_2d || a.minmax || a.frames_lo) ? 1 : 0;
  a.inv_A = (float)(1.0 / (double)A);
  a.eps = kernel_eps(h);
  a.db_scale = kDbScale;
  a.out_mag = c.k_mag;
  a.out_db = c.k_db;
#ifdef FDOCT_DEV_BUILD
  dev_build_hooks(a, st);
#endif

  const FusedPlan& p = *h->plan.fused;
  const FusedLaunch& l = r.fused;
  a.lds_planes = l.lds_planes;
  a.prec = l.prec;
  if (l.tro) {
    if (!h->d_tro_fault) {
      // (coherent, mapped host memory: the buffer's flags, fdoct_ctx.h.  The kernels raise the word with a plain system-scope
      // STORE of 1 -- a read-modify-write atomic on host memory would need PCIe AtomicOps on the link and is dropped silently
      // where they are missing: ADVICE r4)
      if ((rc = h->d_tro_fault.reserve(h, sizeof(unsigned)))) return rc;
      *h->d_tro_fault = 0u;
    }
    h->tro_used = true;
    a.tr_fault = h->d_tro_fault;
    a.tro = 1;
    a.tr_ring = l.tro->ring;
    a.tr_tpf = l.tro->tpf;
    a.tr_tpf_magic = l.tro->tpf_magic;
    a.tr_total_tiles = l.tro->total_tiles;
  }
  if (h->record_now && h->rec_first) HIP_TRY(h, hipEventRecord(h->ev[1], st));
  h->ylin_rows = 0;
  if (h->staged) {
    // one k-linear row per INPUT A-scan between the stages: the resample stage runs over the in_rows input rows as they
    // lie (A = 1), the FFT stage gathers the A rows of an output A-scan
    if ((rc = h->ws_ylin.reserve(h, (size_t)c.in_rows * h->plan.NC * sizeof(float2)))) return rc;
    a.ylin = h->ws_ylin;
    h->ylin_rows = c.in_rows;
    FusedArgs a1 = a;
    a1.stage = 1;
    a1.A = 1;
    a1.inv_A = 1.f;
    a1.total_out_rows = c.in_rows;
    HIP_TRY(h, launch_fused(p, a1, r.kdt, h->plan.cplx, l.lean, (int)l.stage1_grid, l.block, l.lds, st));
    if (h->record_now) HIP_TRY(h, hipEventRecord(h->ev[4], st));
    a.stage = 2;
  }
  HIP_TRY(h, launch_fused(p, a, r.kdt, h->plan.cplx, l.lean, (int)l.grid, l.block, l.lds, st));
  return finish_launch(h, r, c, h->staged);
}

// The passes in front of the chain, as the route names them; leaves what the chain's kernel reads in c.kframes / c.kframes_lo
// (r.kdt samples at r.kpitch bytes per row).
static int run_passes_in_front(fdoct_ctx* h, const Route& r, Call& c, const void* d_frames, fdoct_dtype dtype, size_t pitch_bytes) {
  const int W = h->W, n = h->cfg.movavgn;
  hipStream_t st = c.st;
  int rc;
  if (r.colour) {  // interleaved B,G,R frames: the colour stage, which bins unless the chain's kernel does
    void* co = nullptr;
    if ((rc = run_colour(h, d_frames, c.nframes, W * h->fe_binx, h->H * h->fe_biny, pitch_bytes, h->colour, h->fe_median,
                         r.bin2_in_kernel ? 1 : h->fe_binx, r.bin2_in_kernel ? 1 : h->fe_biny, &co, &pitch_bytes)))
      return rc;
    d_frames = c.kframes = co;
    dtype = h->colour == 3 ? FDOCT_F64 : FDOCT_U8;
  }
  size_t pitch = pitch_bytes;
  if (r.frontend) {  // raw camera frames: medianBlur + binning first (main:953-958); the caller's pitch describes the RAW rows
    void* fo = nullptr;
    if ((rc = run_frontend(h, d_frames, kernel_dtype(dtype), c.nframes, W * h->fe_binx, h->H * h->fe_biny, pitch_bytes, h->fe_median, h->fe_binx,
                           h->fe_biny, &fo, &pitch)))
      return rc;
    c.kframes = fo;
  }
  if (r.pre == PrePass::None) return FDOCT_OK;
  // one f32 plane of packed rows, and where the pass keeps the sums in double a second one with their low words
  DevBuf<float>& hi = r.pre == PrePass::F64Split ? h->ws_f32 : h->ws_mov;
  DevBuf<float>& lo = r.pre == PrePass::F64Split ? h->ws_f32_lo : h->ws_mov_lo;
  if ((rc = hi.reserve(h, (size_t)c.in_rows * W * 4))) return rc;
  if (r.frames_lo() && (rc = lo.reserve(h, (size_t)c.in_rows * W * 4 + 32))) return rc;
  switch (r.pre) {
    case PrePass::F64Split:  // data_y doubles (main:987): split once into two f32 planes on the device, x = hi + lo
      HIP_TRY(h, launch_f64_split(static_cast<const double*>(d_frames), (long long)(pitch_bytes / 8), hi, lo, W, c.in_rows, st));
      break;
    case PrePass::MovAvgF64:  // doubles through smoothmovavg (main:987-991): the tap sums in double, then the two planes
      HIP_TRY(h, launch_movavg_f64(static_cast<const double*>(d_frames), (long long)(pitch_bytes / 8), W, c.in_rows, n, hi, lo, st));
      break;
    case PrePass::MovAvgF32Wide:  // ... of float frames: sums in double, two planes
      HIP_TRY(h, launch_movavg_f32_wide(static_cast<const float*>(d_frames), (long long)(pitch_bytes / 4), W, c.in_rows, n, hi, lo, st));
      break;
    default:  // smoothmovavg (main:990-991) runs before everything else, on the raw samples
      HIP_TRY(h, launch_movavg(c.kframes, kernel_dtype(dtype), (long long)pitch, W, c.in_rows, n, hi, st));
      break;
  }
  c.kframes = hi;
  c.kframes_lo = r.frames_lo() ? static_cast<const float*>(lo) : nullptr;
  return FDOCT_OK;
}

int check_call(fdoct_ctx* h, fdoct_dtype dtype, size_t pitch_bytes, const float* out_bscan, const float* out_db) {
  if (!h->yb.rows) return fail(h, FDOCT_ERR_STATE, "no background set (fdoct_set_background)");
  if (!out_bscan && !out_db) return fail(h, FDOCT_ERR_INVALID, "no output requested");
  if (h->raw_mag && out_db) return fail(h, FDOCT_ERR_INVALID, "raw magnitudes are on (fdoct_set_raw_magnitudes): out_db must be NULL");
  const size_t es = frame_pixel_bytes(h, dtype);
  if (!es) return fail(h, FDOCT_ERR_INVALID, "bad dtype");
  if (pitch_bytes && pitch_bytes < es * h->W) return fail(h, FDOCT_ERR_INVALID, "pitch smaller than a row");  // (0: packed rows)
  return FDOCT_OK;
}

// What both entry points enqueue between the route and the chain's kernel: the call's quantities, the first event, the passes in
// front of the chain and the whole-frame min / max pass.  Where the chain writes is the entry point's to add.
static int begin_call(fdoct_ctx* h, const Route& r, const void* d_frames, fdoct_dtype dtype, int nframes, size_t es, size_t pitch_bytes, Call* c) {
  c->st = h->stream;
  c->nframes = nframes;
  c->G = nframes / h->A;
  c->in_rows = (long long)nframes * h->H;
  c->out_rows = (long long)c->G * h->H;
  c->es = es;
  c->kframes = d_frames;
  if (h->record_now && h->rec_first) HIP_TRY(h, hipEventRecord(h->ev[0], c->st));
  if (int rc = run_passes_in_front(h, r, *c, d_frames, dtype, pitch_bytes)) return rc;
  if (r.need_minmax) {
    // [nframes] results followed by the fast kernel's per-workgroup partials
    const size_t mm_elems = (size_t)nframes + (size_t)minmax_partial_count(nframes);
    if (int rc = h->d_minmax.reserve(h, mm_elems * sizeof(float2))) return rc;
    HIP_TRY(h, launch_minmax(c->kframes, r.kdt, (long long)r.kpitch, h->W, h->H, nframes, h->d_yd, h->yd.rows > 1, h->d_minmax,
                             h->d_minmax + nframes, c->st));
  }
  return FDOCT_OK;
}

// Enqueue the whole path for device-resident frames.  d_out_* are row-major or
// transposed per `layout`.
int enqueue_one(fdoct_ctx* h, const void* d_frames, fdoct_dtype dtype, int nframes, size_t pitch_bytes,
                float* d_out_bscan, float* d_out_db, fdoct_layout layout) {
  if (!h) return FDOCT_ERR_INVALID;
  if (!d_frames || nframes <= 0) return fail(h, FDOCT_ERR_INVALID, "no frames");
  if (nframes % h->A) return fail(h, FDOCT_ERR_INVALID, "nframes must be a multiple of averages");
  if (int rc = check_call(h, dtype, pitch_bytes, d_out_bscan, d_out_db)) return rc;
  const size_t es = frame_pixel_bytes(h, dtype);
  if (pitch_bytes == 0) pitch_bytes = es * h->W * h->fe_binx;
  DEVICE_SCOPE(h);
  int rc;
  Route r;
  RouteInputs in = route_inputs(h, dtype, (uintptr_t)d_frames, pitch_bytes, nframes);
  in.out_bscan_addr = (uintptr_t)d_out_bscan;
  in.out_db_addr = (uintptr_t)d_out_db;
  in.layout = layout;
  if ((rc = choose_route(h, in, &r))) return rc;
  Call c;
  c.d_out_bscan = d_out_bscan;
  c.d_out_db = d_out_db;
  if ((rc = begin_call(h, r, d_frames, dtype, nframes, es, pitch_bytes, &c))) return rc;
  // ---- where the chain writes: the caller's arrays, or the transpose pass's input
  c.k_mag = d_out_bscan;
  c.k_db = d_out_db;
  if (r.transpose_pass) {
    const size_t bytes = (size_t)c.out_rows * h->D * 4;
    if ((rc = h->ws_tr.reserve(h, bytes * 2))) return rc;
    if (d_out_bscan) c.k_mag = h->ws_tr;
    if (d_out_db) c.k_db = h->ws_tr + (size_t)c.out_rows * h->D;
  }
  switch (r.family) {
    case FDOCT_KERNEL_WAVE:
    case FDOCT_KERNEL_WAVE_JIT: return launch_family_wave(h, r, c);
    case FDOCT_KERNEL_LONG_ROWS: return launch_family_long_rows(h, r, c);
    case FDOCT_KERNEL_GENERIC: return launch_family_generic(h, r, c);
    default: return launch_family_fused(h, r, c);
  }
}

// The complex A-scan (include/fdoct_complex.h; the entry point is the add-on library's, fdoct_complex.cpp): the chain of enqueue_one up
// to the final transform, whose first numdisplaypoints bins go out as (re, im) pairs, row-major, to d_out -- [nframes H D].  Device
// memory on both sides, enqueues only.  d_out null: every check, the route (which may compile) and nothing else -- what the entry point
// asks before it copies host frames up; frames_addr is then all that is read of d_frames.
int enqueue_complex(fdoct_ctx* h, const void* d_frames, fdoct_dtype dtype, int nframes, size_t pitch_bytes, float2* d_out) {
  if (!h) return FDOCT_ERR_INVALID;
  if (!d_frames || nframes <= 0) return fail(h, FDOCT_ERR_INVALID, "no frames");
  if (!h->yb.rows) return fail(h, FDOCT_ERR_STATE, "no background set (fdoct_set_background)");
  // the reference averages magnitudes (main:1192-1211); a mean of complex A-scans is another quantity, which nothing here defines
  if (h->A != 1 || h->sim_group != 1) return fail(h, FDOCT_ERR_UNSUPPORTED, "the complex A-scan needs averages = 1");
  const size_t es = frame_pixel_bytes(h, dtype);
  if (!es) return fail(h, FDOCT_ERR_INVALID, "bad dtype");
  if (pitch_bytes && pitch_bytes < es * h->W * h->fe_binx) return fail(h, FDOCT_ERR_INVALID, "pitch smaller than a row");
  if (pitch_bytes == 0) pitch_bytes = es * h->W * h->fe_binx;
  DEVICE_SCOPE(h);
  int rc;
  Route r;
  RouteInputs in = route_inputs(h, dtype, (uintptr_t)d_frames, pitch_bytes, nframes);
  in.cx = true;
  if ((rc = choose_route(h, in, &r))) return rc;
  if (r.family != FDOCT_KERNEL_WAVE_JIT && r.family != FDOCT_KERNEL_GENERIC) return fail(h, FDOCT_ERR_DEVICE, "internal: the complex A-scan routed to a kernel that does not write it");
  if (!d_out) return FDOCT_OK;
  h->rec_first = h->rec_last = true;
  h->record_now = h->async_timing;  // (event records cost stream time: as fdoct_process_async, only where fdoct_set_timing asked)
  Call c;
  c.k_cx = d_out;
  if ((rc = begin_call(h, r, d_frames, dtype, nframes, es, pitch_bytes, &c))) return rc;
  return r.family == FDOCT_KERNEL_GENERIC ? launch_family_generic(h, r, c) : launch_family_wave(h, r, c);
}

// The whole path for device-resident frames.  The reference's own layout (bscan is D x H, main:1220) is produced by the
// chain writing row-major B-scans into a library-owned intermediate and a transpose pass; a long batch is cut into chunks of
// whole B-scans whose intermediate (tr_chunk_bytes, reused by every chunk) is small enough to stay in the 256 MB Infinity
// Cache between the two kernels, so that per A-scan only the camera samples and the final image cross HBM.
int enqueue(fdoct_ctx* h, const void* d_frames, fdoct_dtype dtype, int nframes, size_t pitch_bytes,
            float* d_out_bscan, float* d_out_db, fdoct_layout layout) {
  if (!h) return FDOCT_ERR_INVALID;
  if (h->d_tro_fault && *static_cast<volatile unsigned*>(h->d_tro_fault)) {  // raised by an earlier asynchronous call
    *static_cast<volatile unsigned*>(h->d_tro_fault) = 0u;
    return fail(h, FDOCT_ERR_DEVICE, "transposed store: a wave of an earlier call timed out waiting for its tile buffer; that call's results are invalid");
  }
  h->rec_first = h->rec_last = true;
  if (layout != FDOCT_LAYOUT_TRANSPOSED_DxH || nframes <= 0 || (nframes % h->A) || !d_frames)
    return enqueue_one(h, d_frames, dtype, nframes, pitch_bytes, d_out_bscan, d_out_db, layout);
  const int G = nframes / h->A;
  const size_t per_group = (size_t)h->H * h->D * 4 * ((d_out_bscan ? 1 : 0) + (d_out_db ? 1 : 0));
  long long cg = per_group ? (long long)(h->tr_chunk_bytes / per_group) : G;
  if (cg < 1) cg = 1;
  if (G <= cg) return enqueue_one(h, d_frames, dtype, nframes, pitch_bytes, d_out_bscan, d_out_db, layout);
  const size_t es = frame_pixel_bytes(h, dtype);
  if (!es) return fail(h, FDOCT_ERR_INVALID, "bad dtype");
  const size_t pitch = pitch_bytes ? pitch_bytes : es * (size_t)h->W * h->fe_binx;
  {  // the whole call's route: where the chain writes D x H itself there is no intermediate at all, and nothing to cut
    DEVICE_SCOPE(h);
    Route whole;
    RouteInputs in = route_inputs(h, dtype, (uintptr_t)d_frames, pitch, nframes);
    in.out_bscan_addr = (uintptr_t)d_out_bscan;
    in.out_db_addr = (uintptr_t)d_out_db;
    in.layout = layout;
    if (h->yb.rows && choose_route(h, in, &whole) == FDOCT_OK && whole.fused.tro)
      return enqueue_one(h, d_frames, dtype, nframes, pitch_bytes, d_out_bscan, d_out_db, layout);
  }
  const size_t frame_stride = pitch * (size_t)h->H * h->fe_biny;  // raw camera rows when a front end is set
  const size_t out_group = (size_t)h->H * h->D;
  uint64_t ascans = 0, bin = 0, bout = 0;
  for (long long g0 = 0; g0 < G; g0 += cg) {
    const int ng = (int)std::min<long long>(cg, G - g0);
    h->rec_first = g0 == 0;
    h->rec_last = g0 + ng >= G;
    const unsigned char* fr = static_cast<const unsigned char*>(d_frames) + (size_t)g0 * h->A * frame_stride;
    int rc = enqueue_one(h, fr, dtype, ng * h->A, pitch_bytes, d_out_bscan ? d_out_bscan + (size_t)g0 * out_group : nullptr,
                         d_out_db ? d_out_db + (size_t)g0 * out_group : nullptr, layout);
    if (rc) {
      h->rec_first = h->rec_last = true;
      return rc;
    }
    ascans += h->timing.ascans;
    bin += h->timing.bytes_in;
    bout += h->timing.bytes_out;
  }
  h->rec_first = h->rec_last = true;
  h->timing.ascans = ascans;
  h->timing.bytes_in = bin;
  h->timing.bytes_out = bout;
  return FDOCT_OK;
}

}  // namespace fdoct_impl
