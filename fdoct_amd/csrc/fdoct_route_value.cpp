// fdoct_route_value.cpp -- make_route (fdoct_route_value.h).  Plain C++ without HIP.
#include "fdoct_route_value.h"

#include <algorithm>

namespace fdoct {

int kernel_dtype(int dt) {
  switch (dt) {
    case FDOCT_U8: return FDOCT_K_U8;
    case FDOCT_U16: return FDOCT_K_U16;
    case FDOCT_F32: return FDOCT_K_F32;
    default: return -1;
  }
}

size_t dtype_size(int dt) {
  switch (dt) {
    case FDOCT_U8: return 1;
    case FDOCT_U16: return 2;
    case FDOCT_F32: return 4;
    case FDOCT_F64: return 8;
    default: return 0;
  }
}

static int refuse(std::string* why, int code, const std::string& text) {
  *why = text;
  return code;
}

int colour_refusal(const char* who, int channelnum, int dtype, int mediann, std::string* why) {
  const std::string w = std::string(who) + ": ";
  if (channelnum < 0 || channelnum > 3) return refuse(why, FDOCT_ERR_INVALID, w + "channelnum must be 0, 1, 2 (B, G, R) or 3 (their sum)");
  if (dtype != FDOCT_U8)
    return refuse(why, FDOCT_ERR_UNSUPPORTED, w + "colour input takes 8-bit interleaved B,G,R frames (what cv::VideoCapture::read delivers), no other sample type");
  if (mediann != 0 && mediann != 3 && mediann != 5 && mediann != 7) return refuse(why, FDOCT_ERR_INVALID, w + "mediann must be 0, 3, 5 or 7");
  if (channelnum == 3 && mediann > 0)
    return refuse(why, FDOCT_ERR_UNSUPPORTED, w + "the channel sum is a frame of doubles and cv::medianBlur rejects CV_64F: no median with channelnum 3");
  return FDOCT_OK;
}

// What make_fused_launch reads of the route's inputs for a call whose kernel reads samples of type kdt.
static FusedLaunchInputs fused_launch_inputs(const RouteInputs& in, int kdt, bool need_minmax, bool frames_lo, bool want_tro) {
  FusedLaunchInputs f;
  f.W = in.W; f.H = in.H; f.D = in.D; f.A = in.A;
  f.kdt = kdt;
  f.bg_rows = in.bg_rows; f.pi = in.pi; f.dark = in.dark;
  f.rowwisenormalize = in.rowwisenormalize; f.minmax = need_minmax; f.frames_lo = frames_lo;
  f.precise_div = in.precise_div; f.staged = in.staged; f.force_general = in.force_general;
  f.block_override = in.block_override; f.grid_override = in.grid_override; f.num_cu = in.num_cu;
  f.groups = in.nframes / in.A; f.in_rows = (long long)in.nframes * in.H; f.out_rows = f.groups * in.H;
  f.want_tro = want_tro; f.ring_cap = in.ring_cap;
  return f;
}

// May the chain write the reference's D x H layout itself, as far as the CALL says (whether the configuration has such a kernel and
// its launch fits is make_fused_launch's part)?  8/16-bit frames that go to the kernel as they are, 16-byte aligned outputs, and
// offsets the write-out can address.  (dtype, frames_addr, pitch_bytes: of the frames as the passes in front of the chain see them.)
static bool transposed_store_callable(const RouteInputs& in, int dtype, uintptr_t frames_addr, size_t pitch_bytes) {
  if (!in.tro_enabled || !in.plan->fused || !in.bg_rows) return false;
  if (dtype != FDOCT_U8 && dtype != FDOCT_U16) return false;
  if (in.fe_median > 0 || in.fe_binx > 1 || in.fe_biny > 1 || in.movavgn > 0) return false;
  const size_t valign = dtype == FDOCT_U8 ? 8 : 16;
  if ((frames_addr % valign) || (pitch_bytes % valign)) return false;
  if ((in.out_bscan_addr % 16) || (in.out_db_addr % 16)) return false;
  if ((long long)(in.nframes / in.A) * in.H >= 0x7fffffffLL) return false;
  // the write-out addresses one B-scan with 32-bit byte offsets inside a buffer descriptor of 0x7ffffff0 bytes
  return (size_t)in.D * (size_t)in.H * 4 < 0x7ffffff0u;
}

int route_precheck(const RouteInputs& in, std::string* why) {
  const Plan& pl = *in.plan;
  if (in.cx && pl.gen.use_big)
    return refuse(why, FDOCT_ERR_UNSUPPORTED, "the complex A-scan is not written by the long-row path (rows that do not fit a compute unit's LDS)");
  if (!(pl.fused && !in.cx) && pl.gen.rc) return refuse(why, pl.gen.rc, pl.gen.why);
  if (in.D > in.N) return refuse(why, FDOCT_ERR_INVALID, "numdisplaypoints > numfftpoints");
  if (in.colour >= 0) {
    if (int rc = colour_refusal("colour input", in.colour, in.dtype, in.fe_median, why)) return rc;
    if (in.pitch_bytes < 3 * (size_t)in.W * in.fe_binx) return refuse(why, FDOCT_ERR_INVALID, "pitch smaller than a row of B,G,R pixels");
  }
  return FDOCT_OK;
}

int make_route(const RouteInputs& in, CanCompile can_compile, void* ctx, RouteDecision* out, std::string* why) {
  if (int rc = route_precheck(in, why)) return rc;
  const Plan& pl = *in.plan;
  const bool cx = in.cx;
  RouteDecision d;
  d.tables |= (pl.fused && !cx) ? TABLES_FUSED : TABLES_GENERIC;
  const int W = in.W, H = in.H, D = in.D, A = in.A;
  const long long out_rows = (long long)(in.nframes / A) * H;
  int dtype = in.dtype;
  uintptr_t frames_addr = in.frames_addr;
  size_t pitch_bytes = in.pitch_bytes;
  // A colour handle: the colour stage runs first and takes the median / binning with it; from here on the call is routed as
  // what that stage leaves -- the front end's bytes in a library workspace (channelnum 0-2), or packed doubles (3).
  const bool colour = in.colour >= 0;
  if (colour) {
    d.colour = true;
    frames_addr = 0;
    if (in.colour == 3) {
      dtype = FDOCT_F64;
      pitch_bytes = frontend_pitch(W, 8);
    } else {
      pitch_bytes = frontend_pitch(W * in.fe_binx, 1);  // (the unbinned channel: what a kernel that bins in its own loads would read)
    }
  }
  const size_t es = dtype_size(dtype);
  int kdt = kernel_dtype(dtype);
  // with row-wise normalisation on, every non-degenerate row already spans [0,1] and the whole-frame pass (main:1128) is the identity
  d.need_minmax = in.normalize && !in.rowwisenormalize;
  // pi / dark frames, the band-pass and the normalisations are compile-time options of the wave-per-row kernel: the library's own
  // instantiations are the plain set-up, a handle that uses one of them gets its kernel from the run-time compiler
  // ... and so are the dispersion phase (complex rows, a full-length final transform) and a display beyond numfftpoints / 2
  const int wave_opt = (in.pi ? FDOCT_WAVE_OPT_PI : 0) | (in.dark ? FDOCT_WAVE_OPT_DARK : 0) |
                       (in.bandpass && in.M > 1 ? FDOCT_WAVE_OPT_BANDPASS : 0) | (in.rowwisenormalize ? FDOCT_WAVE_OPT_ROWNORM : 0) |
                       (d.need_minmax ? FDOCT_WAVE_OPT_FRAMENORM : 0) | (in.phase ? FDOCT_WAVE_OPT_CPLX : 0) |
                       (!in.phase && D > in.N / 2 ? FDOCT_WAVE_OPT_DEEP : 0) | (cx ? FDOCT_WAVE_OPT_CXOUT : 0);
  // The wave-per-row kernel's launch, where its tables leave room for at least one wave's buffers: as many waves as LDS and
  // the shape's register budget allow, at most one workgroup per CU.
  struct WaveLaunch {
    int waves = 0;
    size_t lds = 0;
    long long grid = 0;
  };
  auto wave_launch = [&](int opt, WaveLaunch* l) {
    const size_t shared = wave_shared_lds_bytes(pl.wave_tw.count, W, in.M, in.N, in.bg_rows > 1, opt);
    const size_t priv = wave_private_lds_bytes(W, in.M, in.N, opt);
    if (shared + priv > 160 * 1024 - 64) return false;
    int waves = (int)((160 * 1024 - 64 - shared) / priv);
    if (waves > wave_max_waves(W, in.M, in.N, opt)) waves = wave_max_waves(W, in.M, in.N, opt);
    if (in.block_override && in.block_override / 64 >= 1 && in.block_override / 64 <= waves) waves = in.block_override / 64;
    l->waves = waves;
    l->lds = shared + (size_t)waves * priv;
    l->grid = std::min<long long>(in.grid_override > 0 ? in.grid_override : in.num_cu, (out_rows + waves - 1) / waves);   // (a wave takes one row at a time)
    return true;
  };
  auto take = [&](const WaveLaunch& l) { d.waves = l.waves, d.lds = l.lds, d.grid = l.grid; };
  bool compiled = false;   // the run-time compiler delivers the kernel of d.wave_opt
  // 2 x 2 binning with nothing else in front of the chain, on a configuration the wave-per-row kernel takes: the kernel compiled
  // for the handle does the binning in its own loads (FDOCT_WAVE_OPT_BIN2) and the pass over the raw frames is skipped.
  // (Measured on the shipped shapes, tools/bench_generic.py with and without FDOCT_JIT=0: + 4.5 % on 160-sample 8-bit rows, + 5 % on
  // 640-sample 16-bit rows, - 1 % on 640-sample 8-bit rows -- twenty 2-byte loads per lane cost what the pass saves: those keep the pass.)
  if (!cx && in.fe_median == 0 && in.fe_binx == 2 && in.fe_biny == 2 && (dtype == FDOCT_U16 || (dtype == FDOCT_U8 && W <= 320)) && in.movavgn == 0 &&
      in.jit && !pl.fused && !pl.gen.use_big && in.plan_override > -2 && !in.phase && D <= in.N / 2 && !d.need_minmax &&
      (frames_addr % 4 == 0) && (pitch_bytes % 4 == 0) && pitch_bytes >= es * 2 * (size_t)W && out_rows < 0x7fffffffLL &&
      wave_jit_shape_ok(W, in.M, in.N, D)) {
    d.tables |= TABLES_WAVE;
    // (no room for even one wave, or no kernel: the ordinary path -- binning pass, then whichever kernel fits)
    WaveLaunch l;
    if (wave_launch(wave_opt | FDOCT_WAVE_OPT_BIN2, &l) && can_compile(ctx, kdt, wave_opt | FDOCT_WAVE_OPT_BIN2)) {
      d.bin2_in_kernel = true;
      compiled = true;
      d.wave_opt = wave_opt | FDOCT_WAVE_OPT_BIN2;
      take(l);
    }
  }
  // ---- passes in front of the chain, and what they leave for its kernel to read
  uintptr_t kaddr = frames_addr;
  size_t kpitch = pitch_bytes;
  if (colour) {
    if (in.colour != 3 && !d.bin2_in_kernel) kpitch = frontend_pitch(W, 1);
  } else if (!d.bin2_in_kernel && (in.fe_median > 0 || in.fe_binx > 1 || in.fe_biny > 1)) {
    if (dtype != FDOCT_U8 && dtype != FDOCT_U16)
      return refuse(why, FDOCT_ERR_UNSUPPORTED, "the front end (median / binning) takes the camera's 8- or 16-bit frames");
    if (pitch_bytes < es * (size_t)W * in.fe_binx) return refuse(why, FDOCT_ERR_INVALID, "pitch smaller than a raw camera row");
    d.frontend = true;
    kaddr = 0;                                                  // a library workspace: aligned
    kpitch = frontend_pitch(W, es);
  }
  if (dtype == FDOCT_F64) {
    if (pitch_bytes % 8) return refuse(why, FDOCT_ERR_INVALID, "f64 pitch must be a multiple of 8");
    d.pre = PrePass::F64Split;
    kaddr = 0;
    kpitch = (size_t)W * 4;
    kdt = FDOCT_K_F32;
  }
  if (in.movavgn > 0) {
    // (float frames: the tap sums of non-integer samples go on as two planes, like the doubles' -- round 6: a float sum rounds at
    // the size of the DC level, 0.87 x the tolerance from the chain in double under fringes of 1e-3 of it in the sweeps)
    const bool wide = dtype == FDOCT_F32 && !d.frontend && (pitch_bytes % 4 == 0) && (frames_addr % 4 == 0);
    d.pre = dtype == FDOCT_F64 ? PrePass::MovAvgF64 : wide ? PrePass::MovAvgF32Wide : PrePass::MovAvg;
    kaddr = 0;
    kpitch = (size_t)W * 4;
    kdt = FDOCT_K_F32;
  }
  d.kdt = kdt;
  d.kpitch = kpitch;
  // the specialised kernels read 16-byte vectors; anything else goes through the generic kernel
  const size_t valign = (kdt == FDOCT_K_U8) ? 8 : 16;
  const bool misaligned = (kaddr % valign) || (kpitch % valign);
  const bool run_generic = cx || !pl.fused || misaligned;
  if (run_generic && pl.gen.rc) return refuse(why, pl.gen.rc, pl.gen.why);
  if (run_generic) d.tables |= TABLES_GENERIC;
  if (run_generic && in.staged) return refuse(why, FDOCT_ERR_UNSUPPORTED, "staged mode needs a specialised kernel for this configuration");

  const bool transposed = in.layout == FDOCT_LAYOUT_TRANSPOSED_DxH;
  if (!run_generic) {  // the fused family: its whole launch, or why it cannot run
    const bool want_tro = transposed && !d.frontend && d.pre == PrePass::None && transposed_store_callable(in, dtype, frames_addr, pitch_bytes);
    if (int rc = make_fused_launch(pl, fused_launch_inputs(in, kdt, d.need_minmax, d.frames_lo(), want_tro), &d.fused, why)) return rc;
  }
  d.transpose_pass = !cx && transposed && !d.fused.tro;   // (the complex call's D x H layout is made by its own entry point)

  // the acquisition configurations the reference ships: one wave per A-scan (fdoct_wave.hip) instead of one workgroup
  // (frames handed over as doubles carry a low word per sample: the fused any-option, workgroup-per-row and long-row kernels take it)
  const bool wave_scope = run_generic && !pl.gen.use_big && in.plan_override > -2 && kdt >= 0 && !d.frames_lo() &&
                          (kaddr % 4 == 0) && (kpitch % 4 == 0) && out_rows < 0x7fffffffLL;
  if (d.bin2_in_kernel && !wave_scope) return refuse(why, FDOCT_ERR_DEVICE, "internal: binning left to a kernel that does not run");
  bool run_wave = d.bin2_in_kernel;
  if (wave_scope && !run_wave) {
    const bool wave_builtin = wave_opt == 0 && wave_kernel_available(W, in.M, in.N, kdt, D);   // (never the complex call's: its option bit is set)
    // any other shape the template can take: compiled for this handle's geometry at run time (fdoct_set_jit); the first call
    // (or fdoct_prepare) pays the compile, a refusal falls back to the workgroup-per-row kernel
    if (!wave_builtin && in.jit && wave_jit_shape_ok(W, in.M, in.N, D, wave_opt) && can_compile(ctx, kdt, wave_opt)) {
      compiled = true;
      d.wave_opt = wave_opt;
    }
    run_wave = wave_builtin || compiled;
  }
  if (run_wave && !d.bin2_in_kernel) {  // (the kernel that bins is known to fit)
    d.tables |= TABLES_WAVE;
    WaveLaunch l;
    if (wave_launch(d.wave_opt, &l)) {
      take(l);
    } else {  // not even one wave's buffer next to the tables
      run_wave = false;
      compiled = false;
      d.wave_opt = 0;
    }
  }
  if (run_wave)
    d.family = compiled ? FDOCT_KERNEL_WAVE_JIT : FDOCT_KERNEL_WAVE;
  else if (run_generic) {
    d.family = pl.gen.use_big ? FDOCT_KERNEL_LONG_ROWS : FDOCT_KERNEL_GENERIC;
    if (!pl.gen.use_big) {
      d.lds = generic_lds_bytes(PlanInputs{W, in.M, in.N, D, in.phase, in.plan_override, in.force_general}, pl.gen);
      // generic_kernel is compiled for 6 waves per SIMD = 6 workgroups of 4 waves per CU
      const int per_cu = std::clamp((int)((160 * 1024 - 1024) / d.lds), 1, 6);
      d.grid = std::min<long long>((long long)in.num_cu * per_cu, out_rows);
    }
    // the cliff an integrator should see: rows in HBM run an order of magnitude below their LDS-resident neighbours
    if (pl.gen.use_big)
      d.note = "this geometry runs on the long-row path (rows in HBM, fdoct_big.hip: one launch per group of DFT passes): its transforms do not fit "
               "the 160 KB of LDS of a compute unit; expect 1e6 ... 1e7 A-scans/s where LDS-resident rows reach 1e8";
  }
  else
    d.family = in.staged ? FDOCT_KERNEL_FUSED_STAGED : (d.fused.tro ? FDOCT_KERNEL_FUSED_TRANSPOSED : FDOCT_KERNEL_FUSED);
  *out = d;
  return FDOCT_OK;
}

}  // namespace fdoct
