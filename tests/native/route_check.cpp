// Prints make_route's decision (fdoct_amd/csrc/fdoct_route_value.h) for a fixed grid of handles and calls, one line each: the
// inputs that differ from the base call, then the decision -- family, the passes in front of the chain, what the kernel reads, the
// fields that reach the family's launch (waves / LDS / grid of the wave-per-row and workgroup-per-row families, the whole fused
// launch), the table sets, whether the decision leaves a note, and every question put to the run-time compiler with its answer --
// or the refusal and its text.  tests/test_abi.py compares the output with route_check.expected, recorded from the arithmetic moved
// as it stood in choose_route_of before the route became a value.  Host-only: no GPU needed, no HIP call made.
//
// The base call of a shape: H = 500, 524 B-scans (262 000 A-scans), averages 1, packed 16-bit frames at an aligned address, no
// normalisation, row-major outputs, the compiler answering yes.  Every option is applied to it on its own; where a line asked the
// compiler, the line is repeated with the compiler answering no; every line the complex call takes (averages 1) is repeated as the
// complex call.  In full that is done on a fused, a built-in wave and an off-list shape (the complex call on the built-in one); the
// other shapes, and the complex call elsewhere, take the options whose route or launch figures depend on the shape.  Refusals: every text of make_route
// appears, and where two could apply one line sets both triggers.  (Not reachable from any inputs, hence not here: "internal:
// binning left to a kernel that does not run".)  The EXTRA, Bluestein and long-row shapes also take f64, moving average, median, colour,
// misaligned frames, staged mode, plan -2 and jit off.
#include <cstdio>
#include <string>
#include <vector>

#include "fdoct_route_value.h"

using namespace fdoct;

struct Shape {
  int W, M, N, D;
  const char* what;
};

// plan_check.cpp's shapes of each kind, C1 as stated, and the in-kernel binning's u8 edge (W = 320 takes it, wider rows do not)
static const Shape kShapes[] = {
    {1024, 1, 1024, 512, "fused"},          {2048, 1, 2048, 1024, "fused"},       {160, 4, 2560, 320, "wave built-in"},
    {640, 4, 2560, 320, "wave built-in"},   {720, 4, 2880, 360, "wave built-in"}, {640, 1, 640, 320, "wave built-in"},
    {192, 4, 2560, 320, "wave EXTRA"},      {1280, 1, 1280, 640, "smooth, off both lists"},
    {321, 4, 2048, 512, "odd width"},       {640, 1, 1400, 320, "Bluestein"},     {4096, 1, 131072, 2048, "long rows"},
};
static const Shape kBinEdges[] = {{320, 4, 2560, 320, "wave built-in"}, {336, 4, 2560, 320, "not smooth"}, {384, 4, 2560, 320, "wave EXTRA"}};

struct Case {
  RouteInputs in;
  std::string label;
  bool phase = false, deep = false, pitch_set = false, stub_yes = true, bad_generic = false;
  bool narrow = false;  // an option that only passes through to the launch, or repeats its neighbour's path: on one fused and one wave shape
  bool core = false;    // an option whose waves / LDS / grid differ from shape to shape: on every shape, the others on one shape of each kind
  bool mid = false;     // an option that changes the route of the EXTRA, Bluestein and long-row shapes too: on those as well
  int D = 0;  // 0: the shape's
};

struct Stub {
  bool yes;
  std::string asked;
  static bool can_compile(void* p, int kdt, int opt) {
    Stub& s = *static_cast<Stub*>(p);
    s.asked += " ask(k" + std::to_string(kdt) + ",o" + std::to_string(opt) + ")=" + (s.yes ? "1" : "0");
    return s.yes;
  }
};

static const char* family_name(int f) {
  switch (f) {
    case FDOCT_KERNEL_FUSED: return "fused";
    case FDOCT_KERNEL_FUSED_STAGED: return "fused_staged";
    case FDOCT_KERNEL_FUSED_TRANSPOSED: return "fused_transposed";
    case FDOCT_KERNEL_GENERIC: return "generic";
    case FDOCT_KERNEL_WAVE: return "wave";
    case FDOCT_KERNEL_WAVE_JIT: return "wave_jit";
    case FDOCT_KERNEL_LONG_ROWS: return "long_rows";
    default: return "none";
  }
}

// One line.  Returns whether the compiler was asked.
static bool run(const Shape& s, Case c) {
  RouteInputs& in = c.in;
  in.W = s.W; in.M = s.M; in.N = s.N;
  in.D = c.D ? c.D : c.deep ? s.N / 2 + s.N / 8 : s.D;
  in.phase = c.phase;
  if (!c.pitch_set) in.pitch_bytes = (in.colour >= 0 && in.dtype == FDOCT_U8 ? 3 : dtype_size(in.dtype)) * (size_t)in.W * in.fe_binx;
  std::printf("%d:", s.W);  // (the shape is in the header line above; D only where the case changes it)
  if (in.D != s.D) std::printf(" D=%d", in.D);
  std::printf("%s%s%s:", c.label.c_str(), in.cx ? " cx" : "", c.stub_yes ? "" : " compiler=no");
  Plan pl;
  std::string why;
  if (int rc = make_plan(PlanInputs{in.W, in.M, in.N, in.D > in.N ? in.N : in.D, in.phase, in.plan_override, in.force_general}, &pl, &why)) {
    std::printf(" no plan: rc=%d %s\n", rc, why.c_str());
    return false;
  }
  if (c.bad_generic) pl.gen.rc = FDOCT_ERR_UNSUPPORTED, pl.gen.why = "rows of more than 2^24 points";  // (no shape has a fused plan AND this: set by hand)
  in.plan = &pl;
  Stub stub{c.stub_yes, {}};
  RouteDecision d;
  why.clear();
  if (int rc = make_route(in, Stub::can_compile, &stub, &d, &why)) {
    std::printf(" rc=%d %s |%s\n", rc, why.c_str(), stub.asked.c_str());
    return !stub.asked.empty();
  }
  if (!why.empty()) std::printf(" WHY-WRITTEN-ON-SUCCESS");
  // (flags only where set: fe front end, col colour stage, pre the pre-pass, mm min/max pass, tr transpose pass, bin2 binning in the kernel)
  std::printf(" %s%s%s", family_name(d.family), d.frontend ? " fe" : "", d.colour ? " col" : "");
  if (d.pre != PrePass::None) std::printf(" pre=%d", (int)d.pre);
  std::printf(" kdt=%d kpitch=%zu%s%s%s", d.kdt, d.kpitch, d.need_minmax ? " mm" : "", d.transpose_pass ? " tr" : "", d.bin2_in_kernel ? " bin2" : "");
  switch (d.family) {
    case FDOCT_KERNEL_WAVE_JIT: std::printf(" opt=%d", d.wave_opt);  // fall through
    case FDOCT_KERNEL_WAVE: std::printf(" waves=%d lds=%zu grid=%lld", d.waves, d.lds, d.grid); break;
    case FDOCT_KERNEL_GENERIC: std::printf(" lds=%zu grid=%lld", d.lds, d.grid); break;
    case FDOCT_KERNEL_LONG_ROWS: break;
    default: {
      const FusedLaunch& l = d.fused;
      std::printf(" lean=%d prec=%d planes=%d block=%d lds=%zu grid=%lld", l.lean ? 1 : 0, l.prec, l.lds_planes, l.block, l.lds, l.grid);
      if (in.staged) std::printf(" stage1=%lld", l.stage1_grid);
      if (l.tro) std::printf(" tro ring=%u tpf=%u magic=%u tiles=%u", l.tro->ring, l.tro->tpf, l.tro->tpf_magic, l.tro->total_tiles);
    }
  }
  std::printf(" tables=%u%s |%s\n", d.tables, d.note ? " note" : "", stub.asked.c_str());
  return !stub.asked.empty();
}

// the line; with the compiler answering no where it was asked; and both again as the complex call where that call is taken
static const struct Case* base_case = nullptr;  // the options' first: the base call
static void lines(const Shape& s, const Case& c, bool with_cx = true) {
  for (int cx = 0; cx < (with_cx ? 2 : 1); cx++) {
    Case k = c;
    k.in.cx = cx != 0;
    if (cx && (k.in.A != 1 || k.in.layout != FDOCT_LAYOUT_ROWMAJOR_HxD || k.in.out_bscan_addr || k.in.out_db_addr)) continue;  // (not the complex call's to set)
    if (!run(s, k) || (cx && &c != base_case)) continue;
    k.stub_yes = false;
    run(s, k);
  }
}

static Case base() {
  Case c;
  RouteInputs& in = c.in;
  in.H = 500; in.A = 1; in.nframes = 524;
  in.dtype = FDOCT_U16;
  in.frames_addr = (uintptr_t)0x7f0000000000ull;
  in.out_bscan_addr = in.out_db_addr = 0;
  return c;
}

template <typename F>
static Case with(const char* label, F f, Case c = base()) {
  c.label += std::string(" ") + label;
  f(c);
  return c;
}

static std::vector<Case> options() {
  std::vector<Case> v;
  auto add = [&](const char* label, auto f) { v.push_back(with(label, f)); };
  auto narrow = [&](const char* label, auto f) { v.push_back(with(label, f)), v.back().narrow = true; };
  auto mid = [&](const char* label, auto f) { v.push_back(with(label, f)), v.back().mid = true; };
  auto core = [&](const char* label, auto f) { v.push_back(with(label, f)), v.back().core = true; };
  auto dt = [](int d) { return [d](Case& c) { c.in.dtype = d; }; };
  core("base", [](Case&) {});
  core("u8", dt(FDOCT_U8));
  core("f32", dt(FDOCT_F32));
  mid("f64", dt(FDOCT_F64));
  add("pi", [](Case& c) { c.in.pi = true; });
  add("dark", [](Case& c) { c.in.dark = true; });
  add("bandpass", [](Case& c) { c.in.bandpass = true; });
  add("rownorm", [](Case& c) { c.in.rowwisenormalize = true; });
  add("framenorm", [](Case& c) { c.in.normalize = true; });
  narrow("rownorm+normalize", [](Case& c) { c.in.rowwisenormalize = c.in.normalize = true; });
  core("phase", [](Case& c) { c.phase = true; });
  core("deep", [](Case& c) { c.deep = true; });
  core("bg=2d", [](Case& c) { c.in.bg_rows = c.in.H; });
  // the moving average with each sample type; float frames off the 4-byte grid
  for (int d : {FDOCT_U8, FDOCT_U16, FDOCT_F32, FDOCT_F64}) {
    static const char* n[] = {"movavg u8", "movavg u16", "movavg f32", "movavg f64"};
    d == FDOCT_U16 || d == FDOCT_F64 ? mid(n[d], [d](Case& c) { c.in.movavgn = 5, c.in.dtype = d; }) : add(n[d], [d](Case& c) { c.in.movavgn = 5, c.in.dtype = d; });
  }
  add("movavg f32 addr+2", [](Case& c) { c.in.movavgn = 5, c.in.dtype = FDOCT_F32, c.in.frames_addr += 2; });
  add("movavg f32 pitch+2", [](Case& c) { c.in.movavgn = 5, c.in.dtype = FDOCT_F32, c.in.pitch_bytes = 4 * (size_t)8192 * 16 + 2, c.pitch_set = true; });
  // the front end: median and binning
  mid("median3", [](Case& c) { c.in.fe_median = 3; });
  add("median7 u8", [](Case& c) { c.in.fe_median = 7, c.in.dtype = FDOCT_U8; });
  core("bin2x2", [](Case& c) { c.in.fe_binx = c.in.fe_biny = 2; });
  add("bin2x2 u8", [](Case& c) { c.in.fe_binx = c.in.fe_biny = 2, c.in.dtype = FDOCT_U8; });
  add("bin2x2 framenorm", [](Case& c) { c.in.fe_binx = c.in.fe_biny = 2, c.in.normalize = true; });
  add("bin2x2 median3", [](Case& c) { c.in.fe_binx = c.in.fe_biny = 2, c.in.fe_median = 3; });
  narrow("bin2x2 jit=0", [](Case& c) { c.in.fe_binx = c.in.fe_biny = 2, c.in.jit = false; });
  add("bin4x4", [](Case& c) { c.in.fe_binx = c.in.fe_biny = 4; });
  add("bin2x2 f32", [](Case& c) { c.in.fe_binx = c.in.fe_biny = 2, c.in.dtype = FDOCT_F32; });
  // colour frames
  for (int ch = 0; ch < 4; ch++) {
    static const char* n[] = {"colour0", "colour1", "colour2", "colour3"};
    static const char* nm[] = {"colour0 median3", "colour1 median3", "colour2 median3", "colour3 median3"};
    auto put = [&](const char* label, auto f) { ch == 1 || ch == 2 ? narrow(label, f) : mid(label, f); };  // (a channel is a channel)
    put(n[ch], [ch](Case& c) { c.in.colour = ch, c.in.dtype = FDOCT_U8; });
    put(nm[ch], [ch](Case& c) { c.in.colour = ch, c.in.dtype = FDOCT_U8, c.in.fe_median = 3; });
  }
  add("colour1 bin2x2", [](Case& c) { c.in.colour = 1, c.in.dtype = FDOCT_U8, c.in.fe_binx = c.in.fe_biny = 2; });
  // addresses and pitches off the vector grids
  mid("addr+2", [](Case& c) { c.in.frames_addr += 2; });
  add("addr+4", [](Case& c) { c.in.frames_addr += 4; });
  narrow("u8 addr+8", [](Case& c) { c.in.dtype = FDOCT_U8, c.in.frames_addr += 8; });
  add("pitch+4", [](Case& c) { c.in.pitch_bytes = 2 * (size_t)8192 * 16 + 4, c.pitch_set = true; });
  add("pitch+2", [](Case& c) { c.in.pitch_bytes = 2 * (size_t)8192 * 16 + 2, c.pitch_set = true; });
  // layouts and outputs
  core("DxH", [](Case& c) { c.in.layout = FDOCT_LAYOUT_TRANSPOSED_DxH; });
  add("DxH out+4", [](Case& c) { c.in.layout = FDOCT_LAYOUT_TRANSPOSED_DxH, c.in.out_db_addr = 4; });
  narrow("DxH tro=0", [](Case& c) { c.in.layout = FDOCT_LAYOUT_TRANSPOSED_DxH, c.in.tro_enabled = false; });
  narrow("out+4", [](Case& c) { c.in.out_bscan_addr = 4; });
  // switches and overrides
  mid("staged", [](Case& c) { c.in.staged = true; });
  mid("plan=-2", [](Case& c) { c.in.plan_override = -2; });
  narrow("general", [](Case& c) { c.in.force_general = true; });
  narrow("precise=0", [](Case& c) { c.in.precise_div = false; });
  core("block=64", [](Case& c) { c.in.block_override = 64; });
  add("block=256", [](Case& c) { c.in.block_override = 256; });
  core("block=2048", [](Case& c) { c.in.block_override = 2048; });
  add("grid=4", [](Case& c) { c.in.grid_override = 4; });
  add("grid=100000", [](Case& c) { c.in.grid_override = 100000; });
  narrow("cus=64", [](Case& c) { c.in.num_cu = 64; });
  add("A=16", [](Case& c) { c.in.A = 16, c.in.nframes = 524 * 16; });
  core("one B-scan", [](Case& c) { c.in.H = 8, c.in.nframes = 1; });
  narrow("one B-scan A=16", [](Case& c) { c.in.H = 8, c.in.A = 16, c.in.nframes = 16; });
  mid("jit=0", [](Case& c) { c.in.jit = false; });
  return v;
}

int main() {
  const std::vector<Case> opts = options();
  base_case = &opts[0];
  for (size_t i = 0; i < sizeof kShapes / sizeof *kShapes; i++) {
    const Shape& s = kShapes[i];
    std::printf("# %d x%d -> %d, %d deep: %s\n", s.W, s.M, s.N, s.D, s.what);
    const bool full = i == 0 || i == 3 || i == 7, cx_in_full = i == 3;
    for (const Case& c : opts)
      if (c.core || (c.mid && (i == 6 || i == 9 || i == 10)) || (full && (!c.narrow || i == 0 || i == 3))) lines(s, c, cx_in_full || (full && c.core) || &c == &opts[0]);
  }
  std::printf("# the in-kernel binning's edges\n");
  for (const Shape& s : kBinEdges)
    for (const Case& c : opts)
      if (c.in.fe_binx == 2 && c.in.colour < 0 && c.in.fe_median == 0 && c.in.jit && c.in.dtype != FDOCT_F32) lines(s, c, false);

  std::printf("# refusals, in their order of precedence: each alone, then with the next ones' triggers set too\n");
  const Shape fused = kShapes[0], wave = kShapes[3], big = kShapes[10];
  // (as the complex call too where that call's own refusals and checks come into it: the first five)
  int nth = 0;
  auto one = [&](const Shape& s, const char* label, auto f) { lines(s, with(label, f), nth++ < 5); };
  auto small_pitch = [](Case& c) { c.in.pitch_bytes = 64, c.pitch_set = true; };
  one(big, "base", [](Case&) {});                                                         // the complex call on long rows
  one(big, "D>N", [](Case& c) { c.D = 200000; });                                         // ... wins over D > N
  one(fused, "generic-refused", [](Case& c) { c.bad_generic = true; });                   // a refused generic plan: the complex call, not the fused one
  one(wave, "generic-refused", [](Case& c) { c.bad_generic = true; });
  one(wave, "generic-refused D>N", [](Case& c) { c.bad_generic = true, c.D = 4000; });
  one(fused, "D>N", [](Case& c) { c.D = 2000; });
  one(wave, "D>N", [](Case& c) { c.D = 4000; });
  one(wave, "D>N colour7", [](Case& c) { c.D = 4000, c.in.colour = 7, c.in.dtype = FDOCT_U8; });
  one(wave, "colour7", [](Case& c) { c.in.colour = 7, c.in.dtype = FDOCT_U8; });
  one(wave, "colour7 u16 median4", [](Case& c) { c.in.colour = 7, c.in.fe_median = 4; });
  one(wave, "colour1 u16", [](Case& c) { c.in.colour = 1; });
  one(wave, "colour1 u16 median4", [](Case& c) { c.in.colour = 1, c.in.fe_median = 4; });
  one(wave, "colour1 median4", [](Case& c) { c.in.colour = 1, c.in.dtype = FDOCT_U8, c.in.fe_median = 4; });
  one(wave, "colour3 median4", [](Case& c) { c.in.colour = 3, c.in.dtype = FDOCT_U8, c.in.fe_median = 4; });
  one(wave, "colour1 u16 pitch=64", [&](Case& c) { c.in.colour = 1, small_pitch(c); });
  one(wave, "colour3 median3 pitch=64", [&](Case& c) { c.in.colour = 3, c.in.dtype = FDOCT_U8, c.in.fe_median = 3, small_pitch(c); });
  one(wave, "colour1 pitch=64", [&](Case& c) { c.in.colour = 1, c.in.dtype = FDOCT_U8, small_pitch(c); });
  one(wave, "colour3 pitch=64", [&](Case& c) { c.in.colour = 3, c.in.dtype = FDOCT_U8, small_pitch(c); });
  one(wave, "colour1 pitch=64 staged", [&](Case& c) { c.in.colour = 1, c.in.dtype = FDOCT_U8, c.in.staged = true, small_pitch(c); });
  one(wave, "median3 f32 pitch=64", [&](Case& c) { c.in.fe_median = 3, c.in.dtype = FDOCT_F32, small_pitch(c); });
  one(wave, "median3 f64 pitch=68", [](Case& c) { c.in.fe_median = 3, c.in.dtype = FDOCT_F64, c.in.pitch_bytes = 68, c.pitch_set = true; });
  one(wave, "D>N bin2x2 f32", [](Case& c) { c.D = 4000, c.in.fe_binx = c.in.fe_biny = 2, c.in.dtype = FDOCT_F32; });
  one(wave, "bin2x2 pitch=64", [&](Case& c) { c.in.fe_binx = c.in.fe_biny = 2, small_pitch(c); });
  one(wave, "bin4x4 pitch=64 staged", [&](Case& c) { c.in.fe_binx = c.in.fe_biny = 4, c.in.staged = true, small_pitch(c); });
  one(wave, "f64 pitch+4", [](Case& c) { c.in.dtype = FDOCT_F64, c.in.pitch_bytes = 8 * 640 + 4, c.pitch_set = true; });
  one(fused, "f64 pitch+4 staged", [](Case& c) { c.in.dtype = FDOCT_F64, c.in.staged = true, c.in.pitch_bytes = 8 * 1024 + 4, c.pitch_set = true; });
  one(fused, "f64 pitch+4 addr+2 generic-refused", [](Case& c) { c.in.dtype = FDOCT_F64, c.bad_generic = true, c.in.frames_addr += 2, c.in.pitch_bytes = 8 * 1024 + 4, c.pitch_set = true; });
  one(fused, "addr+2 generic-refused", [](Case& c) { c.bad_generic = true, c.in.frames_addr += 2; });
  one(fused, "addr+2 generic-refused staged", [](Case& c) { c.bad_generic = true, c.in.staged = true, c.in.frames_addr += 2; });
  one(fused, "addr+2 staged", [](Case& c) { c.in.staged = true, c.in.frames_addr += 2; });
  one(fused, "addr+2 staged u8", [](Case& c) { c.in.staged = true, c.in.dtype = FDOCT_U8, c.in.frames_addr += 2; });   // ... wins over the launch's refusal
  one(wave, "staged", [](Case& c) { c.in.staged = true; });
  one(fused, "staged u8", [](Case& c) { c.in.staged = true, c.in.dtype = FDOCT_U8; });                                  // make_fused_launch's refusals pass through
  one(fused, "staged framenorm", [](Case& c) { c.in.staged = true, c.in.normalize = true; });
  one(fused, "staged bg=2d", [](Case& c) { c.in.staged = true, c.in.bg_rows = c.in.H; });
  // a 2-3-5-smooth half length of 13 passes (5^11 x 18), more than a WavePlan holds: no wave kernel can exist for it, so nothing may
  // hand it to wave_plan on the way to the planner's refusal (this program runs under -fsanitize=address,undefined in review)
  std::printf("# lengths beyond every wave kernel\n");
  run(Shape{8, 1, 1757812500, 1, ""}, with("base", [](Case&) {}));
  static_assert(wave_tw_layout(8, 1, 1757812500, 1, false).count == 0 && wave_tw_layout(640, 4, 2560, 320, false).count > 0, "");
  return 0;
}
