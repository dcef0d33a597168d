// Prints make_fused_launch's decision (fdoct_amd/csrc/fdoct_launch.h) for a fixed grid of handles and calls, one line each: every
// field of the launch value, or the refusal and its text.  tests/test_abi.py compares the output with launch_check.expected,
// recorded from the arithmetic as it stood in launch_family_fused and fused_transposed_store_applies before the launch became a
// value.  Host-only: no GPU needed.
#include <cstdio>
#include <string>

#include "fdoct_launch.h"

using namespace fdoct;

struct Shape {
  int W, M, N, D;
};

// every shape of plan_check.cpp that gets a fused plan, and C1 as stated (1024 samples -> 1024 points: the 512-point plan with
// 16 lanes per row, the one besides the row-swap plan that has the transposed store)
static const Shape kShapes[] = {
    {128, 1, 1024, 512}, {1024, 1, 1024, 512}, {2048, 1, 2048, 1024}, {4096, 1, 4096, 2048}, {256, 1, 256, 128},
    {512, 1, 512, 256},  {3000, 1, 2048, 1024}, {2048, 1, 2048, 1500},
};

enum Opt { PLAIN, PI, DARK, ROWNORM, FRAMENORM, LOW_WORDS, FORCE_GENERAL, STAGED, kOpts };
static const char* kOptNames[kOpts] = {"plain", "pi", "dark", "rownorm", "framenorm", "lo", "general", "staged"};
static const char* kTypeNames[3] = {"u8", "u16", "f32"};

static void apply(FusedLaunchInputs& in, int opt) {
  in.pi = opt == PI;
  in.dark = opt == DARK;
  in.rowwisenormalize = opt == ROWNORM;
  in.minmax = opt == FRAMENORM;
  in.frames_lo = opt == LOW_WORDS;
  in.force_general = opt == FORCE_GENERAL;
  in.staged = opt == STAGED;
}

static void rows(FusedLaunchInputs& in, int H, long long out_rows) {
  in.H = H;
  in.groups = (out_rows + H - 1) / H;
  in.out_rows = in.groups * H;
  in.in_rows = in.out_rows * in.A;
}

static void print(const Plan& pl, const FusedLaunchInputs& in, int opt) {
  // (inputs and outputs at their defaults are left out of the line)
  std::printf("H=%d D=%d A=%d %s bg=%d pd=%d %s rows=%lld", in.H, in.D, in.A, kTypeNames[in.kdt], in.bg_rows > 1 ? 2 : 1, in.precise_div ? 1 : 0,
              kOptNames[opt], in.out_rows);
  if (in.block_override || in.grid_override) std::printf(" set_launch=%d,%d", in.block_override, in.grid_override);
  if (in.want_tro) std::printf(" DxH");
  if (in.ring_cap) std::printf(" cap=%u", in.ring_cap);
  FusedLaunch l;
  std::string why;
  if (int rc = make_fused_launch(pl, in, &l, &why)) {
    std::printf(": rc=%d %s\n", rc, why.c_str());
    return;
  }
  std::printf(": lean=%d prec=%d planes=%d block=%d lds=%zu grid=%lld", l.lean ? 1 : 0, l.prec, l.lds_planes, l.block, l.lds, l.grid);
  if (in.staged) std::printf(" stage1=%lld", l.stage1_grid);
  if (l.tro)
    std::printf(" tro ring=%u tpf=%u magic=%u tiles=%u", l.tro->ring, l.tro->tpf, l.tro->tpf_magic, l.tro->total_tiles);
  else if (in.want_tro)
    std::printf(" tro none");
  std::printf("\n");
}

// one line: the base call with these few fields changed
struct Case {
  int A = 1, kdt = FDOCT_K_U16;
  bool full_bg = false, precise = true;
  int opt = PLAIN, block = 0, grid = 0;
  long long out_rows = 262000;
};

int main() {
  for (const Shape& s : kShapes)
    for (int phase = 0; phase < 2; phase++) {
      Plan pl;
      std::string why;
      if (make_plan(PlanInputs{s.W, s.M, s.N, s.D, phase != 0, -1, false}, &pl, &why) || !pl.fused) continue;
      const FusedPlan& p = *pl.fused;
      std::printf("# W=%d N=%d D=%d phase=%d: plan %d kind %d T %d WCH %d NC %d scratch %d\n", s.W, s.N, s.D, phase, p.id, p.kind, p.T,
                  p.WCH, pl.NC, pl.scratch_bytes);
      auto run = [&](const Case& c, int H, int D, bool want_tro, unsigned cap) {
        FusedLaunchInputs in;
        in.W = s.W;
        in.D = D;
        in.A = c.A;
        in.kdt = c.kdt;
        in.bg_rows = c.full_bg ? H : 1;
        in.precise_div = c.precise;
        in.block_override = c.block;
        in.grid_override = c.grid;
        in.want_tro = want_tro;
        in.ring_cap = cap;
        apply(in, c.opt);
        rows(in, H, c.out_rows);
        print(pl, in, c.opt);
      };
      // every option of handle and call on its own, those that averaging bears on with it too; then sample type x background x
      // form of the division
      for (int opt = 0; opt < kOpts; opt++) run(Case{1, FDOCT_K_U16, false, true, opt}, 8, s.D, false, 0);
      for (int opt : {PLAIN, FRAMENORM, LOW_WORDS, STAGED}) run(Case{16, FDOCT_K_U16, false, true, opt}, 8, s.D, false, 0);
      for (int kdt : {FDOCT_K_U8, FDOCT_K_U16, FDOCT_K_F32})
        for (bool full_bg : {false, true})
          for (bool precise : {true, false})
            if (kdt != FDOCT_K_U16 || full_bg || !precise) run(Case{1, kdt, full_bg, precise}, 8, s.D, false, 0);
      // launch overrides on many rows and on few
      static const Case kOverrides[] = {
          {1, FDOCT_K_U16, false, true, PLAIN, 128, 0},         {1, FDOCT_K_U16, false, true, PLAIN, 192, 0},
          {1, FDOCT_K_U16, false, true, PLAIN, 256, 0},         {1, FDOCT_K_U16, false, true, PLAIN, 512, 0},
          {1, FDOCT_K_U16, false, true, PLAIN, 0, 1},           {1, FDOCT_K_U16, false, true, PLAIN, 0, 2},
          {1, FDOCT_K_U16, false, true, PLAIN, 192, 2},         {1, FDOCT_K_U16, false, true, PLAIN, 0, 0, 8},
          {1, FDOCT_K_U16, false, true, PLAIN, 512, 1, 8},      {16, FDOCT_K_U16, false, true, PLAIN, 128, 2},
          {1, FDOCT_K_U16, false, true, FORCE_GENERAL, 256, 1}, {16, FDOCT_K_U16, false, true, STAGED, 192, 2, 8},
      };
      for (const Case& c : kOverrides) run(c, 8, s.D, false, 0);
      // the transposed store: asked for on every plan, in full where the plan has it -- plain, 8-bit frames normalised with one
      // word of the reciprocal, full-frame background, averaging
      if (!(fused_tro_compiled(p.kind, p.T, p.WCH) && !pl.cplx && s.W == 8 * p.T * p.WCH)) {
        run(Case{}, 500, 512, true, 0);
        continue;
      }
      static const Case kStores[] = {{}, {1, FDOCT_K_U8, false, false, FRAMENORM}, {1, FDOCT_K_U16, true}, {16}};
      for (int H : {8, 500, 1000})
        for (int D : {256, 512, 1024})
          for (Case c : kStores) {
            c.out_rows = H == 8 ? 8 : 262000;
            run(c, H, D, true, 0);
            // ... with launch overrides (two, three, four, eight waves; one and two workgroups) and the ring cap
            if (H != 500 || (D != 1024 && (c.A > 1 || c.kdt == FDOCT_K_U8))) continue;
            for (int block : {128, 192, 256, 512}) c.block = block, run(c, H, D, true, 0);
            run(c, H, D, true, 20);
            c.block = 0, run(c, H, D, true, 20);
            c.grid = 1, run(c, H, D, true, 0);
            c.block = 192, c.grid = 2, run(c, H, D, true, 0);
          }
      // ... and what rules it out there: every other option, float frames, rows not in fours, bins not in whole write-out steps
      for (int opt = PI; opt < kOpts; opt++) run(Case{1, FDOCT_K_U16, false, true, opt, 0, 0, 32}, 8, 512, true, 0);
      run(Case{1, FDOCT_K_F32, false, true, PLAIN, 0, 0, 32}, 8, 512, true, 0);
      run(Case{1, FDOCT_K_U16, false, true, PLAIN, 0, 0, 24}, 6, 512, true, 0);
      run(Case{1, FDOCT_K_U16, false, true, PLAIN, 0, 0, 32}, 8, 500, true, 0);
    }
  return 0;
}
