// Prints make_plan's decision (fdoct_amd/csrc/fdoct_plan.h) for a fixed grid of configurations, one line each: the fused plan
// and its geometry or the generic path, then the generic plan.  tests/test_abi.py compares the output with plan_check.expected,
// recorded from the planner as it was before it became a value.  Host-only: no GPU needed.
#include <cstdio>
#include <string>
#include <vector>

#include "fdoct_plan.h"

using namespace fdoct;

static std::string list(const std::vector<int>& v) {
  std::string s;
  for (int x : v) s += (s.empty() ? "" : ",") + std::to_string(x);
  return "[" + s + "]";
}

struct Shape {
  int W, M, N, D;
};

static const Shape kShapes[] = {
    // BASELINE C1, C2 (also C3 with the phase, and C5), C4
    {128, 1, 1024, 512}, {2048, 1, 2048, 1024}, {4096, 1, 4096, 2048},
    // the shipped ini files: 640 / 720 samples zero-padded x4 (2560 / 2880 points), 160 x4, 640 and 1280 unpadded
    {640, 4, 2560, 320}, {720, 4, 2880, 360}, {160, 4, 2560, 320}, {640, 1, 640, 320}, {1280, 1, 1280, 640},
    // fused-plan edges: 256- and 512-point rows, a width off the 8-sample grid, wider than the plan's chunks, display beyond N/2
    {256, 1, 256, 128}, {512, 1, 512, 256}, {2044, 1, 2048, 1024}, {3000, 1, 2048, 1024}, {2048, 1, 2048, 1500},
    // odd widths
    {321, 4, 2048, 512}, {101, 3, 1024, 256}, {99, 2, 512, 128},
    // prime factors above 5 (Bluestein), an odd length
    {640, 1, 1400, 320}, {512, 1, 1022, 256}, {640, 1, 16382, 320}, {208, 4, 2560, 320}, {640, 1, 1001, 320},
    // half lengths beyond 9000 points (one buffer in place, radix-16 passes)
    {2048, 1, 20000, 1000}, {4096, 1, 16384, 2048}, {4096, 8, 32768, 2048}, {1024, 16, 32768, 4096},
    // rows beyond the LDS (long-row path), and beyond what that path takes
    {4096, 1, 131072, 2048}, {8192, 4096, 1024, 512},
};

// one configuration's decision
static std::string describe(const PlanInputs& in) {
  Plan p;
  std::string why;
  if (int rc = make_plan(in, &p, &why)) return "rc=" + std::to_string(rc) + " " + why;
  char buf[256];
  if (p.fused)
    std::snprintf(buf, sizeof buf, "fused=%d split=%d scratch=%d tw=%d", p.fused->id, p.split, p.scratch_bytes, p.tw_count);
  else
    std::snprintf(buf, sizeof buf, "generic");
  std::string s = buf + std::string(" cplx=") + std::to_string(p.cplx) + " NC=" + std::to_string(p.NC) + " | ";
  const GenericPlan& g = p.gen;
  if (g.rc) return s + "generic rc=" + std::to_string(g.rc) + " " + g.why;
  s += "n=" + list(g.rad_n) + " nh=" + list(g.rad_nh) + " wh=" + list(g.rad_wh) + " mwh=" + list(g.rad_mwh) +
       " blu=" + std::to_string(g.blu_m) + list(g.rad_blu);
  if (g.zn)  // (the zero-pad stage at full length was considered)
    s += " zp_full=" + std::to_string(g.zp_full) + " zn=" + std::to_string(g.zn) + " zf=" + std::to_string(g.gzf.n) + "/" +
         std::to_string(g.gzf.blu_m) + list(g.gzf.rad) + " zi=" + std::to_string(g.gzi.n) + "/" + std::to_string(g.gzi.blu_m) +
         list(g.gzi.rad);
  return s + " inplace=" + std::to_string(g.inplace) + " radix16=" + std::to_string(g.radix16) + " big=" + std::to_string(g.use_big);
}

int main() {
  std::vector<int> overrides = {-1, -2, -3};
  for (int id = 0; id < 64; id++) {
    FusedPlan q{};
    if (fused_plan_get(id, &q)) overrides.push_back(id);
  }
  for (const Shape& s : kShapes)
    for (int phase = 0; phase < 2; phase++)
      for (int ov : overrides) {
        const std::string a = describe(PlanInputs{s.W, s.M, s.N, s.D, phase != 0, ov, false});
        const std::string b = describe(PlanInputs{s.W, s.M, s.N, s.D, phase != 0, ov, true});
        const std::string cfg = "W=" + std::to_string(s.W) + " M=" + std::to_string(s.M) + " N=" + std::to_string(s.N) + " D=" +
                                std::to_string(s.D) + " phase=" + std::to_string(phase) + " override=" + std::to_string(ov);
        if (a == b)
          std::printf("%s force_general=0,1: %s\n", cfg.c_str(), a.c_str());
        else
          std::printf("%s force_general=0: %s\n%s force_general=1: %s\n", cfg.c_str(), a.c_str(), cfg.c_str(), b.c_str());
      }
  return 0;
}
