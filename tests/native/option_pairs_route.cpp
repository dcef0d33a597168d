// Prints make_route's kernel family (fdoct_amd/csrc/fdoct_route_value.h) for every call of a file: one call per line as 29 integers,
// in the order of tests/option_pairs.py::route_line --
//   W M N D H A nframes dtype bg_rows pi dark bandpass rowwisenormalize normalize phase movavgn fe_median fe_bin jit staged
//   plan_override force_general precise_div grid_override frames_addr_offset pitch_bytes out_bscan_offset out_db_offset layout
// (an output offset of -1: that pointer is null) -- and answers one line each: the family's number (fdoct_kernel), " tr" where a
// transpose pass follows, " opt=<bits>" for the run-time compiled wave-per-row kernel; or "rc=<code> <text>" where plan or route
// refuse the call.  The run-time compiler answers yes.  tests/test_option_pairs.py holds the catalogue's expected kernels to it.
// Host-only: no GPU needed, no HIP call made.
#include <cstdio>
#include <string>

#include "fdoct_route_value.h"

using namespace fdoct;

static bool yes(void*, int, int) { return true; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  long long v[29];
  for (;;) {
    int got = 0;
    while (got < 29 && std::fscanf(f, "%lld", &v[got]) == 1) got++;
    if (got == 0) break;
    if (got != 29) return 3;
    RouteInputs in;
    in.W = (int)v[0]; in.M = (int)v[1]; in.N = (int)v[2]; in.D = (int)v[3]; in.H = (int)v[4]; in.A = (int)v[5]; in.nframes = (int)v[6];
    in.dtype = (int)v[7]; in.bg_rows = (int)v[8]; in.pi = v[9] != 0; in.dark = v[10] != 0; in.bandpass = v[11] != 0;
    in.rowwisenormalize = v[12] != 0; in.normalize = v[13] != 0; in.phase = v[14] != 0; in.movavgn = (int)v[15];
    in.fe_median = (int)v[16]; in.fe_binx = in.fe_biny = (int)v[17]; in.jit = v[18] != 0; in.staged = v[19] != 0;
    in.plan_override = (int)v[20]; in.force_general = v[21] != 0; in.precise_div = v[22] != 0; in.grid_override = (int)v[23];
    const uintptr_t base = (uintptr_t)0x7f0000000000ull;
    in.frames_addr = base + (uintptr_t)v[24];
    in.pitch_bytes = (size_t)v[25];
    in.out_bscan_addr = v[26] < 0 ? 0 : base + (uintptr_t)v[26];
    in.out_db_addr = v[27] < 0 ? 0 : base + (uintptr_t)v[27];
    in.layout = (int)v[28];
    Plan pl;
    std::string why;
    if (int rc = make_plan(PlanInputs{in.W, in.M, in.N, in.D, in.phase, in.plan_override, in.force_general}, &pl, &why)) {
      std::printf("rc=%d plan: %s\n", rc, why.c_str());
      continue;
    }
    in.plan = &pl;
    RouteDecision d;
    why.clear();
    if (int rc = make_route(in, yes, nullptr, &d, &why)) {
      std::printf("rc=%d %s\n", rc, why.c_str());
      continue;
    }
    std::printf("%d%s", d.family, d.transpose_pass ? " tr" : "");
    if (d.family == FDOCT_KERNEL_WAVE_JIT) std::printf(" opt=%d", d.wave_opt);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
