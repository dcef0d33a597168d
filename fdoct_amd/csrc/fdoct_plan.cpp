// fdoct_plan.cpp -- make_plan (fdoct_plan.h): which kernel family takes a configuration, and with what geometry.
#include "fdoct_plan.h"

#include <algorithm>
#include <cstdlib>
#include <iterator>

#include "../../include/fdoct.h"

namespace fdoct {

namespace {

bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

// n = 2^a 3^b 5^c -> Stockham radices (4s first), false if another prime divides n
// Radix plan of the generic kernel's Stockham DFT (radices 16/8/4/2/5/3).  The first pass writes butterfly j's
// outputs R apart (stride R*8 bytes across lanes), so it gets an odd radix -- or a small power of two -- to keep
// those LDS writes off the same banks; it is also the pass without twiddle multiplies.
bool factor_radices(int n, std::vector<int>& rad, int log2max = 0) {
  rad.clear();
  int a = 0, b = 0, c = 0;
  while (n % 2 == 0) { a++; n /= 2; }
  while (n % 3 == 0) { b++; n /= 3; }
  while (n % 5 == 0) { c++; n /= 5; }
  if (n != 1) return false;
  for (int i = 0; i < c; i++) rad.push_back(5);
  for (int i = 0; i < b; i++) rad.push_back(3);
  if (rad.empty() && a > 0) {
    const int first = (a % 2) ? 1 : 2;
    rad.push_back(1 << first);
    a -= first;
  }
  const int kLog2Max = log2max ? log2max : (GENERIC_MAX_RADIX >= 16 ? 4 : 3);
  for (; a >= kLog2Max; a -= kLog2Max) rad.push_back(1 << kLog2Max);
  if (a) rad.push_back(1 << a);
  return (int)rad.size() <= GENERIC_MAX_PASSES;
}

// the pass plans again with radix-16 butterflies (the 1024-thread kernels)
void use_radix16(const PlanInputs& in, GenericPlan& g) {
  if (!g.rad_n.empty()) factor_radices(in.N, g.rad_n, 4);
  if (!g.rad_nh.empty()) factor_radices(in.N / 2, g.rad_nh, 4);
  if (in.M > 1) {
    factor_radices(in.W / 2, g.rad_wh, 4);
    factor_radices(in.W * in.M / 2, g.rad_mwh, 4);
  }
}

// The any-configuration path: checks that fdoct_generic.hip (or, with the rows in HBM, fdoct_big.hip) can run this geometry.
int plan_generic(const PlanInputs& in, GenericPlan& g, std::string* why) {
  const int W = in.W, M = in.M, N = in.N, MW = W * M;
  // cv::dft takes any length (main:1185).  Lengths with prime factors up to 5 run as mixed-radix Stockham passes; any
  // other length as Bluestein's algorithm: two power-of-two DFTs of length >= 2n - 1 around a chirp multiplication.
  const int tlen = generic_real_half(in) ? N / 2 : N;  // the transform the kernel actually runs
  std::vector<int> probe;
  if (!factor_radices(tlen, probe)) {
    int mb = 1;
    while (mb < 2 * tlen - 1) mb <<= 1;
    // (round 6: the smallest length 2^a 3^b 5^c >= 2n - 1 where the host can afford the transformed chirp by the DFT's definition:
    // 1296 instead of 2048 around a 642-point transform)
    if (2 * tlen - 1 <= 8192) {
      for (int c = 2 * tlen - 1; c < mb; c++) {
        int m = c;
        for (int f : {2, 3, 5})
          while (m % f == 0) m /= f;
        std::vector<int> tmp;
        if (m == 1 && factor_radices(c, tmp)) {
          mb = c;
          break;
        }
      }
    }
    g.blu_m = mb;
    factor_radices(mb, g.rad_blu);
  } else {
    if (!factor_radices(N, g.rad_n)) g.rad_n.clear();  // (only used when the full-length transform runs)
    if ((N % 2) == 0 && !factor_radices(N / 2, g.rad_nh)) g.rad_nh.clear();
  }
  // an odd width (the reference's fftshift leaves the last column of the spectrum where it is and, under an even multiplier,
  // pads to M W - 1 bins, main:215-241) and zero-pad lengths with a prime factor above 5: the long-row path, whose DFTs run at
  // full length and take any length (the LDS kernels halve the transforms of a real row, which needs an even width)
  if (M > 1 && ((W % 2) || !factor_radices(W / 2, g.rad_wh) || !factor_radices(MW / 2, g.rad_mwh))) {
    g.rad_wh.clear();
    g.rad_mwh.clear();
    // Round 6: such a row stays in LDS when two buffers of its full-length transforms fit -- the W-point and the padded
    // spectrum's zn-point +i transforms inside generic_kernel (Stockham passes, or Bluestein around a power of two: 321 x 4 ->
    // 1283 points, a prime, runs around 4096) -- and leaves for HBM only when they do not.
    g.zn = W + 2 * ((MW - W) / 2);
    auto plan = [](int n, GenericDftPlan& p) {
      p.n = n;
      if (!factor_radices(n, p.rad)) {
        // Bluestein around the smallest length 2^a 3^b 5^c >= 2n - 1 (the convolution only needs that much room; the passes
        // take radices 2, 3, 4, 5, 8): 2592 for a 1283-point transform where the next power of two is 4096
        int mb = 2 * n - 1;
        for (;; mb++) {
          int m = mb;
          for (int f : {2, 3, 5})
            while (m % f == 0) m /= f;
          if (m == 1 && factor_radices(mb, p.rad)) break;
          if (mb > 4 * n) return false;
        }
        p.blu_m = mb;
        return mb <= 8192;   // (the host builds the transformed chirp by the DFT's definition: bounded work)
      }
      return true;
    };
    g.zp_full = plan(W, g.gzf) && plan(g.zn, g.gzi);
    if (g.zp_full && generic_lds_bytes(in, g, 2) + 1024 > 160 * 1024) g.zp_full = false;
    static const bool no_full = [] { const char* e = std::getenv("FDOCT_NO_ZP_FULL"); return e && std::atoi(e) != 0; }();  // measurement: round 5's route
    if (no_full) g.zp_full = false;
    if (!g.zp_full) g.use_big = true;
  }
  // rows whose two DFT buffers do not fit the 160 KB of LDS (half-length transforms beyond about 9000 points): with ONE buffer and
  // every step in place (generic_kernel<1024, 1, true>) up to 16384 points -- 4096 samples upsampled x8 -- as long as a thread of
  // the 1024 holds its share of a pass in 16 registers (radices 5 / 3: 15), the zero-pad spectrum in 8 and the resampled row
  // in 32, and the length needs no Bluestein; what lies beyond runs with the rows in HBM (fdoct_big.hip)
  // (FDOCT_GENERIC_INPLACE_ABOVE: the two-buffer footprint above which the one-buffer kernel is taken, for measurements)
  static const size_t inplace_above = [] { const char* e = std::getenv("FDOCT_GENERIC_INPLACE_ABOVE"); return e ? (size_t)std::atol(e) : (size_t)160 * 1024; }();
  const bool must_inplace = generic_lds_bytes(in, g, 2) + 1024 > 160 * 1024;
  if (!g.zp_full && generic_lds_bytes(in, g, 2) + 1024 > inplace_above) {
    auto pass_ok = [](const std::vector<int>& rad, int n) {
      for (int R : rad)
        if (R > 16 || n / R > 1024 * (16 / R)) return false;
      return !rad.empty();
    };
    // (the in-place passes take radix-16 butterflies -- one per thread on a 16384-point transform -- and with them a pass less)
    GenericPlan r16 = g;
    use_radix16(in, r16);
    const bool ok = !g.use_big && !g.blu_m && generic_lds_bytes(in, g, 1) + 1024 <= 160 * 1024 && N <= 32 * 1024 &&
                    (generic_real_half(in) ? pass_ok(r16.rad_nh, N / 2) : pass_ok(r16.rad_n, N)) &&
                    (M == 1 || (W / 2 <= 8 * 1024 && pass_ok(r16.rad_wh, W / 2) && pass_ok(r16.rad_mwh, MW / 2)));
    if (ok) {
      g = std::move(r16);
      g.inplace = true;
    } else if (must_inplace) {
      g.use_big = true;
    }
  }
  // rows of which a CU holds one (two buffers beyond half the LDS) run with 1024 threads, 128 registers each: radix-16 passes there too
  g.radix16 = g.inplace;
  static const int r16 = [] { const char* e = std::getenv("FDOCT_GENERIC_RADIX16"); return e ? std::atoi(e) : 1; }();  // measurement
  if (r16 && !g.inplace && !g.use_big && !g.blu_m && !g.zp_full && generic_lds_bytes(in, g, 2) > (160 * 1024 - 1024) / 2) {
    use_radix16(in, g);
    g.radix16 = true;
  }
  static const int force = [] { const char* e = std::getenv("FDOCT_FORCE_LONG_ROWS"); return e ? std::atoi(e) : 0; }();  // measurement
  if (force || in.plan_override == -3) g.use_big = true, g.inplace = false, g.zp_full = false;   // (-3: fdoct_set_plan's "rows in HBM")
  if (g.use_big && (N > (1 << 24) || MW > (1 << 24))) {
    *why = "rows of more than 2^24 points";
    return FDOCT_ERR_UNSUPPORTED;
  }
  return FDOCT_OK;
}

}  // namespace

int generic_buffer_len(const PlanInputs& in, const GenericPlan& g) {
  const int MW = in.W * in.M;
  int L = generic_real_half(in) ? in.N / 2 : in.N;
  if (in.M > 1) L = std::max(L, MW / 2);  // the zero-pad DFTs run at half length (real row, Hermitian spectrum)
  if (g.blu_m > L) L = g.blu_m;           // Bluestein: the transform runs as two power-of-two DFTs of this length
  if (in.M > 1 && g.zp_full) {            // the zero-pad stage at full length: both transforms, and the upsampled row as floats
    L = std::max(L, std::max(g.gzf.blu_m ? g.gzf.blu_m : in.W, g.gzi.blu_m ? g.gzi.blu_m : g.zn));
    L = std::max(L, (MW + 1) / 2);
  }
  return L;
}

size_t generic_lds_bytes(const PlanInputs& in, const GenericPlan& g, int buffers) {
  const int L = generic_buffer_len(in, g);
  const int ybuf = (in.W + 3) & ~3;
  if (!buffers) buffers = g.inplace ? 1 : 2;
  return (size_t)ybuf * 4 + (size_t)L * 8 * buffers + (size_t)((in.D + 3) & ~3) * 4;  // row, the DFT buffer(s), magnitude sums
}

// The compiled fused plan for (N, W, phase) where one applies, and the LDS geometry it runs with; configurations without a
// specialised kernel go to the generic path.
int make_plan(const PlanInputs& in, Plan* out, std::string* why) {
  Plan p;
  p.cplx = in.phase;
  p.NC = p.cplx ? in.N : in.N / 2;
  p.gen.rc = plan_generic(in, p.gen, &p.gen.why);
  p.wave_tw = wave_tw_layout(in.W, in.M, in.N, in.D, in.phase);
  const bool special_ok = is_pow2(in.N) && in.M == 1 && (in.W % 8) == 0 && (p.cplx || in.D <= in.N / 2) && in.plan_override > -2;
  // preference order for equal NC: the override, then the measured-fastest plan ids
  static const int pref[] = {5, 2, 3, 0, 1, 7, 6, 8, 4};  // per NC: fastest first; equal plans: smallest chunk count that holds W
  for (int i = -1; special_ok && !p.fused && i < (int)std::size(pref); i++) {
    FusedPlan q{};
    if (fused_plan_get(i < 0 ? in.plan_override : pref[i], &q) && q.nc == p.NC && in.W <= 8 * q.T * q.WCH) p.fused = q;
  }
  if (!p.fused) {
    if (p.gen.rc) {
      *why = p.gen.why;
      return p.gen.rc;
    }
  } else {
    const FusedPlan& f = *p.fused;
    const int WC = 8 * f.T * f.WCH;
    const int LP = f.R1 == 32 ? 5 : f.R1 == 16 ? 4 : f.R1 == 8 ? 3 : 2;
    const int stg = 4 * (WC + 4);
    const int xch = f.kind == 1 ? 8 * (65 * 16 + 2) : f.kind == 2 ? 8 * (129 * 16 + 2) : 8 * (p.NC + (p.NC >> LP) + 2);
    p.scratch_bytes = ((stg > xch ? stg : xch) + 15) & ~15;
    const double sigma = (p.cplx ? 1.0 : 2.0) * (double)(in.W * in.M) / (double)in.N;
    p.split = (sigma >= 1.5 && sigma <= 3.0) ? 1 : 0;
    int tw = (f.R2 - 1) * f.R1 + (f.R3 > 1 ? (f.R3 - 1) * f.R1 * f.R2 : 0);
    if (f.kind == 1) tw = 48 + 15 * 64;
    if (f.kind == 2) tw = 96 + 128;  // step-5 twiddles are formed as powers of W_2048^(l') in the kernel
    p.tw_count = (tw + 1) & ~1;
  }
  *out = std::move(p);
  return FDOCT_OK;
}

}  // namespace fdoct
