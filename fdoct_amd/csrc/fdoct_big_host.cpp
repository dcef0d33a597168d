// fdoct_big_host.cpp -- the long-row path's host side: the DFT plan and tables of one length (big_plan_get), what stands
// in front of a transform (BigLoader), one transform as grouped launches or Bluestein around them (big_idft), and the whole chain for
// device-resident frames, chunk by chunk (run_big: launch_family_long_rows of fdoct_route.cpp calls it).  Part of the C-ABI layer
// (fdoct_ctx.h).
#include "fdoct_ctx.h"

namespace fdoct_impl {

// ---- long-row path (fdoct_big.hip) ----------------------------------------------------------------------------------
// (the plans of its transforms and the chunks of a batch are values: fdoct_big_plan.h)
// DFT plan of one length: Stockham radices when it factors into 2, 3, 5, else Bluestein around a power of two >= 2n - 1.
int big_plan_get(fdoct_ctx* h, int n, fdoct_ctx::BigPlan** out) {
  auto it = h->big_plans.find(n);
  if (it != h->big_plans.end()) {
    *out = &it->second;
    return FDOCT_OK;
  }
  fdoct_ctx::BigPlan p;
  static const bool per_pass = [] { const char* e = std::getenv("FDOCT_BIG_PER_PASS"); return e && std::atoi(e) != 0; }();  // measurement: round 3's form
  BigTransform t = make_big_transform(n, per_pass);
  p.rad = std::move(t.rad);
  p.groups = std::move(t.groups);
  p.mb = t.mb;
  const int tn = t.tn;
  if (p.mb) {
    std::vector<float2> chirp, bhat;
    build_bluestein_tables(n, p.mb, chirp, bhat);
    int rc;
    if ((rc = upload(h, p.d_chirp, chirp))) return rc;
    if ((rc = upload(h, p.d_bhat, bhat))) return rc;
  }
  std::vector<float2> tw(tn);
  for (int j = 0; j < tn; j++) {
    const double a = 2.0 * kPi * (double)j / (double)tn;
    tw[j] = make_float2((float)std::cos(a), (float)std::sin(a));
  }
  int rc;
  if ((rc = upload(h, p.d_tw, tw))) return rc;
  *out = &h->big_plans.emplace(n, std::move(p)).first->second;
  return FDOCT_OK;
}

// What stands in front of a transform, fused into the loads of its first launch (or run as a kernel of its own where the
// transform is not one of grouped launches): the row of floats read as complex (A4's first transform), the W-point spectrum
// re-packed into the M W-point one (A4), the slope step and lambda -> k gather with the phase (A5 / A6 / A6').
struct BigLoader {
  int load = BIG_LOAD_CPLX;
  const float* yr = nullptr;
  const float2* yc = nullptr;
  const float2* spec = nullptr;
  int ylen = 0, W = 0, bandpass = 0;
  const int32_t* idx = nullptr;
  const float* g = nullptr;
  const float2* phase = nullptr;
};

// X = IDFT_n (+i exponent, unscaled) of `rows` rows; x holds them (ld == null) or is free and the loader supplies them;
// `other` is the second buffer (both hold rows * max(n, mb) values).  *result = the buffer that holds the rows * n result;
// out_limit > 0: only the first out_limit values of each result row are needed (and, with grouped launches, written).
int big_idft(fdoct_ctx* h, float2* x, float2* other, long long rows, int n, float2** result, hipStream_t st, const BigLoader* ld = nullptr,
             int out_limit = 0) {
  fdoct_ctx::BigPlan* p = nullptr;
  int rc;
  if ((rc = big_plan_get(h, n, &p))) return rc;
  auto materialise = [&]() -> int {  // the loader as a kernel of its own, into x
    if (!ld) return FDOCT_OK;
    switch (ld->load) {
      case BIG_LOAD_REAL: HIP_TRY(h, big_launch_real_to_complex(ld->yr, rows * n, x, st)); break;
      case BIG_LOAD_PAD: HIP_TRY(h, big_launch_pad(ld->spec, rows, ld->W, n, ld->bandpass, x, st)); break;
      case BIG_LOAD_RESAMPLE: HIP_TRY(h, big_launch_resample(ld->yr, ld->yc, rows, ld->ylen, n, ld->idx, ld->g, ld->phase, x, st)); break;
      default: break;
    }
    return FDOCT_OK;
  };
  // the passes of one len-point transform over src -> ... -> *last (ping-pong between the two buffers)
  auto passes = [&](float2*& src, float2*& dst, int len, const BigLoader* first_ld, int limit) -> int {
    if (!p->groups.empty()) {
      for (size_t gi = 0; gi < p->groups.size(); gi++) {
        const auto& gp = p->groups[gi];
        BigGroup g{};
        g.src = src; g.dst = dst; g.rows = rows; g.n = len;
        g.P = gp.P; g.Q = gp.Q; g.F = gp.F; g.log2ts = gp.log2ts;
        g.npass = (int)gp.rad.size();
        for (int i = 0; i < g.npass; i++) g.rad[i] = gp.rad[i];
        g.out_limit = (gi + 1 == p->groups.size() && limit > 0) ? limit : len;
        g.tw = p->d_tw;
        g.load = BIG_LOAD_CPLX;
        if (gi == 0 && first_ld) {
          g.load = first_ld->load;
          g.yr = first_ld->yr; g.yc = first_ld->yc; g.ylen = first_ld->ylen;
          g.idx = first_ld->idx; g.g = first_ld->g; g.phase = first_ld->phase;
          g.W = first_ld->W; g.bandpass = first_ld->bandpass;
          if (first_ld->load == BIG_LOAD_PAD) g.src = first_ld->spec;
        }
        HIP_TRY(h, big_launch_fft_group(g, st));
        std::swap(src, dst);
      }
      return FDOCT_OK;
    }
    int Ns = 1;
    for (int R : p->rad) {
      HIP_TRY(h, big_launch_fft_pass(src, dst, rows, len, R, Ns, p->d_tw, st));
      std::swap(src, dst);
      Ns *= R;
    }
    return FDOCT_OK;
  };
  float2 *src = x, *dst = other;
  if (!p->mb) {
    const bool fused = ld && !p->groups.empty();
    if (!fused && (rc = materialise())) return rc;
    if ((rc = passes(src, dst, n, fused ? ld : nullptr, out_limit))) return rc;
    *result = src;
    return FDOCT_OK;
  }
  // Bluestein: u = conj(x c) zero-padded; conj(IDFT u) = DFT(x c); times bhat; IDFT; times c
  if ((rc = materialise())) return rc;
  HIP_TRY(h, big_launch_chirp_in(x, rows, n, p->mb, p->d_chirp, other, st));
  src = other;
  dst = x;
  if ((rc = passes(src, dst, p->mb, nullptr, 0))) return rc;
  HIP_TRY(h, big_launch_conj_mul(src, rows, p->mb, p->d_bhat, st));
  if ((rc = passes(src, dst, p->mb, nullptr, 0))) return rc;
  HIP_TRY(h, big_launch_chirp_out(src, rows, n, p->mb, p->d_chirp, dst, st));
  *result = dst;
  return FDOCT_OK;
}

// The whole chain for device-resident frames on the long-row path, chunk by chunk of whole averaging groups.
int run_big(fdoct_ctx* h, const void* kframes, const float* kframes_lo, int kdt, size_t kpitch, int nframes, bool need_minmax, float* k_mag, float* k_db,
            hipStream_t st) {
  const int W = h->W, H = h->H, N = h->N, D = h->D, M = h->M, A = h->A;
  // the padded spectrum / upsampled row: W + 2 floor((M W - W) / 2) points (main:229) -- M W, or M W - 1 for an odd width under an
  // even multiplier
  const int MW = W + 2 * ((W * M - W) / 2);
  int rc;
  size_t lmax = (size_t)std::max(N, M > 1 ? MW : 0);
  for (int n : {N, M > 1 ? W : 0, M > 1 ? MW : 0}) {
    if (!n) continue;
    fdoct_ctx::BigPlan* p = nullptr;
    if ((rc = big_plan_get(h, n, &p))) return rc;
    lmax = std::max(lmax, (size_t)std::max(n, p->mb));
  }
  const int G = nframes / A;
  long long chunk_mb = 0;
  if (const char* e = std::getenv("FDOCT_BIG_CHUNK_MB")) chunk_mb = std::atoll(e);  // read per call, like FDOCT_HOST_CHUNK_MB: the tests cut small batches with it
  const BigChunks ch = make_big_chunks(W, H, A, G, lmax, big_chunk_budget(chunk_mb));
  const long long cg = ch.cg;
  const size_t crow = ch.rows;
  if ((rc = h->ws_big_y.reserve(h, crow * W * 4))) return rc;
  if ((rc = h->ws_big_a.reserve(h, crow * lmax * sizeof(float2)))) return rc;
  if ((rc = h->ws_big_b.reserve(h, crow * lmax * sizeof(float2)))) return rc;
  for (long long g0 = 0; g0 < G; g0 += cg) {
    const long long ng = std::min<long long>(cg, G - g0);
    BigArgs a{};
    a.frames = static_cast<const unsigned char*>(kframes) + (size_t)g0 * A * H * kpitch;
    a.frames_lo = kframes_lo ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(kframes_lo) + (size_t)g0 * A * H * kpitch) : nullptr;
    a.pitch_bytes = (long long)kpitch;
    a.in_rows = ng * A * H;
    a.out_rows = ng * H;
    a.dtype = kdt;
    a.W = W; a.H = H; a.N = N; a.D = D; a.M = M; a.A = A;
    a.ib = h->yb.rows == 1 ? h->d_ib : h->d_ib2d;
    a.il = h->yb.rows == 1 ? h->d_il : h->d_il2d;
    a.ib_2d = h->yb.rows > 1;
    a.yp = h->d_yp; a.yp_2d = h->yp.rows > 1;
    a.yd = h->d_yd; a.yd_2d = h->yd.rows > 1;
    a.win = h->d_win_g;
    a.minmax = need_minmax ? h->d_minmax + (size_t)g0 * A : nullptr;
    a.rowwisenormalize = h->cfg.rowwisenormalize;
    a.dcmask = h->cfg.dc_mask;
    a.inv_A = (float)(1.0 / (double)A);
    a.eps = kernel_eps(h);
    a.db_scale = (float)(20.0 / 2.303 * 0.6931471805599453);
    HIP_TRY(h, big_launch_pre(a, h->ws_big_y, st));
    // Buffer discipline of big_idft with a loader: the first launch reads the loader's source and writes `other`, the next one
    // writes `x`, and so on; so the source may live in x (it is dead once the first launch is through) but never in `other`.
    // A transform that cannot fuse its loader (one launch per pass, Bluestein) materialises the rows into x first: there the
    // source must not live in x.
    float2 *bufa = h->ws_big_a, *bufb = h->ws_big_b, *res = nullptr;
    auto fuses = [&](int n, bool* yes) -> int {
      fdoct_ctx::BigPlan* p = nullptr;
      if (int rc2 = big_plan_get(h, n, &p)) return rc2;
      *yes = !p->mb && !p->groups.empty();
      return FDOCT_OK;
    };
    BigLoader rs;                 // A5 / A6 / A6': what the final transform reads
    rs.load = BIG_LOAD_RESAMPLE;
    rs.yr = h->ws_big_y;
    rs.ylen = W;
    rs.idx = h->d_idx_g;
    rs.g = h->d_g_g;
    rs.phase = h->d_phase;
    float2* held = nullptr;       // the buffer the final transform's source rows live in (null: the float rows)
    if (M > 1) {  // A4
      BigLoader l1;
      l1.load = BIG_LOAD_REAL;
      l1.yr = h->ws_big_y;
      if ((rc = big_idft(h, bufa, bufb, a.in_rows, W, &res, st, &l1))) return rc;
      BigLoader l2;
      l2.load = BIG_LOAD_PAD;
      l2.spec = res;
      l2.W = W;
      l2.bandpass = h->bandpass ? 1 : 0;
      float2* spare = (res == bufa) ? bufb : bufa;
      bool f = false;
      if ((rc = fuses(MW, &f))) return rc;
      if ((rc = f ? big_idft(h, res, spare, a.in_rows, MW, &res, st, &l2) : big_idft(h, spare, res, a.in_rows, MW, &res, st, &l2))) return rc;
      rs.yr = nullptr;
      rs.yc = res;
      rs.ylen = MW;
      held = res;
    }
    {  // A5 / A6 / A7; only the first numdisplaypoints bins of the result are needed
      float2* spare = held ? (held == bufa ? bufb : bufa) : bufb;
      float2* mine = held ? held : bufa;
      bool f = false;
      if ((rc = fuses(N, &f))) return rc;
      if ((rc = f ? big_idft(h, mine, spare, a.in_rows, N, &res, st, &rs, D) : big_idft(h, held ? spare : mine, held ? mine : spare, a.in_rows, N, &res, st, &rs, D)))
        return rc;
    }
    HIP_TRY(h, big_launch_post(res, a, k_mag ? k_mag + (size_t)g0 * H * D : nullptr, k_db ? k_db + (size_t)g0 * H * D : nullptr, st));
  }
  return FDOCT_OK;
}

}  // namespace fdoct_impl
