// fdoct_state.cpp -- the plan and the device state of a handle: the plan it adopts (fdoct_plan.h makes it), and everything the
// kernels read that is built on the host in double and uploaded once per change of the handle's state (reciprocal words of the
// background and their half-float pattern, window and slope planes, gather tables, twiddles, Bluestein chirps).  Part of the
// C-ABI layer (fdoct_ctx.h); no CPU compute path.
#include "fdoct_ctx.h"

namespace fdoct_impl {

int copy_ref_frame(fdoct_ctx* h, RefFrame& dst, const void* data, fdoct_dtype dtype, int rows, size_t pitch) {
  if (!data) {
    dst.v.clear();
    dst.rows = 0;
    invalidate(h);
    return FDOCT_OK;
  }
  const size_t es = dtype_size(dtype);
  if (!es) return fail(h, FDOCT_ERR_INVALID, "bad dtype");
  if (rows != 1 && rows != h->H) return fail(h, FDOCT_ERR_INVALID, "reference frame rows must be 1 or height");
  if (pitch == 0) pitch = es * h->W;
  if (pitch < es * h->W) return fail(h, FDOCT_ERR_INVALID, "pitch smaller than a row");
  dst.v.resize((size_t)rows * h->W);
  for (int r = 0; r < rows; r++) {
    const unsigned char* row = static_cast<const unsigned char*>(data) + (size_t)r * pitch;
    double* o = dst.v.data() + (size_t)r * h->W;
    for (int i = 0; i < h->W; i++) {
      switch (dtype) {
        case FDOCT_U8: o[i] = reinterpret_cast<const uint8_t*>(row)[i]; break;
        case FDOCT_U16: o[i] = reinterpret_cast<const uint16_t*>(row)[i]; break;
        case FDOCT_F32: o[i] = reinterpret_cast<const float*>(row)[i]; break;
        default: o[i] = reinterpret_cast<const double*>(row)[i]; break;
      }
    }
  }
  dst.rows = rows;
  invalidate(h);
  return FDOCT_OK;
}

PlanInputs plan_inputs(const fdoct_ctx* h) {
  return {h->W, h->M, h->N, h->D, !h->phase.empty(), h->plan_override, h->force_general};
}

// Makes the plan for `in` the handle's plan.  Nothing changes unless the plan is made in full; a new plan invalidates every
// device table.
int adopt_plan(fdoct_ctx* h, const PlanInputs& in) {
  Plan p;
  std::string why;
  if (int rc = make_plan(in, &p, &why)) return fail(h, rc, why);
  h->plan = std::move(p);
  invalidate(h);
  return FDOCT_OK;
}

// main:1132 divides by data_yb in double.  The kernels multiply by the reciprocal, held as an unevaluated sum of two floats
// ib + il = 1/yb to 2^-48: ib = fl32(1/yb) alone is off by up to 6e-8 of the quotient -- a fixed per-column pattern of the
// size of the DC level, which the chain turns into up to 4e-6 of the DC level per depth bin: more than the whole tolerance
// once the fringes are weaker than about 1 % of it.  With d = fma(v, ib, -c0) (rounded at the size of the deviation from the
// mean estimate c0) followed by d = fma(v, il, d), nothing is rounded at the size of the DC level.  x/0 -> 0 (OpenCV 3.x
// Mat division).
// float -> IEEE half bits, round to nearest even (values here are at most 2^14 in magnitude: no overflow handling needed beyond inf)
uint16_t half_bits(float f) {
  uint32_t x;
  std::memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  const int32_t e = (int32_t)((x >> 23) & 0xffu) - 127 + 15;
  uint32_t m = x & 0x7fffffu;
  if (((x >> 23) & 0xffu) == 0xffu) return (uint16_t)(sign | 0x7c00u | (m ? 0x200u : 0u));
  if (e >= 31) return (uint16_t)(sign | 0x7c00u);
  if (e <= 0) {  // subnormal half (or zero)
    if (e < -10) return (uint16_t)sign;
    m |= 0x800000u;
    const int shift = 14 - e;  // 13 + (1 - e)
    uint32_t r = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
    if (rem > halfway || (rem == halfway && (r & 1u))) r++;
    return (uint16_t)(sign | r);
  }
  uint32_t r = ((uint32_t)e << 10) | (m >> 13);
  const uint32_t rem = m & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) r++;  // (a carry into the exponent is the right result)
  return (uint16_t)(sign | r);
}

// The second word as the fast-path kernels with at most 32 samples per lane apply it (fdoct_fused_rules.h: fused_il_half): what
// v * ib leaves out of v / yb is (v * ib) * rho, rho = (1/yb - ib) / ib, |rho| <= 2^-24; the kernel adds c0 * rho (c0: its
// estimate of the row mean of v / yb).  rho * 2^38 as half floats, in the order the lanes read them: the lane's 8-sample group
// of chunk c is 16 bytes at ((c T + lane) * 16), dword q = samples chunk_pair_offset(q), + 2 (the RawChunk pair order).
void half_pattern_row(const double* yb, int WC, int T, uint32_t* out) {
  auto rho_h = [&](int i) -> uint16_t {
    if (yb[i] == 0.0) return 0;
    const double q = 1.0 / yb[i];
    const float ib = (float)q;
    if (!std::isfinite(ib) || ib == 0.f) return 0;
    return half_bits((float)(std::ldexp((q - (double)ib) / (double)ib, kPrec16Shift)));
  };
  for (int i0 = 0; i0 < WC; i0 += 8) {
    const int grp = i0 / 8, ln = grp % T, c = grp / T;
    for (int q = 0; q < 4; q++) {
      const int off = (q & 1) * 4 + (q >> 1);
      out[(size_t)(c * T + ln) * 4 + q] = (uint32_t)rho_h(i0 + off) | ((uint32_t)rho_h(i0 + off + 2) << 16);
    }
  }
}

void reciprocal_words(const std::vector<double>& yb, std::vector<float>& ib, std::vector<float>& il) {
  ib.resize(yb.size());
  il.resize(yb.size());
  for (size_t i = 0; i < yb.size(); i++) {
    if (yb[i] != 0.0) {
      const double q = 1.0 / yb[i];
      ib[i] = (float)q;
      const double lo = q - (double)ib[i];
      il[i] = std::isfinite(lo) ? (float)lo : 0.f;  // (1/yb beyond the float range: ib is inf, as before)
    } else {
      ib[i] = il[i] = 0.f;
    }
  }
}

// smoothmovavg (main:247-304, 990-991) divides its 2n + 2 taps by 2 (n + 1) in double.  An f32 quotient would be a rounding at the
// size of the DC level unless n + 1 is a power of two (5 x the tolerance on fringes of 0.1 % of it with n = 2), so the pass in front
// of the chain hands on the tap SUMS -- exact in f32 for the camera's integer samples up to n = 126 -- and the factor K = 2 (n + 1)
// goes where the reference's arithmetic puts it: into the dark frame (subtracted from the samples themselves), and, unless a min-max
// normalisation follows (it is scale-invariant), into the pi frame and the background as well.
PlaneScales plane_scales(const fdoct_ctx* h) {
  const double K = h->cfg.movavgn > 0 ? 2.0 * ((double)h->cfg.movavgn + 1.0) : 1.0;
  const bool norm_on = h->cfg.rowwisenormalize || (h->cfg.variant == FDOCT_VARIANT_SIM) || !h->cfg.donotnormalize;
  return {norm_on ? 1.0 : K, norm_on ? 1.0 : K, K};
}
std::vector<double> scaled_copy(const std::vector<double>& v, double s) {
  std::vector<double> t(v);
  if (s != 1.0)
    for (double& x : t) x *= s;
  return t;
}

// What the fused and the generic tables share: 1/background in double as two floats (reciprocal_words, into ib / il; a
// one-row background is uploaded as d_ib / d_il), the pi and dark frames with their second words, the phase.
static int upload_shared(fdoct_ctx* h, std::vector<float>& ib, std::vector<float>& il) {
  int rc;
  drain(h);  // the one wait of a rebuild (upload, fdoct_ctx.h): calls enqueued before the setter still read the tables that go
  reciprocal_words(scaled_copy(h->yb.v, plane_scales(h).yb), ib, il);
  if (h->yb.rows == 1) {
    if ((rc = upload(h, h->d_ib, ib))) return rc;
    if ((rc = upload(h, h->d_il, il))) return rc;
  } else {
    h->d_ib.release();
    h->d_il.release();
  }
  // (second words: what the float planes leave of the double ones -- read where the row is formed in double, BscanDark's band-pass)
  auto up_ref = [&](const RefFrame& f, double scale, DevBuf<float>& d, DevBuf<float>& d_lo) -> int {
    std::vector<float> t(f.v.size()), tl(f.v.size());
    for (size_t i = 0; i < t.size(); i++) {
      t[i] = (float)(f.v[i] * scale);
      tl[i] = (float)(f.v[i] * scale - (double)t[i]);
    }
    if (int e = upload(h, d_lo, tl)) return e;
    return upload(h, d, t);
  };
  if ((rc = up_ref(h->yp, plane_scales(h).yp, h->d_yp, h->d_yp_lo))) return rc;
  if ((rc = up_ref(h->yd, plane_scales(h).yd, h->d_yd, h->d_yd_lo))) return rc;
  std::vector<float2> ph(h->phase.size() / 2);
  for (size_t i = 0; i < ph.size(); i++) ph[i] = make_float2(h->phase[2 * i], h->phase[2 * i + 1]);
  return upload(h, h->d_phase, ph);
}

// Tables of the fused kernels.
int ensure_fused_tables(fdoct_ctx* h) {
  if (h->tables_ok & TABLES_FUSED) return FDOCT_OK;
  const int W = h->W, H = h->H, N = h->N;
  const Plan& pl = h->plan;
  const FusedPlan& p = *pl.fused;
  const int WC = 8 * p.T * p.WCH;
  DEVICE_SCOPE(h);
  int rc;
  {
    std::vector<float> ib, il;
    if ((rc = upload_shared(h, ib, il))) return rc;
    {  // the half-float pattern of the second word (rows exactly one chunk width wide: the fast path's condition)
      const std::vector<double> ybs = scaled_copy(h->yb.v, plane_scales(h).yb);
      std::vector<uint32_t> h16, h16_2d;
      if (W == WC && h->yb.rows == 1) {
        h16.resize((size_t)WC / 2);
        half_pattern_row(ybs.data(), WC, p.T, h16.data());
      } else if (W == WC && h->yb.rows > 1) {
        h16_2d.resize((size_t)H * WC / 2);
        for (int r = 0; r < H; r++) half_pattern_row(ybs.data() + (size_t)r * W, WC, p.T, h16_2d.data() + (size_t)r * WC / 2);
      }
      if ((rc = upload(h, h->d_il16, h16))) return rc;
      if ((rc = upload(h, h->d_il16_2d, h16_2d))) return rc;
    }
    if (h->yb.rows == 1) {
      // the low words again in the slot order of the kernels' LDS planes (sample 8 (ln + T c) + e -> c 8T + (e & 1) 4T + 4 ln + (e >> 1))
      std::vector<float> ilp((size_t)WC, 0.f);
      for (int i = 0; i < W; i++) {
        const int e = i & 7, ln = (i >> 3) & (p.T - 1), c = i / (8 * p.T);
        ilp[(size_t)c * 8 * p.T + (e & 1) * 4 * p.T + 4 * ln + (e >> 1)] = il[i];
      }
      if ((rc = upload(h, h->d_il_p, ilp))) return rc;
      h->d_ib2d_f.release();
      h->d_il2d_f.release();
    } else {
      // the fused kernels read a 2-D background with every 8-sample group stored evens first, then odds (the
      // order their sample pairs are held in), rows padded to the plan's chunk width; the generic kernel keeps
      // its own natural-order copy (d_ib2d)
      std::vector<float> perm((size_t)H * WC, 0.f);
      auto permute = [&](const std::vector<float>& src) {
        for (int r = 0; r < H; r++)
          for (int i = 0; i < W; i++) perm[(size_t)r * WC + (i & ~7) + ((i & 1) * 4 + ((i & 7) >> 1))] = src[(size_t)r * W + i];
      };
      permute(ib);
      if ((rc = upload(h, h->d_ib2d_f, perm))) return rc;
      permute(il);
      if ((rc = upload(h, h->d_il2d_f, perm))) return rc;
    }
  }
  {
    // Window (main:1142) and slope step (main:1153-1173) folded into two per-sample planes: with t = x - mean and
    // y = t * w, s_i = y_i + g_i (y_i - y_(i-1)) = a_i t_i + b_i t_(i-1), a_i = (1 + g_i) w_i, b_i = -g_i w_(i-1).
    // Sample 0 has slopes[0] = slopes[1] (main:1161): s_0 = (1 - g_0) w_0 t_0 + g_0 w_1 t_1; the kernel feeds t_1 there.
    // g_i = fractionalk[i]: the reference indexes fractionalk (N entries) by nearestkindex[q], a SAMPLE index; past N
    // it is out of bounds there and defined as 0 here.  Real path: the 1/2 of the real-input untangle is folded into
    // the window (exact: power of two).  Products in double, rounded once.
    std::vector<float> pa(W), pb(W);
    const double half = pl.cplx ? 1.0 : 0.5;
    auto gg = [&](int i) { return i < N ? h->frac[i] : 0.0; };
    for (int i = 1; i < W; i++) {
      pa[i] = (float)((1.0 + gg(i)) * half * h->win[i]);
      pb[i] = (float)(-gg(i) * half * h->win[i - 1]);
    }
    pa[0] = (float)((1.0 - gg(0)) * half * h->win[0]);
    pb[0] = (float)(gg(0) * half * h->win[1]);
    if ((rc = upload(h, h->d_win, pa))) return rc;
    if ((rc = upload(h, h->d_g, pb))) return rc;
  }
  {
    // gather sources: data_ylin[q] = s[nearestkindex[q]] for q = 1..N-2, else 0 (main:1164)
    std::vector<uint32_t> gi(pl.NC);
    auto off = [&](int q) -> uint32_t {
      if (q <= 0 || q >= N - 1) return (uint32_t)(4 * WC);
      return (uint32_t)staging_offset_bytes(h->idx[q], WC, pl.split);
    };
    for (int n = 0; n < pl.NC; n++) gi[n] = pl.cplx ? off(n) : (off(2 * n) | (off(2 * n + 1) << 16));
    if ((rc = upload(h, h->d_gidx, gi))) return rc;
  }
  {
    std::vector<float2> tw(pl.tw_count, make_float2(0.f, 0.f));
    size_t o = 0;
    if (p.kind == 1 || p.kind == 2) {
      // row-swap plans: tw2[(3c + i-1)*4 + j] = W_(4Q)^(i*(4c+j)), c < Q/4; tw3[(b-1)*L + l] = W_NC^(b*l), l < L = NC/16
      // (Q = first radix: 16 for fft1024_rowswap, 32 for fft2048_rowswap)
      const int Q = p.R1, L = pl.NC / 16;
      for (int c = 0; c < Q / 4; c++)
        for (int i = 1; i < 4; i++)
          for (int j = 0; j < 4; j++) {
            const double a = 2.0 * kPi * (double)(i * (4 * c + j)) / (double)(4 * Q);
            tw[(3 * c + i - 1) * 4 + j] = make_float2((float)std::cos(a), (float)std::sin(a));
          }
      for (int b = 1; b < (p.kind == 1 ? 16 : 2); b++)  // kind 2 keeps only the b = 1 row
        for (int l = 0; l < L; l++) {
          const double a = 2.0 * kPi * (double)(b * l) / (double)pl.NC;
          tw[3 * Q + (b - 1) * L + l] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
    } else
    for (int r = 1; r < p.R2; r++)
      for (int k = 0; k < p.R1; k++) {
        const double a = 2.0 * kPi * (double)r * (double)k / (double)(p.R1 * p.R2);
        tw[o++] = make_float2((float)std::cos(a), (float)std::sin(a));
      }
    if (p.kind == 0 && p.R3 > 1)
      for (int r = 1; r < p.R3; r++)
        for (int k = 0; k < p.R1 * p.R2; k++) {
          const double a = 2.0 * kPi * (double)r * (double)k / (double)pl.NC;
          tw[o++] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
    if ((rc = upload(h, h->d_tw, tw))) return rc;
    std::vector<float2> utw(p.T);
    for (int l = 0; l < p.T; l++) {
      const double a = 2.0 * kPi * (double)l / (double)N;
      utw[l] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    if ((rc = upload(h, h->d_utw, utw))) return rc;
  }
  h->tables_ok |= TABLES_FUSED;
  return FDOCT_OK;
}

// Bluestein tables for the +i transform of length n: X[k] = c[k] * sum_m (x[m] c[m]) conj(c[k-m]), c[m] = e^(+i pi m^2/n)
// (m^2 taken mod 2n in integers, so the angle stays exact); bhat = forward DFT of the wrapped conj(c), scaled by 1/Mb for
// the unscaled inverse transform that follows it in the kernels.  Computed in double.
void build_bluestein_tables(int n, int Mb, std::vector<float2>& chirp, std::vector<float2>& bhat) {
  std::vector<double> cr(n), ci(n);
  chirp.resize(n);
  for (long long m = 0; m < n; m++) {
    const double ang = kPi * (double)((m * m) % (2LL * n)) / (double)n;
    cr[m] = std::cos(ang);
    ci[m] = std::sin(ang);
    chirp[m] = make_float2((float)cr[m], (float)ci[m]);
  }
  std::vector<double> br(Mb, 0.0), bi(Mb, 0.0);
  for (int m = 0; m < n; m++) {
    br[m] = cr[m];
    bi[m] = -ci[m];
    if (m) {
      br[Mb - m] = cr[m];
      bi[Mb - m] = -ci[m];
    }
  }
  if (Mb & (Mb - 1)) {
    // Mb = 2^a 3^b 5^c (the LDS kernels' Bluestein, round 6: the smallest such length >= 2n - 1 instead of the next power of
    // two -- 2592 instead of 4096 around a 1283-point transform): the forward DFT by its definition, in double, with the
    // angle's index taken mod Mb in integers (<= 8192^2 complex multiply-adds, once per handle)
    std::vector<double> wr(Mb), wi(Mb);
    for (int j = 0; j < Mb; j++) {
      const double ang = -2.0 * kPi * (double)j / (double)Mb;
      wr[j] = std::cos(ang);
      wi[j] = std::sin(ang);
    }
    std::vector<int> nz;   // (the wrapped chirp has 2n - 1 non-zero entries)
    for (int m = 0; m < Mb; m++)
      if (br[m] != 0.0 || bi[m] != 0.0) nz.push_back(m);
    bhat.resize(Mb);
    for (int k = 0; k < Mb; k++) {
      double sr = 0.0, si = 0.0;
      for (int m : nz) {
        const int t = (int)(((long long)m * k) % Mb);
        sr += br[m] * wr[t] - bi[m] * wi[t];
        si += br[m] * wi[t] + bi[m] * wr[t];
      }
      bhat[k] = make_float2((float)(sr / Mb), (float)(si / Mb));
    }
    return;
  }
  // forward DFT of length Mb (power of two) in double: iterative radix-2
  for (int i = 1, j = 0; i < Mb; i++) {
    int bit = Mb >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) {
      std::swap(br[i], br[j]);
      std::swap(bi[i], bi[j]);
    }
  }
  for (int len = 2; len <= Mb; len <<= 1) {
    const double ang = -2.0 * kPi / (double)len;
    for (int i = 0; i < Mb; i += len)
      for (int k = 0; k < len / 2; k++) {
        const double wr = std::cos(ang * k), wi = std::sin(ang * k);
        const double ur = br[i + k], ui = bi[i + k];
        const double vr = br[i + k + len / 2] * wr - bi[i + k + len / 2] * wi, vi = br[i + k + len / 2] * wi + bi[i + k + len / 2] * wr;
        br[i + k] = ur + vr;
        bi[i + k] = ui + vi;
        br[i + k + len / 2] = ur - vr;
        bi[i + k + len / 2] = ui - vi;
      }
  }
  bhat.resize(Mb);
  for (int m = 0; m < Mb; m++) bhat[m] = make_float2((float)(br[m] / Mb), (float)(bi[m] / Mb));
}

// Tables of the generic path (and of the long-row path, which makes its own DFT tables as it goes: big_plan_get).
int ensure_generic_tables(fdoct_ctx* h) {
  const GenericPlan& gp = h->plan.gen;
  if (gp.rc) return fail(h, gp.rc, gp.why);
  if (h->tables_ok & TABLES_GENERIC) return FDOCT_OK;
  int rc;
  const int W = h->W, N = h->N, MW = h->W * h->M;
  DEVICE_SCOPE(h);
  {
    std::vector<float> ib, il;
    if ((rc = upload_shared(h, ib, il))) return rc;
    if (h->yb.rows == 1) {
      h->d_ib2d.release();
      h->d_il2d.release();
    } else {
      if ((rc = upload(h, h->d_ib2d, ib))) return rc;
      if ((rc = upload(h, h->d_il2d, il))) return rc;
    }
  }
  std::vector<float> w(W), g(MW);
  for (int i = 0; i < W; i++) w[i] = (float)h->win[i];
  for (int i = 0; i < MW; i++) g[i] = (i < N) ? (float)h->frac[i] : 0.f;  // fractionalk[nearestkindex[q]], 0 past its end
  if ((rc = upload(h, h->d_win_g, w))) return rc;
  {
    std::vector<float> wl(W);
    for (int i = 0; i < W; i++) wl[i] = (float)(h->win[i] - (double)w[i]);
    if ((rc = upload(h, h->d_win_lo_g, wl))) return rc;
  }
  if ((rc = upload(h, h->d_g_g, g))) return rc;
  if ((rc = upload(h, h->d_idx_g, h->idx))) return rc;
  auto up_tw = [&](int n, DevBuf<float2>& d) -> int {
    std::vector<float2> t(n);
    for (int j = 0; j < n; j++) {
      const double a = 2.0 * kPi * (double)j / (double)n;
      t[j] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    return upload(h, d, t);
  };
  if ((rc = up_tw(N, h->d_twg_n))) return rc;
  if ((N % 2) == 0 && (rc = up_tw(N / 2, h->d_twg_nh))) return rc;
  if (gp.blu_m) {
    const int n = generic_real_half(plan_inputs(h)) ? N / 2 : N, Mb = gp.blu_m;
    std::vector<float2> chirp, bhat;
    build_bluestein_tables(n, Mb, chirp, bhat);
    if ((rc = upload(h, h->d_blu_chirp, chirp))) return rc;
    if ((rc = upload(h, h->d_blu_bhat, bhat))) return rc;
    if ((rc = up_tw(Mb, h->d_twg_blu))) return rc;
  }
  if (h->M > 1 && gp.zp_full) {  // the full-length zero-pad stage's two plans
    auto up_dft = [&](const GenericDftPlan& p, fdoct_ctx::GenericDftTables& d) -> int {
      if (int e = up_tw(p.blu_m ? p.blu_m : p.n, d.tw)) return e;
      if (!p.blu_m) return FDOCT_OK;
      std::vector<float2> chirp, bhat;
      build_bluestein_tables(p.n, p.blu_m, chirp, bhat);
      if (int e = upload(h, d.chirp, chirp)) return e;
      return upload(h, d.bhat, bhat);
    };
    if ((rc = up_dft(gp.gzf, h->d_gzf)) || (rc = up_dft(gp.gzi, h->d_gzi))) return rc;
  }
  if (h->M > 1) {
    if ((rc = up_tw(W, h->d_twg_w))) return rc;     // untangle factors of the half-length transforms
    if ((rc = up_tw(MW, h->d_twg_mw))) return rc;
    if ((rc = up_tw(W / 2, h->d_twg_wh))) return rc;
    if ((rc = up_tw(MW / 2, h->d_twg_mwh))) return rc;
  }
  if (!h->d_gen_tickets && (rc = h->d_gen_tickets.assign(h, 64))) return rc;   // generic_kernel's row counters (launch_family_generic)
  h->tables_ok |= TABLES_GENERIC;
  return FDOCT_OK;
}

// Tables of the wave-per-row kernels: packed gather sources and the twiddle blob, laid out by wave_tw_layout (fdoct_wave_rules.h)
// [N/2 passes][M W/2 passes][W/2 passes][e^(2 pi i k/W), k < W/2][e^(2 pi i k/(M W)), k < W/2][e^(2 pi i k/N), k < D];
// with the generic path's, whose device copies of the window and the resample table they read.
int ensure_wave_tables(fdoct_ctx* h) {
  int rc;
  if ((rc = ensure_generic_tables(h))) return rc;
  if (h->tables_ok & TABLES_WAVE) return FDOCT_OK;
  if (h->d_wave_gidx) drain(h);  // (the generic rebuild above has waited when it ran; this holds where it did not)
  // complex rows (dispersion phase): the final transform runs over the whole row, one gather source per point
  const bool cplx = !h->phase.empty();
  const int W = h->W, M = h->M, N = h->N, MW = W * M, NC = cplx ? N : N / 2;
  std::vector<uint32_t> gi(NC);
  auto src = [&](int q) -> uint32_t { return (q <= 0 || q >= N - 1) ? (uint32_t)MW : (uint32_t)h->idx[q]; };  // main:1164
  for (int n = 0; n < NC; n++) gi[n] = cplx ? src(n) : (src(2 * n) | (src(2 * n + 1) << 16));
  const WaveTwLayout& lay = h->plan.wave_tw;
  std::vector<float2> tw(lay.count);
  auto unit = [&](double num, double den) {
    const double ang = 2.0 * kPi * num / den;
    return make_float2((float)std::cos(ang), (float)std::sin(ang));
  };
  auto pass_tables = [&](int at, int n) {
    const WavePlan p = wave_plan(n);
    for (int i = 0; i < p.npass; i++)
      if (p.Ns[i] > 1)
        for (int k = 0; k < p.Ns[i]; k++) tw[at++] = unit((double)k, (double)p.Ns[i] * p.R[i]);
  };
  pass_tables(lay.off[0], NC);
  if (M > 1) {
    pass_tables(lay.off[1], MW / 2);
    pass_tables(lay.off[2], W / 2);
    for (int k = 0; k < W / 2; k++) tw[lay.off[3] + k] = unit((double)k, (double)W);
    for (int k = 0; k < W / 2; k++) tw[lay.off[4] + k] = unit((double)k, (double)MW);
  }
  // untangle factors of the real rows: bins below numdisplaypoints, or (displayed beyond N/2: the upper bins mirror) up to N/2
  for (int k = 0; lay.off[5] + k < lay.count; k++) tw[lay.off[5] + k] = unit((double)k, (double)N);
  if ((rc = upload(h, h->d_wave_gidx, gi))) return rc;
  if ((rc = upload(h, h->d_wave_tw, tw))) return rc;
  h->tables_ok |= TABLES_WAVE;
  return FDOCT_OK;
}

}  // namespace fdoct_impl
