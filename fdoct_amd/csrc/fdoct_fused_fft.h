// fdoct_fused_fft.h -- the inverse DFT of fused_kernel (fdoct_kernels.hip, A7): Stockham passes through the padded LDS exchange
// buffer, and the one-exchange row-swap plans of 1024 and 2048 points.
#pragma once
#include "fdoct_fused_dev.h"

namespace fdoct {

// Exchange-buffer layout: element e lives at slot e + (e >> LP) (one pad slot per
// 2^LP elements, LP = log2 of the first radix).  Unlike an XOR swizzle this is
// additive, so every LDS access below is <one per-lane base VGPR> + <immediate>;
// writes are conflict free for every compiled plan and read-backs are conflict
// free when the first radix is 32 (tests/kernel_model.py checks the banking).
template <int LP>
__device__ __forceinline__ constexpr int padded(int e) {
  return e + (e >> LP);
}

// One Stockham pass over the T-lane group, in three pieces so that the kernel can issue the
// (row-invariant) twiddle reads of a pass behind the previous pass's exchange writes and have a
// single wait cover both:  z[m] = element (l + T*m).
//   pass_twiddles : LDS -> registers, (R-1) twiddles per butterfly
//   pass_compute  : twiddle multiply, radix-R butterflies, exchange writes (or registers if LAST)
//   pass_readback : natural-order read-back of the exchange buffer
template <int NC, int T, int R, int NS>
__device__ __forceinline__ void pass_twiddles(v2f* twr, int l, const v2f* tw) {
  constexpr int P = NC / T;
  constexpr int NB = P / R;
  static_for<0, NB>([&](auto tc) {
    constexpr int t = decltype(tc)::value;
    const v2f* twk = tw + ((l + T * t) & (NS - 1));
    static_for<1, R>([&](auto rc) {
      constexpr int r = decltype(rc)::value;
      twr[t * (R - 1) + (r - 1)] = twk[(r - 1) * NS];
    });
  });
}

template <int NC, int T, int R, int NS, bool LAST, int LP, bool INV>
__device__ __forceinline__ void pass_compute(v2f* z, int l, v2f* xch, const v2f* twr) {
  constexpr int P = NC / T;
  constexpr int NB = P / R;  // butterflies per lane
  static_assert(P % R == 0, "radix must divide the per-lane point count");
  static_assert(NS == 1 || NS >= (1 << LP), "later passes must keep pad-aligned strides");
  static_for<0, NB>([&](auto tc) {
    constexpr int t = decltype(tc)::value;
    const int j = l + T * t;
    const int k = j & (NS - 1);
    v2f v[R];
    static_for<0, R>([&](auto rc) {
      constexpr int r = decltype(rc)::value;
      v[r] = z[t + r * NB];
    });
    if constexpr (NS > 1) {
      static_for<1, R>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        v[r] = cmul(v[r], twr[t * (R - 1) + (r - 1)]);
      });
    }
    fft_reg<R, INV>(v);
    if constexpr (LAST) {
      static_for<0, R>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        z[t + r * NB] = v[r];
      });
    } else {
      const int e0 = (j / NS) * (NS * R) + k;
      v2f* dst = xch + (e0 + (e0 >> LP));
      static_for<0, R>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        dst[padded<LP>(r * NS)] = v[r];  // (e0 + r*NS) >> LP == (e0 >> LP) + ((r*NS) >> LP) here
      });
    }
  });
}

template <int NC, int T, int LP>
__device__ __forceinline__ void pass_readback(v2f* z, int l, const v2f* xch) {
  constexpr int P = NC / T;
  if constexpr (T >= (1 << LP)) {
    const v2f* src = xch + (l + (l >> LP));
    static_for<0, P>([&](auto mc) {
      constexpr int m = decltype(mc)::value;
      z[m] = src[padded<LP>(T * m)];
    });
  } else {
    const v2f* src = xch + l;  // l < T < 2^LP: the pad term depends on m only
    static_for<0, P>([&](auto mc) {
      constexpr int m = decltype(mc)::value;
      z[m] = src[T * m + ((T * m) >> LP)];
    });
  }
}

// 1024-point inverse DFT on a full wave with ONE LDS exchange (plan "16 | row swap | 4 | LDS | 16").
// Index split n = 64*m + 16*a + b (m: register, a: 16-lane row, b: lane in row), output
// k = k1 + 16*k2 + 64*k3:
//   1. radix-16 over m in registers                      -> A[k1][a][b], k1 in the register index
//   2. 4x4 transpose between the lane row a and the low two bits of k1, done with
//      v_permlane32_swap / v_permlane16_swap on register quads (no LDS)
//   3. twiddle W_64^(a*k1), radix-4 over a               -> B[k1][k2][b]
//   4. LDS exchange b <-> (k1,k2): element (b, l') at slot 65*b + l', l' = k1 + 16*k2
//      (stride 65: conflict-free writes; reads are contiguous)
//   5. twiddle W_1024^(b*l'), radix-16 over b            -> X[l' + 64*k3] in register k3 (natural)
// tw2[(3*c + i-1)*4 + j] = W_64^(i*(4c+j)), tw3[(b-1)*64 + l'] = W_1024^(b*l')  (host tables).
// tests/kernel_model.py::fft1024_rowswap_model is the index-for-index numpy model.
__device__ __forceinline__ void swap_rows32(float& x, float& y) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
  x = __uint_as_float(r[0]);
  y = __uint_as_float(r[1]);
}
__device__ __forceinline__ void swap_rows16(float& x, float& y) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
  x = __uint_as_float(r[0]);
  y = __uint_as_float(r[1]);
}

// RESTW: the caller keeps the 12 + 15 row-invariant twiddles in registers (rt2 / rt3, loaded with
// fft1024_rowswap_twiddles) instead of re-reading them from LDS for every row.
__device__ __forceinline__ void fft1024_rowswap_twiddles(int lane, const v2f* tw2, const v2f* tw3, v2f* rt2, v2f* rt3) {
  const int j = lane >> 4;
  static_for<0, 12>([&](auto ec) {
    constexpr int e = decltype(ec)::value;
    rt2[e] = tw2[e * 4 + j];
  });
  static_for<1, 16>([&](auto bc) {
    constexpr int bb = decltype(bc)::value;
    rt3[bb - 1] = tw3[(bb - 1) * 64 + lane];
  });
}

template <int RES2, bool RES3>  // RES2: how many of the 12 step-3 twiddles the caller keeps in registers (the first RES2)
__device__ __forceinline__ void fft1024_rowswap(v2f* z, int lane, v2f* xch, const v2f* tw2, const v2f* tw3, const v2f* rt2,
                                                const v2f* rt3, FusedProbe& pr) {
  const int j = lane >> 4, b = lane & 15;
  // 1. radix-16 over the register index
  fft_reg<16, true>(z);
  FDOCT_FPR(pr, 3);
  // Steps 2-4 one register quad at a time (the transposition stays inside a quad).  The quad's three step-3 twiddles come
  // from the caller's registers (the first RES2 of the twelve) or from LDS, read one quad ahead: six registers in flight
  // instead of twenty-four.
  auto quad_twiddles = [&](auto cc, v2f* t) {
    constexpr int c = decltype(cc)::value;
    static_for<0, 3>([&](auto ic) {
      constexpr int e = 3 * c + decltype(ic)::value;
      if constexpr (e < RES2)
        t[e - 3 * c] = rt2[e];
      else
        t[e - 3 * c] = tw2[e * 4 + j];
    });
  };
  v2f* dst = xch + (65 * b + j);
  v2f tnext[3];
  quad_twiddles(IC<0>{}, tnext);
  static_for<0, 4>([&](auto cc) {
    constexpr int c = decltype(cc)::value;
    const v2f t2[3] = {tnext[0], tnext[1], tnext[2]};
    if constexpr (c < 3) quad_twiddles(IC<c + 1>{}, tnext);
    // 2. transpose (row a) <-> (k1 & 3) inside the register quad
    float x0 = z[4 * c].x, y0 = z[4 * c].y, x1 = z[4 * c + 1].x, y1 = z[4 * c + 1].y;
    float x2 = z[4 * c + 2].x, y2 = z[4 * c + 2].y, x3 = z[4 * c + 3].x, y3 = z[4 * c + 3].y;
    swap_rows32(x0, x2);
    swap_rows32(y0, y2);
    swap_rows32(x1, x3);
    swap_rows32(y1, y3);
    swap_rows16(x0, x1);
    swap_rows16(y0, y1);
    swap_rows16(x2, x3);
    swap_rows16(y2, y3);
    // 3. register 4c+i of lane (j,b) now holds A[k1 = 4c+j][a = i][b]
    v2f v[4] = {mk(x0, y0), cmul(mk(x1, y1), t2[0]), cmul(mk(x2, y2), t2[1]), cmul(mk(x3, y3), t2[2])};
    fft_reg<4, true>(v);
    // 4. B[k1 = 4c+j][k2][b] -> slot 65*b + (4c + j) + 16*k2
    static_for<0, 4>([&](auto kc) {
      constexpr int k2 = decltype(kc)::value;
      dst[4 * c + 16 * k2] = v[k2];
    });
  });
  // step-5 twiddles queue behind the exchange writes so one wait covers both
  v2f t3[15];
  static_for<1, 16>([&](auto bc) {
    constexpr int bb = decltype(bc)::value;
    if constexpr (RES3)
      t3[bb - 1] = rt3[bb - 1];
    else
      t3[bb - 1] = tw3[(bb - 1) * 64 + lane];
  });
  wave_lds_sync();
  FDOCT_FPR(pr, 5);   // (the 1024-point plan does the row swap quad by quad inside steps 3 / 4: phase 4 stays empty)
  const v2f* src = xch + lane;
  static_for<0, 16>([&](auto bc) {
    constexpr int bb = decltype(bc)::value;
    z[bb] = src[65 * bb];
  });
  wave_lds_sync();
  FDOCT_FPR(pr, 6);
  // 5. twiddle and radix-16 over b
  static_for<1, 16>([&](auto bc) {
    constexpr int bb = decltype(bc)::value;
    z[bb] = cmul(z[bb], t3[bb - 1]);
  });
  fft_reg<16, true>(z);
  FDOCT_FPR(pr, 7);
}

// 2048-point version of the same plan ("32 | row swap | 4 | LDS | 16 x2"): n = 64*m + 16*a + b with 32 registers m,
// output k = k1 + 32*k2 + 128*k3.  Steps 1-4 as above with radix 32 and eight register quads (twiddle W_128^(a*k1),
// exchange slot 129*b + l', l' = k1 + 32*k2 < 128); in step 5 every lane takes TWO columns l' = lane + 64*s, s = 0, 1
// (twiddle W_2048^(b*l'), radix-16 over b) and leaves X[lane + 64*(s + 2*k3)] in register s + 2*k3 -- the natural slot
// order.  tw2[(3*c + i-1)*4 + j] = W_128^(i*(4c+j)) (c < 8), tw3[l'] = W_2048^(l'), l' < 128.
// tests/kernel_model.py::fft2048_rowswap_model is the index-for-index numpy model.
__device__ __forceinline__ void fft2048_rowswap(v2f* z, int lane, v2f* xch, const v2f* tw2, const v2f* tw3, FusedProbe& pr) {
  const int j = lane >> 4, b = lane & 15;
  fft_reg<32, true>(z);  // 1.
  FDOCT_FPR(pr, 3);
  static_for<0, 8>([&](auto cc) {  // 2.
    constexpr int c = decltype(cc)::value;
    float x0 = z[4 * c].x, y0 = z[4 * c].y, x1 = z[4 * c + 1].x, y1 = z[4 * c + 1].y;
    float x2 = z[4 * c + 2].x, y2 = z[4 * c + 2].y, x3 = z[4 * c + 3].x, y3 = z[4 * c + 3].y;
    swap_rows32(x0, x2);
    swap_rows32(y0, y2);
    swap_rows32(x1, x3);
    swap_rows32(y1, y3);
    swap_rows16(x0, x1);
    swap_rows16(y0, y1);
    swap_rows16(x2, x3);
    swap_rows16(y2, y3);
    z[4 * c] = mk(x0, y0);
    z[4 * c + 1] = mk(x1, y1);
    z[4 * c + 2] = mk(x2, y2);
    z[4 * c + 3] = mk(x3, y3);
  });
  FDOCT_FPR(pr, 4);
  // 3. + 4.: register 4c+i of lane (j,b) holds A[k1 = 4c+j][a = i][b]
  v2f* dst = xch + (129 * b + j);
  static_for<0, 8>([&](auto cc) {
    constexpr int c = decltype(cc)::value;
    const v2f* t2 = tw2 + (3 * c) * 4 + j;
    v2f v[4] = {z[4 * c], cmul(z[4 * c + 1], t2[0]), cmul(z[4 * c + 2], t2[4]), cmul(z[4 * c + 3], t2[8])};
    fft_reg<4, true>(v);
    static_for<0, 4>([&](auto kc) {
      constexpr int k2 = decltype(kc)::value;
      dst[4 * c + 32 * k2] = v[k2];
    });
  });
  wave_lds_sync();
  FDOCT_FPR(pr, 5);
  // 5. two columns per lane; the second one is read while the first is being transformed
  const v2f* src = xch + lane;
  v2f u[16], w[16];
  static_for<0, 16>([&](auto bc) {
    constexpr int bb = decltype(bc)::value;
    u[bb] = src[129 * bb];
  });
  static_for<0, 16>([&](auto bc) {
    constexpr int bb = decltype(bc)::value;
    w[bb] = src[129 * bb + 64];
  });
  wave_lds_sync();
  FDOCT_FPR(pr, 6);
  // W_2048^(bb*l'), bb = 1..15, as powers of the one table entry W_2048^(l') (squarings / products, depth <= 6
  // multiplies): 15 KB less LDS per workgroup than a full table, which is worth a wave per CU here
  auto column = [&](v2f* col, v2f w1) {
    v2f pw[16];
    pw[1] = w1;
    static_for<2, 16>([&](auto rc) {
      constexpr int r = decltype(rc)::value;
      pw[r] = (r & 1) ? cmul(pw[r - 1], pw[1]) : cmul(pw[r / 2], pw[r / 2]);
    });
    static_for<1, 16>([&](auto bc) {
      constexpr int bb = decltype(bc)::value;
      col[bb] = cmul(col[bb], pw[bb]);
    });
    fft_reg<16, true>(col);
  };
  column(u, tw3[lane]);
  column(w, tw3[lane + 64]);
  static_for<0, 16>([&](auto kc) {
    constexpr int k3 = decltype(kc)::value;
    z[2 * k3] = u[k3];
    z[2 * k3 + 1] = w[k3];
  });
  FDOCT_FPR(pr, 7);
}

}  // namespace fdoct
