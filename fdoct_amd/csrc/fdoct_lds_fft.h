// fdoct_lds_fft.h -- a complex transform of n points inside one workgroup's LDS, as a value and as device code: mixed-radix
// Stockham passes over two ping-pong buffers, radices 16 / 8 / 4 / 2 / 5 / 3 with the butterflies in registers (fdoct_fft_reg.h).
// These are the passes of fdoct_dispersion.hip (and, before it, fdoct_generic.hip) written out for a second user,
// fdoct_ssada.hip; the dispersion kernel keeps its own copy until the two are joined.  Internal.
//   Butterfly j of a pass reads src[j + r nb], so a wave's lanes read consecutive pairs; its stores are Ns apart per register and,
// in the first pass, R apart across lanes, which is why the radix plan puts an odd or small radix first (fdoct_plan.cpp).
#pragma once
#include <hip/hip_runtime.h>

namespace fdoct {

constexpr int kLdsFftMaxPasses = 16;

// The transform as the kernels take it: the Stockham radices of n (fdoct_plan.cpp's factorisation) and, per pass,
// magic = ceil(2^32 / Ns), Ns the product of the radices in front of it (0 for the first pass).
struct LdsFftPlan {
  int n = 0, npass = 0;
  int rad[kLdsFftMaxPasses] = {};
  unsigned magic[kLdsFftMaxPasses] = {};
};

// Fills the plan from the radices; false where there are none or too many, or one is not a butterfly this header has.
inline bool lds_fft_plan(LdsFftPlan* p, int n, const int* rad, int npass) {
  if (npass < 1 || npass > kLdsFftMaxPasses) return false;
  p->n = n, p->npass = npass;
  unsigned long long Ns = 1;
  for (int i = 0; i < npass; i++) {
    const int R = rad[i];
    if (R != 16 && R != 8 && R != 4 && R != 2 && R != 5 && R != 3) return false;
    p->rad[i] = R;
    p->magic[i] = Ns > 1 ? (unsigned)(((1ull << 32) + Ns - 1) / Ns) : 0u;
    Ns *= (unsigned)R;
  }
  return Ns == (unsigned long long)n;
}

}  // namespace fdoct

#ifdef __HIPCC__
#include "fdoct_fft_reg.h"

namespace fdoct {

// One Stockham pass of radix R by a workgroup of BLOCK threads: butterfly j takes src[j + r nb], multiplies by
// exp(+-2 pi i r k / (Ns R)) (k = j mod Ns; tw[m] = exp(+2 pi i m / n)), transforms in registers and writes
// dst[(j div Ns) Ns R + k + r Ns].  j div Ns by multiplication: magic = ceil(2^32 / Ns) is exact for j, Ns < 2^16.
template <int R, bool INV, int BLOCK>
__device__ __forceinline__ void lds_fft_pass(const v2f* src, v2f* dst, int n, int Ns, unsigned magic, const v2f* tw) {
  const int nb = n / R;
  const int twstep = nb / Ns;
  for (int j = threadIdx.x; j < nb; j += BLOCK) {
    int q = j, k = 0;
    if (Ns > 1) {
      q = (int)__umulhi((unsigned)j, magic);
      k = j - q * Ns;
    }
    v2f v[R];
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = src[j + r * nb];
    if (Ns > 1) {
      v2f w[R];
      w[1] = tw[k * twstep];
      if (!INV) w[1].y = -w[1].y;
#pragma unroll
      for (int r = 2; r < R; r++) w[r] = (r & 1) ? cmul(w[r - 1], w[1]) : cmul(w[r / 2], w[r / 2]);
#pragma unroll
      for (int r = 1; r < R; r++) v[r] = cmul(v[r], w[r]);
    }
    if constexpr (R == 3)
      fft_reg3<INV>(v);
    else if constexpr (R == 5)
      fft_reg5<INV>(v);
    else
      fft_reg<R, INV>(v);
    v2f* d = dst + (q * Ns * R + k);
#pragma unroll
    for (int r = 0; r < R; r++) d[r * Ns] = v[r];
  }
}

// The transform over the two buffers, src holding the input behind a barrier; returns the buffer that holds the result.  Ends
// behind a barrier.
template <bool INV, int BLOCK>
__device__ v2f* lds_fft(v2f* src, v2f* dst, const LdsFftPlan& p, const v2f* tw) {
  int Ns = 1;
  for (int i = 0; i < p.npass; i++) {
    const int R = p.rad[i];
    const unsigned magic = p.magic[i];
    switch (R) {
      case 16: lds_fft_pass<16, INV, BLOCK>(src, dst, p.n, Ns, magic, tw); break;
      case 8: lds_fft_pass<8, INV, BLOCK>(src, dst, p.n, Ns, magic, tw); break;
      case 4: lds_fft_pass<4, INV, BLOCK>(src, dst, p.n, Ns, magic, tw); break;
      case 2: lds_fft_pass<2, INV, BLOCK>(src, dst, p.n, Ns, magic, tw); break;
      case 5: lds_fft_pass<5, INV, BLOCK>(src, dst, p.n, Ns, magic, tw); break;
      default: lds_fft_pass<3, INV, BLOCK>(src, dst, p.n, Ns, magic, tw); break;
    }
    __syncthreads();
    v2f* t = src;
    src = dst;
    dst = t;
    Ns *= R;
  }
  return src;
}

}  // namespace fdoct
#endif  // __HIPCC__
