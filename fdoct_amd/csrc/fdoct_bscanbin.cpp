// fdoct_bscanbin.cpp -- the extern "C" entry points of include/fdoct_bscanbin.h: spinjnt's output binning
// (BscanFFTspinjnt.cpp:1856-1861 and the log behind it) over the kernel of fdoct_bscanbin.hip.
#include "../../include/fdoct_bscanbin.h"

#include "fdoct_bscanbin_kernels.h"
#include "fdoct_ctx.h"

using namespace fdoct_impl;

namespace {

// The geometry's checks, shared by fdoct_bscanbin_size and fdoct_bscan_bin.  h may be null (the host-only entry point).
int check_geometry(fdoct_ctx* h, const char* fn, int depths, int ascans, int binx, int biny, int upx, int upy) {
  const std::string f(fn);
  if (depths <= 0 || ascans <= 0) return fail(h, FDOCT_ERR_INVALID, f + ": bad image size");
  if (binx < 1 || binx > fdoct::kBinMaxFactor || biny < 1 || biny > fdoct::kBinMaxFactor)
    return fail(h, FDOCT_ERR_INVALID, f + ": binx and biny must be 1..16");
  if (upx < 1 || upx > fdoct::kBinMaxUp || upy < 1 || upy > fdoct::kBinMaxUp)
    return fail(h, FDOCT_ERR_INVALID, f + ": upx and upy must be 1..64");
  if (depths % biny || ascans % binx)  // INTER_AREA leaves its integer-factor path (BscanFFTspinjnt.cpp:1859)
    return fail(h, FDOCT_ERR_UNSUPPORTED, f + ": depths must be a multiple of biny and ascans of binx");
  if ((long long)(depths / biny) * upy > (1 << 30) || (long long)(ascans / binx) * upx > (1 << 30))
    return fail(h, FDOCT_ERR_INVALID, f + ": the result is too large");
  return FDOCT_OK;
}

// The device's tap table follows the up factors of the last call.  A change waits for the kernels that still read the old one.
int ensure_taps(fdoct_ctx* h, int upx, int upy) {
  if (h->d_bin_taps && h->bin_taps_upx == upx && h->bin_taps_upy == upy) return FDOCT_OK;
  std::vector<double> t(fdoct::kBinTapDoubles, 0.0);
  fdoct::bscanbin_build_taps(upx, t.data());
  fdoct::bscanbin_build_taps(upy, t.data() + fdoct::kBinMaxUp * fdoct::kBinTapStride);
  if (int rc = h->d_bin_taps.reserve(h, t.size() * sizeof(double))) return rc;
  h->bin_taps_upx = h->bin_taps_upy = 0;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(h->d_bin_taps, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
  h->bin_taps_upx = upx, h->bin_taps_upy = upy;
  return FDOCT_OK;
}

}  // namespace

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_bscanbin_size(int depths, int ascans, int binx, int biny, int upx, int upy, int* out_depths, int* out_ascans) try {
  if (!out_depths || !out_ascans) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_bscanbin_size: no output");
  if (int rc = check_geometry(nullptr, "fdoct_bscanbin_size", depths, ascans, binx, biny, upx, upy)) return rc;
  *out_depths = depths / biny * upy;
  *out_ascans = ascans / binx * upx;
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_bscanbin_taps(int up, double* taps4, int* first_src_offset) try {
  if (up < 1 || up > fdoct::kBinMaxUp || !taps4) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_bscanbin_taps: bad arguments");
  double t[fdoct::kBinMaxUp * fdoct::kBinTapStride];
  fdoct::bscanbin_build_taps(up, t);
  for (int p = 0; p < up; p++) {
    for (int i = 0; i < 4; i++) taps4[4 * p + i] = t[fdoct::kBinTapStride * p + i];
    if (first_src_offset) first_src_offset[p] = (int)t[fdoct::kBinTapStride * p + 4];
  }
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_bscan_bin(fdoct_handle h, const float* bscan, const float* jscan, fdoct_memspace mem, fdoct_layout layout, int nbscans,
                    int depths, int ascans, int binx, int biny, int upx, int upy, double multiplyfactor, float* out_bscan,
                    float* out_db, fdoct_memspace out_mem) try {
  // what needs no handle first: a bad call is refused the same way with and without a device
  if (!bscan || !valid_mem(mem) || !valid_mem(out_mem) || !valid_layout(layout) || nbscans <= 0)
    return fail(h, FDOCT_ERR_INVALID, "fdoct_bscan_bin: bad arguments");
  if (!out_bscan && !out_db) return fail(h, FDOCT_ERR_INVALID, "fdoct_bscan_bin: no output");
  if (!std::isfinite(multiplyfactor)) return fail(h, FDOCT_ERR_INVALID, "fdoct_bscan_bin: multiplyfactor is not finite");
  if (int rc = check_geometry(h, "fdoct_bscan_bin", depths, ascans, binx, biny, upx, upy)) return rc;
  const int od = depths / biny * upy, oa = ascans / binx * upx;
  const size_t image = (size_t)depths * ascans, in_floats = image * nbscans, out_floats = (size_t)od * oa * nbscans;
  if (in_floats > ((size_t)1 << 40) || out_floats > ((size_t)1 << 40)) return fail(h, FDOCT_ERR_INVALID, "fdoct_bscan_bin: the batch is too large");
  if (overlap(out_bscan, out_floats * 4, out_db, out_floats * 4) ||
      (mem == out_mem && (overlap(bscan, in_floats * 4, out_bscan, out_floats * 4) || overlap(bscan, in_floats * 4, out_db, out_floats * 4) ||
                          overlap(jscan, image * 4, out_bscan, out_floats * 4) || overlap(jscan, image * 4, out_db, out_floats * 4))))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_bscan_bin: input and output buffers overlap");
  if (!h) return FDOCT_ERR_INVALID;
  DEVICE_SCOPE(h);

  fdoct::BscanBinArgs a;
  a.nb = nbscans;
  a.transposed = layout == FDOCT_LAYOUT_TRANSPOSED_DxH;
  if (a.transposed) {  // memory rows are depths
    a.R = depths, a.C = ascans, a.binr = biny, a.binc = binx, a.upr = upy, a.upc = upx;
  } else {
    a.R = ascans, a.C = depths, a.binr = binx, a.binc = biny, a.upr = upx, a.upc = upy;
  }
  a.NR = a.R / a.binr, a.NC = a.C / a.binc, a.OR = a.NR * a.upr, a.OC = a.NC * a.upc;
  a.in_bs = (long long)image, a.out_bs = (long long)od * oa;
  a.mask = !jscan && h->cfg.dc_mask && od > 4;                            // 1873-1874; none behind the lock-in (1902-1903)
  a.eps = (double)chain_eps(h);
  a.inv_area = 1.0 / ((double)binx * biny);
  a.mf = multiplyfactor;

  // everything that can fail without the kernel comes before anything is enqueued: workspaces, the tap table
  StagePlan sp;
  const int in = sp.in(bscan, mem, in_floats * sizeof(float)), js = sp.in(jscan, mem, image * sizeof(float));
  const int lin = sp.out(out_bscan, out_mem, out_floats * sizeof(float)), db = sp.out(out_db, out_mem, out_floats * sizeof(float));
  if (int rc = stage_reserve(h, &sp)) return rc;
  if (int rc = ensure_taps(h, upx, upy)) return rc;
  a.taps = h->d_bin_taps, a.in = sp.dev<const float>(in), a.jscan = sp.dev<const float>(js);
  a.out_lin = sp.dev<float>(lin), a.out_db = sp.dev<float>(db);
  fdoct::bscanbin_plan(&a, h->num_cu);
  if (a.blocks < 1 || a.lds_bytes > 64 * 1024)  // (no factors within the limits get here: 32 x 128 outputs need 45 KiB at most)
    return fail(h, FDOCT_ERR_UNSUPPORTED, "fdoct_bscan_bin: the tile does not fit a workgroup's LDS");
  if (int rc = stage_upload(h, sp)) return rc;
  HIP_TRY(h, fdoct::launch_bscan_bin(a, h->stream));
  return stage_finish(h, sp);
} FDOCT_CATCH(h)

}  // extern "C"
