// fdoct_roi.cpp -- the extern "C" entry points of include/fdoct_roi.h: the B-scan readouts (A-scan min / max, ROI mean,
// peak hold and the vibration readout of BscanFFTpeak.cpp) over the kernels of fdoct_roi.hip.
#include "../../include/fdoct_roi.h"

#include <limits>

#include "fdoct_ctx.h"
#include "fdoct_roi_kernels.h"

using namespace fdoct_impl;

namespace {

// besseldbinverse, BscanFFTpeak.cpp:243-395, as it stands: x = kBinvX[i] for the first i with y > kBinvT[i], else 0.
constexpr double kBinvT[] = {30,      25,      21.65,   19.2,    17.18,   15.56,   14.19,   13,      11.94,   11,
                             10.15,   9.37,    8.66,    8,       7.4,     6.83,    6.30,    5.82,    5.36,    4.931,
                             4.528,   4.151,   3.797,   3.464,   3.151,   2.858,   2.583,   2.3245,  2.08286, 1.85689,
                             1.64601, 1.44964, 1.26729, 1.09850, 0.94288, 0.80006, 0.66972, 0.55159, 0.44542, 0.35097,
                             0.26807, 0.19654, 0.13625, 0.08708, 0.04893, 0.02173, 0.00543};
constexpr double kBinvX[] = {2.38, 2.33, 2.27, 2.22, 2.17, 2.12, 2.07, 2.02, 1.97, 1.92, 1.87, 1.82, 1.77, 1.72, 1.67, 1.62,
                             1.57, 1.52, 1.47, 1.42, 1.37, 1.32, 1.27, 1.22, 1.17, 1.12, 1.07, 1.02, 0.97, 0.92, 0.87, 0.82,
                             0.77, 0.72, 0.67, 0.62, 0.57, 0.52, 0.47, 0.42, 0.37, 0.32, 0.27, 0.22, 0.17, 0.12, 0.07};
static_assert(sizeof(kBinvT) == sizeof(kBinvX), "one output per threshold");

double besseldbinverse(double y) {
  for (size_t i = 0; i < sizeof(kBinvT) / sizeof(kBinvT[0]); i++)
    if (y > kBinvT[i]) return kBinvX[i];
  return 0.0;
}

// the displacement of one J0 argument, in the reference's order of operations: x * lambda0 * 1e9 / (4 * pi)
double x_to_nm(double x, float lambda0) { return x * lambda0 * 1e9 / (4 * kPi); }

size_t image_bytes(int nbscans, int depths, int ascans) { return (size_t)nbscans * depths * ascans * sizeof(float); }
// The image a kernel reads once the call's staging plan is reserved: the caller's device pointer, or a host batch's device copy.
RoiImage image_of(const StagePlan& sp, int item, fdoct_layout layout, int nbscans, int depths, int ascans) {
  return RoiImage{sp.dev<const float>(item), nbscans, depths, ascans, layout == FDOCT_LAYOUT_TRANSPOSED_DxH};
}

int check_image(fdoct_ctx* h, const char* fn, const float* bscandb, fdoct_memspace mem, fdoct_layout layout, int nbscans,
                int depths, int ascans) {
  if (!bscandb || !valid_mem(mem) || !valid_layout(layout) || nbscans <= 0 || depths <= 0 || ascans <= 0)
    return fail(h, FDOCT_ERR_INVALID, std::string(fn) + ": bad arguments");
  return FDOCT_OK;
}

bool valid_slot(int slot) { return slot >= 1 && slot <= 4; }

// Reads the holds of every slot: cols (4 * roi.w floats, when an ROI is set) and scalars (4 floats).  Synchronises.
int read_holds(fdoct_ctx* h, std::vector<float>* cols, float scalars[4]) {
  std::vector<uint32_t> c(h->roi.set ? 4 * (size_t)h->roi.w : 0), s(4, kRoiHoldZero);
  if (!c.empty()) HIP_TRY(h, hipMemcpyAsync(c.data(), h->d_hold_cols, c.size() * 4, hipMemcpyDeviceToHost, h->stream));
  if (h->d_hold_scalar) HIP_TRY(h, hipMemcpyAsync(s.data(), h->d_hold_scalar, 16, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  cols->resize(c.size());
  for (size_t i = 0; i < c.size(); i++) (*cols)[i] = roi_decode(c[i]);
  for (int i = 0; i < 4; i++) scalars[i] = roi_decode(s[i]);
  return FDOCT_OK;
}

// The four scalar holds exist from the first ROI or clear on and are never reallocated (setting an ROI keeps them).
int ensure_scalar_holds(fdoct_ctx* h) {
  if (h->d_hold_scalar) return FDOCT_OK;
  if (int rc = h->d_hold_scalar.assign(h, 4)) return rc;
  HIP_TRY(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(static_cast<uint32_t*>(h->d_hold_scalar)), kRoiHoldZero, 4,
                               h->stream));
  return FDOCT_OK;
}

}  // namespace

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_ascan_minmax(fdoct_handle h, const float* bscandb, fdoct_memspace mem, fdoct_layout layout, int nbscans,
                       int depths, int ascans, int ascanat, float* out_min, float* out_max, fdoct_memspace out_mem) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (int rc = check_image(h, "fdoct_ascan_minmax", bscandb, mem, layout, nbscans, depths, ascans)) return rc;
  if (!valid_mem(out_mem) || (!out_min && !out_max)) return fail(h, FDOCT_ERR_INVALID, "fdoct_ascan_minmax: no output");
  if (depths < 5) return fail(h, FDOCT_ERR_INVALID, "fdoct_ascan_minmax: needs depths >= 5 (rows 0-3 read as row 4)");
  if (ascanat < 0 || ascanat >= ascans) return fail(h, FDOCT_ERR_INVALID, "fdoct_ascan_minmax: ascanat outside the image");
  DEVICE_SCOPE(h);
  StagePlan sp;
  const int in = sp.in(bscandb, mem, image_bytes(nbscans, depths, ascans));
  const int lo = sp.out_or_scratch(out_min, out_mem, nbscans * sizeof(float)), hi = sp.out_or_scratch(out_max, out_mem, nbscans * sizeof(float));
  if (int rc = stage_begin(h, &sp)) return rc;
  const RoiImage im = image_of(sp, in, layout, nbscans, depths, ascans);
  HIP_TRY(h, launch_roi_ascan_minmax(im, ascanat, sp.dev<float>(lo), sp.dev<float>(hi), h->num_cu, h->stream));  // (writes both: a missing one is scratch)
  return stage_finish(h, sp);
} FDOCT_CATCH(h)

int fdoct_roi_mean(fdoct_handle h, const float* bscandb, fdoct_memspace mem, fdoct_layout layout, int nbscans, int depths,
                   int ascans, int ascanat, int vertpos, int width, double* out_mean, fdoct_memspace out_mem) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (int rc = check_image(h, "fdoct_roi_mean", bscandb, mem, layout, nbscans, depths, ascans)) return rc;
  if (!out_mean || !valid_mem(out_mem)) return fail(h, FDOCT_ERR_INVALID, "fdoct_roi_mean: no output");
  if (ascanat < 0 || width < 1 || (long long)ascanat + width >= ascans)  // the reference's strict guard, BscanFFT.cpp:107
    return fail(h, FDOCT_ERR_INVALID, "fdoct_roi_mean: needs ascanat + width < ascans (BscanFFT.cpp:107)");
  if (vertpos < 0 || (long long)vertpos + 3 > depths) return fail(h, FDOCT_ERR_INVALID, "fdoct_roi_mean: the 3 depth rows do not fit");
  DEVICE_SCOPE(h);
  StagePlan sp;
  const int in = sp.in(bscandb, mem, image_bytes(nbscans, depths, ascans)), out = sp.out(out_mean, out_mem, nbscans * sizeof(double));
  if (int rc = stage_begin(h, &sp)) return rc;
  HIP_TRY(h, launch_roi_mean(image_of(sp, in, layout, nbscans, depths, ascans), ascanat, vertpos, width, sp.dev<double>(out), h->num_cu, h->stream));
  return stage_finish(h, sp);
} FDOCT_CATCH(h)

int fdoct_set_peakhold_roi(fdoct_handle h, int x, int y, int w, int hgt, int ascanat) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (x < 0 || y < 0 || w < 1 || hgt < 1 || ascanat < 0) return fail(h, FDOCT_ERR_INVALID, "fdoct_set_peakhold_roi: bad ROI");
  DEVICE_SCOPE(h);
  if (int rc = ensure_scalar_holds(h)) return rc;
  if (w != h->roi.w || !h->d_hold_cols) {
    h->roi.set = false;  // (until the column holds exist)
    if (int rc = h->d_hold_cols.assign(h, 4 * (size_t)w)) return rc;
  }
  HIP_TRY(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(static_cast<uint32_t*>(h->d_hold_cols)), kRoiHoldZero,
                               4 * (size_t)w, h->stream));
  h->roi = {x, y, w, hgt, ascanat, true};
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_peakhold(fdoct_handle h, int slot, const float* bscandb, fdoct_memspace mem, fdoct_layout layout, int nbscans,
                   int depths, int ascans) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!valid_slot(slot)) return fail(h, FDOCT_ERR_INVALID, "fdoct_peakhold: slot must be 1..4");
  if (int rc = check_image(h, "fdoct_peakhold", bscandb, mem, layout, nbscans, depths, ascans)) return rc;
  if (!h->roi.set) return fail(h, FDOCT_ERR_STATE, "fdoct_peakhold: no ROI set (fdoct_set_peakhold_roi)");
  const auto& r = h->roi;
  if ((long long)r.x + r.w > ascans || (long long)r.y + r.h > depths || r.ascanat >= ascans)
    return fail(h, FDOCT_ERR_INVALID, "fdoct_peakhold: the ROI or ascanat lies outside the image");
  DEVICE_SCOPE(h);
  StagePlan sp;
  const int in = sp.in(bscandb, mem, image_bytes(nbscans, depths, ascans));
  if (int rc = stage_begin(h, &sp)) return rc;
  uint32_t* cols = static_cast<uint32_t*>(h->d_hold_cols) + (size_t)(slot - 1) * r.w;
  uint32_t* scalar = static_cast<uint32_t*>(h->d_hold_scalar) + (slot - 1);
  HIP_TRY(h, launch_roi_hold(image_of(sp, in, layout, nbscans, depths, ascans), r.x, r.y, r.w, r.h, r.ascanat, cols, scalar, h->num_cu, h->stream));
  h->hold_count[slot - 1] += nbscans;
  return stage_finish(h, sp);
} FDOCT_CATCH(h)

int fdoct_get_peakhold(fdoct_handle h, int slot, float* colmax, float* ascanmax, long long* held_bscans) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!valid_slot(slot)) return fail(h, FDOCT_ERR_INVALID, "fdoct_get_peakhold: slot must be 1..4");
  if (colmax && !h->roi.set) return fail(h, FDOCT_ERR_STATE, "fdoct_get_peakhold: no ROI set (fdoct_set_peakhold_roi)");
  DEVICE_SCOPE(h);
  std::vector<float> cols;
  float scalars[4];
  if (int rc = read_holds(h, &cols, scalars)) return rc;
  if (colmax) std::copy(cols.begin() + (size_t)(slot - 1) * h->roi.w, cols.begin() + (size_t)slot * h->roi.w, colmax);
  if (ascanmax) *ascanmax = scalars[slot - 1];
  if (held_bscans) *held_bscans = h->hold_count[slot - 1];
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_clear_peakhold(fdoct_handle h, int slot) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!valid_slot(slot)) return fail(h, FDOCT_ERR_INVALID, "fdoct_clear_peakhold: slot must be 1..4");
  DEVICE_SCOPE(h);
  if (int rc = ensure_scalar_holds(h)) return rc;
  HIP_TRY(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(static_cast<uint32_t*>(h->d_hold_scalar) + (slot - 1)),
                               kRoiHoldZero, 1, h->stream));
  if (h->roi.set)
    HIP_TRY(h, hipMemsetD32Async(
                   reinterpret_cast<hipDeviceptr_t>(static_cast<uint32_t*>(h->d_hold_cols) + (size_t)(slot - 1) * h->roi.w),
                   kRoiHoldZero, h->roi.w, h->stream));
  h->hold_count[slot - 1] = 0;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_vibration_profile(fdoct_handle h, int mode, double lambda0, double* profile_nm, double* disp_nm, double* err_nm) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (mode != 3 && mode != 4) return fail(h, FDOCT_ERR_INVALID, "fdoct_vibration_profile: mode must be 3 or 4");
  if (!h->roi.set) return fail(h, FDOCT_ERR_STATE, "fdoct_vibration_profile: no ROI set (fdoct_set_peakhold_roi)");
  DEVICE_SCOPE(h);
  std::vector<float> cols;
  float mx[4];
  if (int rc = read_holds(h, &cols, mx)) return rc;
  // float lambda0 = (lambdamin + lambdamax) / 2, BscanFFTpeak.cpp:1151
  const float l0 = lambda0 > 0 ? (float)lambda0 : (float)((h->cfg.lambdamin + h->cfg.lambdamax) / 2);
  const int w = h->roi.w;
  auto col = [&](int slot, int i) { return (double)cols[(size_t)(slot - 1) * w + i]; };
  const double max1 = mx[0], max2 = mx[1], max3 = mx[2], max4 = mx[3];
  if (mode == 3) {  // 597-644
    if (disp_nm) *disp_nm = x_to_nm(besseldbinverse(max1 - max3), l0);
    if (err_nm) *err_nm = x_to_nm(2.405 - besseldbinverse(max1 - max2), l0);  // errnull, 397-415
    if (profile_nm)
      for (int i = 0; i < w; i++) profile_nm[i] = x_to_nm(besseldbinverse(col(1, i) - col(3, i)), l0);
  } else {  // 681-731
    if (disp_nm) *disp_nm = x_to_nm(besseldbinverse(max1 - max4), l0);
    if (err_nm) *err_nm = std::numeric_limits<double>::quiet_NaN();
    if (profile_nm)
      for (int i = 0; i < w; i++)
        profile_nm[i] = x_to_nm(besseldbinverse(col(1, i) - col(3, i)), l0) - x_to_nm(besseldbinverse(col(1, i) - col(4, i)), l0);
  }
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_besseldb_inverse(const double* y, int n, double* x) try {
  if (n < 0 || (n > 0 && (!y || !x))) return FDOCT_ERR_INVALID;
  for (int i = 0; i < n; i++) x[i] = besseldbinverse(y[i]);
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

}  // extern "C"
