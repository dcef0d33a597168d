// fdoct_ssada.cpp -- the extern "C" entry points of include/fdoct_ssada.h (libfdoct_ssada.so): split-spectrum amplitude
// decorrelation from repeated complex B-scans.  The split and mean kernels are fdoct_ssada.hip's, the window stage between them is
// fdoct_angio.hip's launch_angio (its object is linked into this library); the chain in front of fdoct_process_ssada is the core
// library's (fdoct_route.cpp: enqueue_complex), called in the order fdoct_capture_plan.h's ComplexFront keeps; the transform's
// radices are the planner's (fdoct_plan.cpp: make_plan on a complex row of n points).  What is this file's own is the calls'
// arguments: the parameters' refusals, the passes over the workspace (plan_ssada; fdoct_ssada_plan reports them), and pairs,
// frames and the outputs in host or device memory -- the three float outputs through the staging plan, a host-memory out_bands
// pass by pass from the workspace itself.
#include "../../include/fdoct_ssada.h"

#include <cmath>
#include <cstddef>

#include "fdoct_angio_kernels.h"
#include "fdoct_capture_plan.h"
#include "fdoct_ssada_kernels.h"

using namespace fdoct_impl;

static_assert(FDOCT_SSADA_MAX_WIN == fdoct::kSsaMaxWin && FDOCT_SSADA_MAX_REPEATS == fdoct::kSsaMaxRepeats && FDOCT_SSADA_MAX_BANDS == fdoct::kSsaMaxBands,
              "the header's limits are the kernels'");
static_assert(fdoct::kSsaMaxWin == fdoct::kAngMaxWin && fdoct::kSsaMaxRepeats == fdoct::kAngMaxRepeats && fdoct::kSsaMinRepeats == fdoct::kAngMinRepeats &&
                  fdoct::kSsaMaxBandFrames == fdoct::kAngMaxFrames && fdoct::kSsaMaxPixels == fdoct::kAngMaxPixels,
              "the window stage is angiography's: its limits are this stage's");

namespace {

// The Stockham radices of a complex row of n points, as the workgroup-per-row kernel would take it: empty where the planner has
// none (a prime factor above 5).
std::vector<int> radices_of(int n) {
  fdoct::PlanInputs in;
  in.W = n, in.M = 1, in.N = n, in.D = n, in.phase = true, in.plan_override = -2;
  fdoct::Plan p;
  std::string why;
  if (fdoct::make_plan(in, &p, &why) != FDOCT_OK || p.gen.blu_m || (int)p.gen.rad_n.size() > fdoct::kLdsFftMaxPasses) return {};
  return p.gen.rad_n;
}

// A call's sizes in bytes and its passes.
struct SsaPlan {
  size_t in = 0;            // the pairs of the whole call
  size_t floats = 0;        // one [groups][ascans][Dc] float image batch
  size_t band_floats = 0;   // one [groups][M][ascans][Dc] float image batch
  size_t bands = 0;         // out_bands
  size_t group_pairs = 0;   // a group's band pairs, bytes
  size_t group_floats = 0;  // a group's d (or p), bytes
  size_t tab = 0;
  int groups = 0, groups_per_pass = 0, passes = 0;   // with the pairs in the workspace
  size_t workspace = 0;     // groups_per_pass (group_pairs + 2 group_floats)
};

// The resolved support of the bands: false where it does not lie in [0, n) or holds no bin.
bool support_range(int first, int count, int n, int* resolved) {
  if (first < 0 || first >= n || count < 0 || count > n - first) return false;
  *resolved = count ? count : n - first;
  return true;
}

// What every entry point decides from the parameters and the images' shape: the refusals, then the kernels' arguments without
// their pointers and for all groups at once, and the sizes.  h may be null (fdoct_ssada_plan, fdoct_ssada_band_table).
int plan_ssada(fdoct_ctx* h, const char* fn, const fdoct_ssada_params* p, int nframes, int ascans, int n, fdoct::SsadaArgs* a, SsaPlan* s) {
  const std::string f(fn);
  if (!p) return fail(h, FDOCT_ERR_INVALID, f + ": no parameters");
  if (n < 1) return fail(h, FDOCT_ERR_INVALID, f + ": n must be at least 1");
  if (n < fdoct::kSsaMinN || n > fdoct::kSsaMaxN) return fail(h, FDOCT_ERR_UNSUPPORTED, f + ": A-scans of fewer than 16 or more than 4096 points");
  const std::vector<int> rad = radices_of(n);
  if (rad.empty() || !fdoct::lds_fft_plan(&a->fft, n, rad.data(), (int)rad.size())) return fail(h, FDOCT_ERR_UNSUPPORTED, f + ": n has a prime factor above 5");
  if (p->repeats < fdoct::kSsaMinRepeats || p->repeats > fdoct::kSsaMaxRepeats) return fail(h, FDOCT_ERR_INVALID, f + ": repeats must be 2..64");
  if (p->bands < 1 || p->bands > fdoct::kSsaMaxBands) return fail(h, FDOCT_ERR_INVALID, f + ": bands must be 1..16");
  if (nframes < 1 || nframes % p->repeats || (long long)nframes * p->bands > fdoct::kSsaMaxBandFrames)
    return fail(h, FDOCT_ERR_INVALID, f + ": nframes must be a positive multiple of repeats, and nframes times bands at most 65536");
  if (ascans < 1) return fail(h, FDOCT_ERR_INVALID, f + ": ascans must be at least 1");
  if (!std::isfinite(p->sigma) || !(p->sigma > 0.0)) return fail(h, FDOCT_ERR_INVALID, f + ": sigma must be finite and greater than 0");
  int k_count = 0;
  if (!support_range(p->k_first, p->k_count, n, &k_count)) return fail(h, FDOCT_ERR_INVALID, f + ": the bands' support must lie in [0, n)");
  if (p->depth_first < 0 || p->depth_first >= n || p->depth_count < 0 || p->depth_count > n - p->depth_first)
    return fail(h, FDOCT_ERR_INVALID, f + ": the depth range must lie in [0, n)");
  const int dc = p->depth_count ? p->depth_count : n / 2 - p->depth_first;
  if (dc < 1) return fail(h, FDOCT_ERR_INVALID, f + ": the depth range holds no bin");
  if ((long long)ascans * dc > fdoct::kSsaMaxPixels) return fail(h, FDOCT_ERR_INVALID, f + ": ascans times the depths kept must not exceed 2^24");
  if (p->win_ascans < 1 || p->win_ascans > fdoct::kSsaMaxWin || p->win_depths < 1 || p->win_depths > fdoct::kSsaMaxWin)
    return fail(h, FDOCT_ERR_INVALID, f + ": win_ascans and win_depths must be 1..16");
  if (!std::isfinite(p->min_power) || p->min_power < 0.0) return fail(h, FDOCT_ERR_INVALID, f + ": min_power must be finite and not negative");

  a->groups = nframes / p->repeats, a->repeats = p->repeats, a->ascans = ascans, a->nbands = p->bands;
  a->depth_first = p->depth_first, a->depth_count = dc;
  a->k_first = p->k_first, a->k_count = k_count;
  a->sigma = p->sigma;
  a->min_power = (float)p->min_power;
  fdoct::ssada_plan_launch(a, h ? h->num_cu : 0);

  const size_t pixels = (size_t)ascans * (size_t)dc;                  // <= 2^24
  const size_t band_images = (size_t)a->groups * (size_t)p->bands;    // <= 2^16
  size_t pairs = 0;
  if (__builtin_mul_overflow((size_t)nframes * (size_t)ascans, (size_t)n, &pairs) || __builtin_mul_overflow(pairs, sizeof(float2), &s->in) ||
      __builtin_mul_overflow((size_t)nframes * (size_t)p->bands * pixels, sizeof(float2), &s->bands))
    return fail(h, FDOCT_ERR_INVALID, f + ": the batch's size does not fit size_t");
  s->floats = (size_t)a->groups * pixels * sizeof(float);
  s->band_floats = band_images * pixels * sizeof(float);
  s->group_floats = (size_t)p->bands * pixels * sizeof(float);
  s->group_pairs = s->group_floats * 2 * (size_t)p->repeats;
  s->tab = fdoct::ssada_tab_bytes(n, p->bands);
  s->groups = a->groups;
  const size_t share = s->group_pairs + 2 * s->group_floats;
  const size_t cap = p->max_workspace_bytes ? p->max_workspace_bytes : fdoct::kSsaDefaultWorkspace;
  if (cap < share) return fail(h, FDOCT_ERR_INVALID, f + ": max_workspace_bytes does not hold one group's bands");
  const size_t fit = cap / share;
  s->groups_per_pass = fit < (size_t)a->groups ? (int)fit : a->groups;
  s->passes = (a->groups + s->groups_per_pass - 1) / s->groups_per_pass;
  s->workspace = (size_t)s->groups_per_pass * share;
  return FDOCT_OK;
}

// The outputs' presence, alignment and overlaps among themselves and with the input (in: its first byte and size; null where the
// memory spaces differ).
int check_outputs(fdoct_ctx* h, const char* fn, const SsaPlan& s, const void* in, size_t in_bytes, const float* out_decorr, const float* out_band_decorr,
                  const float* out_power, const float* out_bands) {
  const std::string f(fn);
  if (!out_decorr && !out_band_decorr && !out_power && !out_bands) return fail(h, FDOCT_ERR_INVALID, f + ": no output");
  const void* const p[4] = {out_decorr, out_band_decorr, out_power, out_bands};
  const size_t nb[4] = {s.floats, s.band_floats, s.floats, s.bands};
  for (int i = 0; i < 3; i++)
    if (reinterpret_cast<uintptr_t>(p[i]) % sizeof(float)) return fail(h, FDOCT_ERR_INVALID, f + ": every float output must be aligned to 4 bytes");
  if (reinterpret_cast<uintptr_t>(out_bands) % sizeof(float2)) return fail(h, FDOCT_ERR_INVALID, f + ": out_bands must be aligned to one (re, im) pair (8 bytes)");
  return refuse_overlaps(h, f, "input", in, in_bytes, p, nb, 4);
}

// What both entry points end with.  sp's item 0 is the input (the pairs, or with `front` the frames of its chain, whose pairs are
// ws_cx's): the float outputs join the plan (a null one is a null pointer), then every reservation, the copies up, the chain, the
// table, and pass by pass the split, the window stage, the mean and -- for an out_bands in host memory -- its copy down; then the
// staged copies down.
int run_stage(fdoct_ctx* h, StagePlan* sp, ComplexFront* front, fdoct::SsadaArgs a, const SsaPlan& s, int wa, int wd, float* out_decorr, float* out_band_decorr,
              float* out_power, float* out_bands, fdoct_memspace out_space) {
  DEVICE_SCOPE(h);
  const bool bands_on_device = out_bands && out_space == FDOCT_MEM_DEVICE;
  const bool need_d = out_decorr || out_band_decorr;
  const bool need_p = out_power || (out_decorr && a.min_power > 0.f);
  const int gpp = bands_on_device ? s.groups : s.groups_per_pass;
  const size_t ws_pairs = bands_on_device ? 0 : (size_t)gpp * s.group_pairs;
  const size_t ws_floats = (size_t)gpp * s.group_floats;
  const int dec = sp->out(out_decorr, out_space, s.floats), bdec = sp->out(out_band_decorr, out_space, s.band_floats);
  const int pw = sp->out(out_power, out_space, s.floats);
  if (out_bands && out_space == FDOCT_MEM_HOST) sp->sync = true;   // copied down below, from the workspace
  if (int rc = front ? reserve_complex_front(h, front) : stage_reserve(h, sp)) return rc;
  if (int rc = h->ws_ssa_tab.reserve(h, s.tab)) return rc;
  if (int rc = h->ws_ssa.reserve(h, ws_pairs + 2 * ws_floats)) return rc;

  const float2* const x = front ? static_cast<const float2*>(h->ws_cx) : sp->dev<const float2>(0);
  unsigned char* const ws = h->ws_ssa;
  float2* const ws_bands = reinterpret_cast<float2*>(ws);
  float* const ws_d = reinterpret_cast<float*>(ws + ws_pairs);
  float* const ws_p = reinterpret_cast<float*>(ws + ws_pairs + ws_floats);
  float* const d_dec = sp->dev<float>(dec);
  float* const d_bdec = sp->dev<float>(bdec);
  float* const d_pw = sp->dev<float>(pw);
  a.tw = reinterpret_cast<float2*>(static_cast<unsigned char*>(h->ws_ssa_tab));
  a.gauss = reinterpret_cast<float*>(a.tw + a.fft.n);

  if (int rc = front ? run_complex_front(h, *front) : stage_upload(h, *sp)) return rc;
  HIP_TRY(h, fdoct::launch_ssada_table(a, h->stream));

  const size_t frame_pairs = (size_t)a.ascans * (size_t)a.fft.n;
  const size_t pixels = (size_t)a.ascans * (size_t)a.depth_count;
  for (int g0 = 0; g0 < s.groups; g0 += gpp) {
    fdoct::SsadaArgs pa = a;
    pa.groups = std::min(gpp, s.groups - g0);
    fdoct::ssada_plan_launch(&pa, h->num_cu);
    const size_t band_images = (size_t)g0 * (size_t)a.nbands;   // in front of this pass
    pa.x = x + (size_t)g0 * (size_t)a.repeats * frame_pairs;
    pa.bands = bands_on_device ? reinterpret_cast<float2*>(out_bands) + band_images * (size_t)a.repeats * pixels : ws_bands;
    HIP_TRY(h, fdoct::launch_ssada_split(pa, h->stream));
    if (need_d || need_p) {
      fdoct::AngioArgs w;
      w.x = pa.bands;
      w.groups = pa.groups * a.nbands, w.repeats = a.repeats, w.ascans = a.ascans, w.depths = a.depth_count;
      w.wa = wa, w.wd = wd;
      w.out_decorr = !need_d ? nullptr : d_bdec ? d_bdec + band_images * pixels : ws_d;
      w.out_power = need_p ? ws_p : nullptr;
      fdoct::angio_plan_launch(&w, h->num_cu);
      HIP_TRY(h, fdoct::launch_angio(w, h->stream));
      if (out_decorr || out_power) {
        pa.band_decorr = out_decorr ? w.out_decorr : nullptr, pa.band_power = w.out_power;
        pa.out_decorr = d_dec ? d_dec + (size_t)g0 * pixels : nullptr, pa.out_power = d_pw ? d_pw + (size_t)g0 * pixels : nullptr;
        HIP_TRY(h, fdoct::launch_ssada_mean(pa, h->stream));
      }
    }
    if (out_bands && !bands_on_device)
      HIP_TRY(h, hipMemcpyAsync(reinterpret_cast<float2*>(out_bands) + band_images * (size_t)a.repeats * pixels, ws_bands, (size_t)pa.groups * s.group_pairs,
                                hipMemcpyDeviceToHost, h->stream));
  }
  return stage_finish(h, *sp);
}

}  // namespace

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_ssada_band_table(const fdoct_ssada_params* params, int n, float* table) try {
  if (!params || !table || n < 1) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_ssada_band_table: bad arguments");
  if (params->bands < 1 || params->bands > fdoct::kSsaMaxBands) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_ssada_band_table: bands must be 1..16");
  if (!std::isfinite(params->sigma) || !(params->sigma > 0.0)) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_ssada_band_table: sigma must be finite and greater than 0");
  int k_count = 0;
  if (!support_range(params->k_first, params->k_count, n, &k_count)) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_ssada_band_table: the bands' support must lie in [0, n)");
  const double spacing = (double)k_count / (double)params->bands;
  for (int m = 0; m < params->bands; m++) {
    const double centre = (double)params->k_first + ((double)m + 0.5) * spacing - 0.5;
    for (int q = 0; q < n; q++) {
      float g = 0.f;
      if (q >= params->k_first && q < params->k_first + k_count) {
        const double u = ((double)q - centre) / params->sigma;
        g = (float)std::exp(-0.5 * (u * u));
      }
      table[(size_t)m * (size_t)n + (size_t)q] = g;
    }
  }
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_ssada_plan(const fdoct_ssada_params* params, int nframes, int ascans, int n, fdoct_ssada_info* info) try {
  if (!info) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_ssada_plan: no output");
  fdoct::SsadaArgs a;
  SsaPlan s;
  if (int rc = plan_ssada(nullptr, "fdoct_ssada_plan", params, nframes, ascans, n, &a, &s)) return rc;
  a.groups = s.groups_per_pass;   // the first pass
  fdoct::ssada_plan_launch(&a, 0);
  info->groups = s.groups, info->depth_count = a.depth_count, info->groups_per_pass = s.groups_per_pass, info->passes = s.passes;
  info->lds_bytes = a.lds_bytes, info->workgroups = a.blocks, info->workspace_bytes = s.workspace;
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_ssada(fdoct_handle h, const float* re_im, fdoct_memspace space, int nframes, int ascans, int n, const fdoct_ssada_params* params,
                float* out_decorr, float* out_band_decorr, float* out_power, float* out_bands, fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!re_im || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_ssada: bad arguments");
  if (reinterpret_cast<uintptr_t>(re_im) % sizeof(float2)) return fail(h, FDOCT_ERR_INVALID, "fdoct_ssada: re_im must be aligned to one (re, im) pair (8 bytes)");
  fdoct::SsadaArgs a;
  SsaPlan s;
  if (int rc = plan_ssada(h, "fdoct_ssada", params, nframes, ascans, n, &a, &s)) return rc;
  if (int rc = check_outputs(h, "fdoct_ssada", s, space == out_space ? re_im : nullptr, s.in, out_decorr, out_band_decorr, out_power, out_bands)) return rc;
  StagePlan sp;
  sp.in(re_im, space, s.in);
  return run_stage(h, &sp, nullptr, a, s, params->win_ascans, params->win_depths, out_decorr, out_band_decorr, out_power, out_bands, out_space);
} FDOCT_CATCH(h)

int fdoct_process_ssada(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                        const fdoct_ssada_params* params, float* out_decorr, float* out_band_decorr, float* out_power, float* out_bands,
                        fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!frames || nframes < 1 || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_process_ssada: bad arguments");
  if (h->D != h->N)
    return fail(h, FDOCT_ERR_UNSUPPORTED, "fdoct_process_ssada: numdisplaypoints must equal numfftpoints (the bands are split from the full-length A-scan)");
  fdoct::SsadaArgs a;
  SsaPlan s;
  if (int rc = plan_ssada(h, "fdoct_process_ssada", params, nframes, h->H, h->N, &a, &s)) return rc;
  ComplexFront front;
  if (int rc = plan_complex_front(h, "fdoct_process_ssada", frames, dtype, space, nframes, pitch_bytes, &front)) return rc;
  if (int rc = check_outputs(h, "fdoct_process_ssada", s, space == out_space ? frames : nullptr, front.in_span, out_decorr, out_band_decorr, out_power, out_bands))
    return rc;
  return run_stage(h, &front.p.stage, &front, a, s, params->win_ascans, params->win_depths, out_decorr, out_band_decorr, out_power, out_bands, out_space);
} FDOCT_CATCH(h)

}  // extern "C"
