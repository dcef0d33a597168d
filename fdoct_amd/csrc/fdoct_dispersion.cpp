// fdoct_dispersion.cpp -- the extern "C" entry points of include/fdoct_dispersion.h (libfdoct_dispersion.so): a numerical
// dispersion search over (a2, a3) on complex A-scans.  The kernels are fdoct_dispersion.hip's; the chain in front of
// fdoct_process_dispersion_search is the core library's (fdoct_route.cpp: enqueue_complex), called in the order
// fdoct_capture_plan.h's ComplexFront keeps; the transform's radices are the planner's (fdoct_plan.cpp: make_plan on a complex row
// of n points).  What is this file's own is the calls' arguments: the grid's refusals, the call's geometry as a value (plan_search;
// fdoct_dispersion_plan reports it), and pairs, frames and all four outputs in host or device memory through the staging plan.
#include "../../include/fdoct_dispersion.h"

#include <cmath>
#include <cstddef>

#include "fdoct_capture_plan.h"
#include "fdoct_dispersion_kernels.h"

using namespace fdoct_impl;

static_assert(sizeof(fdoct::DispBest) == sizeof(fdoct_dispersion_best) && offsetof(fdoct::DispBest, i3) == offsetof(fdoct_dispersion_best, i3) &&
                  offsetof(fdoct::DispBest, a2) == offsetof(fdoct_dispersion_best, a2) && offsetof(fdoct::DispBest, metric) == offsetof(fdoct_dispersion_best, metric),
              "the kernel writes fdoct_dispersion_best");

namespace {

// The Stockham radices of a complex row of n points, as the workgroup-per-row kernel would take it: empty where the planner has
// none (a prime factor above 5).
std::vector<int> radices_of(int n) {
  fdoct::PlanInputs in;
  in.W = n, in.M = 1, in.N = n, in.D = n, in.phase = true, in.plan_override = -2;
  fdoct::Plan p;
  std::string why;
  if (fdoct::make_plan(in, &p, &why) != FDOCT_OK || p.gen.blu_m || (int)p.gen.rad_n.size() > fdoct::kDispMaxPasses) return {};
  return p.gen.rad_n;
}

// What every entry point decides from the grid and the rows' shape: the refusals, then the kernels' arguments without their
// pointers.  h may be null (fdoct_dispersion_plan).
int plan_search(fdoct_ctx* h, const char* fn, const fdoct_dispersion_grid* g, long long rows, int n, fdoct::DispersionArgs* a) {
  const std::string f(fn);
  if (!g) return fail(h, FDOCT_ERR_INVALID, f + ": no grid");
  if (rows < 1 || n < fdoct::kDispMinN) return fail(h, FDOCT_ERR_INVALID, f + ": rows must be at least 1 and n at least 16");
  if (n > fdoct::kDispMaxN) return fail(h, FDOCT_ERR_UNSUPPORTED, f + ": rows of more than 4096 points");
  if (g->a2_count < 1 || g->a3_count < 1 || (long long)g->a2_count * g->a3_count > fdoct::kDispMaxK)
    return fail(h, FDOCT_ERR_INVALID, f + ": a2_count and a3_count must be at least 1 and their product at most 65536");
  const int K = g->a2_count * g->a3_count;
  if (rows > fdoct::kDispMaxRowsK / K) return fail(h, FDOCT_ERR_INVALID, f + ": rows times candidates must not exceed 2^24");
  if (!std::isfinite(g->a2_first) || !std::isfinite(g->a2_step) || !std::isfinite(g->a3_first) || !std::isfinite(g->a3_step))
    return fail(h, FDOCT_ERR_INVALID, f + ": the grid's firsts and steps must be finite");
  if (g->depth_first < 0 || g->depth_first >= n || g->depth_count < 0 || g->depth_count > n - g->depth_first)
    return fail(h, FDOCT_ERR_INVALID, f + ": the depth range must lie in [0, n)");
  const int count = g->depth_count ? g->depth_count : n / 2 - g->depth_first;
  if (count < 1) return fail(h, FDOCT_ERR_INVALID, f + ": the depth range holds no bin");
  const std::vector<int> rad = radices_of(n);
  if (rad.empty()) return fail(h, FDOCT_ERR_UNSUPPORTED, f + ": n has a prime factor above 5");
  a->rows = (int)rows, a->n = n, a->K = K, a->a2_count = g->a2_count, a->a3_count = g->a3_count;
  a->a2_first = g->a2_first, a->a2_step = g->a2_step, a->a3_first = g->a3_first, a->a3_step = g->a3_step;
  a->depth_first = g->depth_first, a->depth_count = count;
  a->npass = (int)rad.size();
  unsigned Ns = 1;
  for (int p = 0; p < a->npass; p++) {
    a->rad[p] = rad[p];
    a->magic[p] = Ns > 1 ? (unsigned)(((1ull << 32) + Ns - 1) / Ns) : 0u;
    Ns *= (unsigned)rad[p];
  }
  fdoct::dispersion_plan_launch(a);
  return FDOCT_OK;
}

struct OutBytes {
  size_t sums = 0, row_sums = 0, table = 0, tab = 0;
};

OutBytes out_bytes(const fdoct::DispersionArgs& a) {
  OutBytes b;
  b.sums = (size_t)a.K * sizeof(double2);
  b.row_sums = (size_t)a.rows * b.sums;   // rows K <= 2^24
  b.table = (size_t)a.n * sizeof(float2);
  b.tab = fdoct::dispersion_tab_entries(a.n, a.a2_count, a.a3_count) * sizeof(float2);
  return b;
}

// The outputs' presence, alignment and overlaps among themselves and with the input (in: its first byte and size; null where the
// memory spaces differ).
int check_outputs(fdoct_ctx* h, const char* fn, const OutBytes& b, const void* in, size_t in_bytes, const double* out_sums, const double* out_row_sums,
                  const fdoct_dispersion_best* out_best, const float* out_cos_sin) {
  const std::string f(fn);
  if (!out_sums && !out_row_sums && !out_best && !out_cos_sin) return fail(h, FDOCT_ERR_INVALID, f + ": no output");
  const void* const p[4] = {out_sums, out_row_sums, out_best, out_cos_sin};
  const size_t nb[4] = {b.sums, b.row_sums, sizeof(fdoct_dispersion_best), b.table};
  for (int i = 0; i < 4; i++)
    if (reinterpret_cast<uintptr_t>(p[i]) % 8) return fail(h, FDOCT_ERR_INVALID, f + ": every output must be aligned to 8 bytes");
  return refuse_overlaps(h, f, "input", in, in_bytes, p, nb, 4);
}

// What both entry points end with.  sp's item 0 is the input (the pairs, or with `front` the frames of its chain, whose pairs are
// ws_cx's): the outputs join the plan -- a null array or winner is scratch the kernels write anyway, a null table a null pointer
// they skip -- then every reservation, the copies up, the chain, the kernels, the copies down.
int run_search(fdoct_ctx* h, StagePlan* sp, ComplexFront* front, fdoct::DispersionArgs a, const OutBytes& b, double* out_sums, double* out_row_sums,
               fdoct_dispersion_best* out_best, float* out_cos_sin, fdoct_memspace out_space) {
  DEVICE_SCOPE(h);
  const int sums = sp->out_or_scratch(out_sums, out_space, b.sums), row_sums = sp->out_or_scratch(out_row_sums, out_space, b.row_sums);
  const int best = sp->out_or_scratch(out_best, out_space, sizeof(fdoct::DispBest)), table = sp->out(out_cos_sin, out_space, b.table);
  if (int rc = front ? reserve_complex_front(h, front) : stage_reserve(h, sp)) return rc;
  if (int rc = h->ws_disp_tab.reserve(h, b.tab)) return rc;
  a.x = front ? static_cast<const float2*>(h->ws_cx) : sp->dev<const float2>(0);
  a.tab = h->ws_disp_tab;
  a.sums = sp->dev<double2>(sums), a.row_sums = sp->dev<double2>(row_sums), a.best = sp->dev<fdoct::DispBest>(best), a.cos_sin = sp->dev<float2>(table);
  if (int rc = front ? run_complex_front(h, *front) : stage_upload(h, *sp)) return rc;
  HIP_TRY(h, fdoct::launch_dispersion(a, h->stream));
  return stage_finish(h, *sp);
}

}  // namespace

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_dispersion_phase_table(int n, double a2, double a3, float* cos_sin_pairs) try {
  if (n < 1 || !cos_sin_pairs || !std::isfinite(a2) || !std::isfinite(a3)) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_dispersion_phase_table: bad arguments");
  for (int q = 0; q < n; q++) {
    const double x = ((double)q - 0.5 * (double)n) / (0.5 * (double)n);
    const double phi = a2 * (x * x) + a3 * (x * x * x);
    cos_sin_pairs[2 * q] = (float)std::cos(phi), cos_sin_pairs[2 * q + 1] = (float)std::sin(phi);
  }
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_dispersion_plan(const fdoct_dispersion_grid* grid, int rows, int n, fdoct_dispersion_info* info) try {
  if (!info) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_dispersion_plan: no output");
  fdoct::DispersionArgs a;
  if (int rc = plan_search(nullptr, "fdoct_dispersion_plan", grid, rows, n, &a)) return rc;
  const OutBytes b = out_bytes(a);
  info->candidates = a.K, info->per_workgroup = a.per_wg, info->chunks = a.chunks, info->lds_bytes = a.lds_bytes;
  info->workgroups = a.workgroups;
  info->workspace_bytes = b.tab + b.row_sums + b.sums + b.table + sizeof(fdoct::DispBest);
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_dispersion_search(fdoct_handle h, const float* re_im, fdoct_memspace space, int rows, int n, const fdoct_dispersion_grid* grid,
                            double* out_sums, double* out_row_sums, fdoct_dispersion_best* out_best, float* out_cos_sin,
                            fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!re_im || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_dispersion_search: bad arguments");
  if (reinterpret_cast<uintptr_t>(re_im) % sizeof(float2))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_dispersion_search: re_im must be aligned to one (re, im) pair (8 bytes)");
  fdoct::DispersionArgs a;
  if (int rc = plan_search(h, "fdoct_dispersion_search", grid, rows, n, &a)) return rc;
  const OutBytes b = out_bytes(a);
  const size_t in_bytes = (size_t)rows * (size_t)n * sizeof(float2);
  if (int rc = check_outputs(h, "fdoct_dispersion_search", b, space == out_space ? re_im : nullptr, in_bytes, out_sums, out_row_sums, out_best, out_cos_sin))
    return rc;
  StagePlan sp;
  sp.in(re_im, space, in_bytes);
  return run_search(h, &sp, nullptr, a, b, out_sums, out_row_sums, out_best, out_cos_sin, out_space);
} FDOCT_CATCH(h)

int fdoct_process_dispersion_search(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes,
                                    size_t pitch_bytes, const fdoct_dispersion_grid* grid, double* out_sums, double* out_row_sums,
                                    fdoct_dispersion_best* out_best, float* out_cos_sin, fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!frames || nframes < 1 || !valid_mem(space) || !valid_mem(out_space))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_process_dispersion_search: bad arguments");
  if (h->D != h->N)
    return fail(h, FDOCT_ERR_UNSUPPORTED, "fdoct_process_dispersion_search: numdisplaypoints must equal numfftpoints (a calibration handle shows the full length)");
  fdoct::DispersionArgs a;
  if (int rc = plan_search(h, "fdoct_process_dispersion_search", grid, (long long)nframes * h->H, h->N, &a)) return rc;
  const OutBytes b = out_bytes(a);
  ComplexFront front;
  if (int rc = plan_complex_front(h, "fdoct_process_dispersion_search", frames, dtype, space, nframes, pitch_bytes, &front)) return rc;
  if (int rc = check_outputs(h, "fdoct_process_dispersion_search", b, space == out_space ? frames : nullptr, front.in_span, out_sums, out_row_sums, out_best,
                             out_cos_sin))
    return rc;
  return run_search(h, &front.p.stage, &front, a, b, out_sums, out_row_sums, out_best, out_cos_sin, out_space);
} FDOCT_CATCH(h)

}  // extern "C"
