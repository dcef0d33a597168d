// fdoct_enface.cpp -- the extern "C" entry points of include/fdoct_enface.h (libfdoct_enface.so): the en-face projection of a
// volume over depth slabs.  The kernels are fdoct_enface.hip's; the chain in front of fdoct_process_enface is the core library's
// (fdoct_route.cpp: enqueue, row-major, into ws_enf_vol), behind its own refusals (check_call, choose_route) made here before
// anything is enqueued.  What is this file's own is the calls' arguments: the parameters' refusals and the geometry (plan_enface;
// fdoct_enface_plan reports it), and volumes, frames and all four outputs in host or device memory through the staging plan.
#include "../../include/fdoct_enface.h"

#include <cmath>
#include <cstddef>

#include "fdoct_capture_plan.h"
#include "fdoct_enface_kernels.h"

using namespace fdoct_impl;

static_assert(FDOCT_ENFACE_MAX_SLABS == fdoct::kEnfMaxSlabs && FDOCT_ENFACE_MAX_SMOOTH == fdoct::kEnfMaxSmooth &&
              FDOCT_ENFACE_MAX_MEDIAN == fdoct::kEnfMaxMedian, "the kernels' registers and lanes are sized by them");

namespace {

// The buffers' sizes, in bytes.
struct EnfBytes {
  size_t vol = 0, slabs = 0, surf = 0;   // the volume; one [nslabs][positions][ascans] image stack; one [positions][ascans] image
  int read_first = 0, read_count = 0;    // surface = 0: from the slabs' first depth to their last
};

// What every entry point decides from the parameters and the volume's shape: the refusals, then the kernels' arguments without
// their pointers, and the buffers' sizes.  h may be null (fdoct_enface_plan).
int plan_enface(fdoct_ctx* h, const char* fn, const fdoct_enface_params* p, int positions, int ascans, int depths, fdoct::EnfaceArgs* a, EnfBytes* b) {
  const std::string f(fn);
  if (!p) return fail(h, FDOCT_ERR_INVALID, f + ": no parameters");
  if (positions < 1 || positions > fdoct::kEnfMaxPositions) return fail(h, FDOCT_ERR_INVALID, f + ": positions must be 1..65536");
  if (ascans < 1 || depths < 1 || (long long)ascans * depths > fdoct::kEnfMaxPixels)
    return fail(h, FDOCT_ERR_INVALID, f + ": ascans and depths must be at least 1 and their product at most 2^24");
  if (p->surface < FDOCT_ENFACE_SURFACE_NONE || p->surface > FDOCT_ENFACE_SURFACE_RELATIVE) return fail(h, FDOCT_ERR_INVALID, f + ": surface must be 0, 1 or 2");
  if (p->smooth < 1 || p->smooth > fdoct::kEnfMaxSmooth) return fail(h, FDOCT_ERR_INVALID, f + ": smooth must be 1..16");
  if (p->median < 1 || p->median > fdoct::kEnfMaxMedian || !(p->median & 1)) return fail(h, FDOCT_ERR_INVALID, f + ": median must be odd, 1..15");
  if (p->nslabs < 1 || p->nslabs > fdoct::kEnfMaxSlabs) return fail(h, FDOCT_ERR_INVALID, f + ": nslabs must be 1..8");
  int search = 0;
  if (p->surface) {
    if (!depth_range(p->search_first, p->search_count, depths, &search) || search < p->smooth)
      return fail(h, FDOCT_ERR_INVALID, f + ": the search range must lie in [0, depths) and hold smooth depths");
    if (!std::isfinite(p->threshold)) return fail(h, FDOCT_ERR_INVALID, f + ": threshold must be finite");
    if (p->surface == FDOCT_ENFACE_SURFACE_RELATIVE && !(p->threshold > 0.0 && p->threshold <= 1.0))
      return fail(h, FDOCT_ERR_INVALID, f + ": a relative threshold must lie in (0, 1]");
  }
  int u0 = depths, u1 = 0;
  for (int s = 0; s < p->nslabs; s++) {
    if (p->slab_count[s] < 1) return fail(h, FDOCT_ERR_INVALID, f + ": every slab_count must be at least 1");
    if (p->surface ? (p->slab_first[s] <= -depths || p->slab_first[s] >= depths) : (p->slab_first[s] < 0 || p->slab_first[s] >= depths))
      return fail(h, FDOCT_ERR_INVALID, f + ": slab_first must lie in [0, depths), or with a surface in (-depths, depths)");
    a->first[s] = p->slab_first[s];
    a->count[s] = (int)std::min<long long>(p->slab_count[s], 2LL * depths);   // the rest is clipped whatever the surface
    if (!p->surface) u0 = std::min(u0, a->first[s]), u1 = std::max(u1, std::min(a->first[s] + a->count[s], depths));
  }
  a->positions = positions, a->ascans = ascans, a->depths = depths;
  a->surface = p->surface, a->smooth = p->smooth, a->median = p->median, a->nslabs = p->nslabs;
  a->s0 = p->surface ? p->search_first : 0, a->s1 = a->s0 + search;
  a->threshold = (float)p->threshold;
  fdoct::enface_plan_launch(a, h ? h->num_cu : 0);
  const size_t rows = (size_t)positions * (size_t)ascans;   // <= 2^40
  if (__builtin_mul_overflow(rows * sizeof(float), (size_t)depths, &b->vol) || __builtin_mul_overflow(rows * sizeof(float), (size_t)p->nslabs, &b->slabs))
    return fail(h, FDOCT_ERR_INVALID, f + ": the volume's size does not fit size_t");
  b->surf = rows * sizeof(int32_t);
  b->read_first = p->surface ? 0 : u0, b->read_count = p->surface ? 0 : u1 - u0;
  return FDOCT_OK;
}

// The outputs' presence, alignment and overlaps among themselves and with the inputs (each its first byte and size; null where the
// memory spaces differ or there is none).
int check_outputs(fdoct_ctx* h, const char* fn, const fdoct::EnfaceArgs& a, const EnfBytes& b, const void* in, size_t in_bytes, const void* in2,
                  size_t in2_bytes, const float* out_mean, const float* out_max, const int32_t* out_argmax, const int32_t* out_surface) {
  const std::string f(fn);
  if (!out_mean && !out_max && !out_argmax && !out_surface) return fail(h, FDOCT_ERR_INVALID, f + ": no output");
  if (out_surface && !a.surface) return fail(h, FDOCT_ERR_INVALID, f + ": out_surface needs a surface");
  const void* const p[4] = {out_mean, out_max, out_argmax, out_surface};
  const size_t nb[4] = {b.slabs, b.slabs, b.slabs, b.surf};
  for (int i = 0; i < 4; i++)
    if (reinterpret_cast<uintptr_t>(p[i]) % sizeof(float)) return fail(h, FDOCT_ERR_INVALID, f + ": every output must be aligned to 4 bytes");
  if (int rc = refuse_overlaps(h, f, "input", in, in_bytes, p, nb, 4)) return rc;
  return refuse_overlaps(h, f, "structure", in2, in2_bytes, p, nb, 4);
}

// The chain in front of fdoct_process_enface: the frames (item 0 of its staging plan) and which of the chain's images is the volume.
struct ChainFront {
  FramePlan p;
  int source = FDOCT_ENFACE_SOURCE_DB;
};

// What both entry points end with.  sp's item 0 is the input (the volume, or with `front` the frames of its chain, whose volume is
// ws_enf_vol's) and without `front` item 1 the structure volume: the outputs join the plan (a null one is a null pointer the kernels
// skip), then every reservation and the chain's refusals, the copies up, the chain, the kernels, the copies down.
int run_stage(fdoct_ctx* h, StagePlan* sp, const ChainFront* front, fdoct::EnfaceArgs a, const EnfBytes& b, bool has_structure, float* out_mean,
              float* out_max, int32_t* out_argmax, int32_t* out_surface, fdoct_memspace out_space) {
  DEVICE_SCOPE(h);
  const int mean = sp->out(out_mean, out_space, b.slabs), mx = sp->out(out_max, out_space, b.slabs);
  const int am = sp->out(out_argmax, out_space, b.slabs), sf = sp->out(out_surface, out_space, b.surf);
  if (int rc = stage_reserve(h, sp)) return rc;
  if (a.surface) {
    if (int rc = h->ws_enf_surf.reserve(h, b.surf)) return rc;
  }
  float *k_mag = nullptr, *k_db = nullptr;
  if (front) {
    if (int rc = h->ws_enf_vol.reserve(h, b.vol)) return rc;
    (front->source == FDOCT_ENFACE_SOURCE_LINEAR ? k_mag : k_db) = h->ws_enf_vol;
    // the chain's refusals, as enqueue will make them, while nothing is enqueued yet: the route may compile and rebuild tables
    if (int rc = check_call(h, front->p.dtype, sp->pitch(0), k_mag, k_db)) return rc;
    Route r;
    RouteInputs in = route_inputs(h, front->p.dtype, reinterpret_cast<uintptr_t>(sp->dev<const void>(0)), sp->pitch(0), front->p.nframes);
    in.out_bscan_addr = reinterpret_cast<uintptr_t>(k_mag), in.out_db_addr = reinterpret_cast<uintptr_t>(k_db);
    in.layout = FDOCT_LAYOUT_ROWMAJOR_HxD;
    if (int rc = choose_route(h, in, &r)) return rc;
  }
  a.vol = front ? static_cast<const float*>(h->ws_enf_vol) : sp->dev<const float>(0);
  a.structure = !front && has_structure ? sp->dev<const float>(1) : a.vol;
  a.z0 = a.surface ? static_cast<int32_t*>(h->ws_enf_surf) : nullptr;
  a.out_mean = sp->dev<float>(mean), a.out_max = sp->dev<float>(mx), a.out_argmax = sp->dev<int32_t>(am), a.out_surface = sp->dev<int32_t>(sf);
  if (int rc = stage_upload(h, *sp)) return rc;
  if (front) {
    h->record_now = h->async_timing;
    if (int rc = enqueue(h, sp->dev<const void>(0), front->p.dtype, front->p.nframes, sp->pitch(0), k_mag, k_db, FDOCT_LAYOUT_ROWMAJOR_HxD)) return rc;
  }
  HIP_TRY(h, fdoct::launch_enface(a, h->stream));
  return stage_finish(h, *sp);
}

}  // namespace

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_enface_plan(const fdoct_enface_params* params, int positions, int ascans, int depths, fdoct_enface_info* info) try {
  if (!info) return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_enface_plan: no output");
  fdoct::EnfaceArgs a;
  EnfBytes b;
  if (int rc = plan_enface(nullptr, "fdoct_enface_plan", params, positions, ascans, depths, &a, &b)) return rc;
  info->ascans = a.rows, info->workgroups = a.blocks;
  info->workspace_bytes = a.surface ? b.surf : 0;
  info->read_first = b.read_first, info->read_count = b.read_count;
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_enface(fdoct_handle h, const float* vol, const float* structure, fdoct_memspace space, int positions, int ascans, int depths,
                 const fdoct_enface_params* params, float* out_mean, float* out_max, int32_t* out_argmax, int32_t* out_surface,
                 fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!vol || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_enface: bad arguments");
  if (reinterpret_cast<uintptr_t>(vol) % sizeof(float) || reinterpret_cast<uintptr_t>(structure) % sizeof(float))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_enface: vol and structure must be aligned to 4 bytes");
  fdoct::EnfaceArgs a;
  EnfBytes b;
  if (int rc = plan_enface(h, "fdoct_enface", params, positions, ascans, depths, &a, &b)) return rc;
  if (structure && !a.surface) return fail(h, FDOCT_ERR_INVALID, "fdoct_enface: a structure volume needs a surface");
  const bool same = space == out_space;
  if (int rc = check_outputs(h, "fdoct_enface", a, b, same ? vol : nullptr, b.vol, same ? structure : nullptr, b.vol, out_mean, out_max, out_argmax, out_surface))
    return rc;
  StagePlan sp;
  sp.in(vol, space, b.vol);
  if (structure) sp.in(structure, space, b.vol);
  return run_stage(h, &sp, nullptr, a, b, structure != nullptr, out_mean, out_max, out_argmax, out_surface, out_space);
} FDOCT_CATCH(h)

int fdoct_process_enface(fdoct_handle h, const void* frames, fdoct_dtype dtype, fdoct_memspace space, int nframes, size_t pitch_bytes,
                         int source, const fdoct_enface_params* params, float* out_mean, float* out_max, int32_t* out_argmax,
                         int32_t* out_surface, fdoct_memspace out_space) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!frames || nframes < 1 || !valid_mem(space) || !valid_mem(out_space)) return fail(h, FDOCT_ERR_INVALID, "fdoct_process_enface: bad arguments");
  if (source != FDOCT_ENFACE_SOURCE_LINEAR && source != FDOCT_ENFACE_SOURCE_DB) return fail(h, FDOCT_ERR_INVALID, "fdoct_process_enface: source must be 0 or 1");
  if (h->sim_group != 1) return fail(h, FDOCT_ERR_UNSUPPORTED, "fdoct_process_enface: the sim variant's averages are not supported");
  if (nframes % h->A) return fail(h, FDOCT_ERR_INVALID, "fdoct_process_enface: nframes must be a multiple of averages");
  fdoct::EnfaceArgs a;
  EnfBytes b;
  if (int rc = plan_enface(h, "fdoct_process_enface", params, nframes / h->A, h->H, h->D, &a, &b)) return rc;
  ChainFront front;
  front.source = source;
  if (int rc = plan_frames(h, "fdoct_process_enface", frames, dtype, space, nframes, pitch_bytes, &front.p)) return rc;
  size_t in_span = 0;
  if (__builtin_mul_overflow(front.p.pitch, (size_t)front.p.raw_h * (size_t)nframes, &in_span))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_process_enface: the batch is too large");
  if (int rc = check_outputs(h, "fdoct_process_enface", a, b, space == out_space ? frames : nullptr, in_span, nullptr, 0, out_mean, out_max, out_argmax, out_surface))
    return rc;
  return run_stage(h, &front.p.stage, &front, a, b, false, out_mean, out_max, out_argmax, out_surface, out_space);
} FDOCT_CATCH(h)

}  // extern "C"
