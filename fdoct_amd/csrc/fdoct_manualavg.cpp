// fdoct_manualavg.cpp -- the extern "C" entry points of include/fdoct_manualavg.h: manual averaging of B-scans
// (BscanFFT.cpp:1399-1444) over the kernel of fdoct_manualavg.hip.  The accumulator (manualaccum) and the counter
// (manualaccumcount) live in the handle: fdoct_ctx::d_mavg and mavg_*.
#include "../../include/fdoct_manualavg.h"

#include "fdoct_ctx.h"
#include "fdoct_manualavg_kernels.h"

using namespace fdoct_impl;

namespace {

bool valid_mode(int mode) { return mode == FDOCT_MANUALAVG_REFERENCE || mode == FDOCT_MANUALAVG_KEEP_ALL; }

void forget(fdoct_ctx* h) {
  if (h->d_mavg) drain(h);  // the adds still in flight use the accumulator
  h->d_mavg.release();
  h->mavg_count = 0;
  h->mavg_m = h->mavg_mode = h->mavg_accumulated = 0;
}

}  // namespace

// ------------------------------------------------------------------ C ABI --
extern "C" {

int fdoct_manualavg_plan(int manualaverages, int mode, int accumulated, int nbscans, int* emitted, int* accumulated_after) try {
  if (manualaverages < 1 || manualaverages == INT32_MAX || !valid_mode(mode) || accumulated < 0 || accumulated > manualaverages || nbscans < 0)
    return fail(nullptr, FDOCT_ERR_INVALID, "fdoct_manualavg_plan: bad arguments");
  int first = 0, period = 1;
  fdoct::manualavg_schedule(manualaverages, mode == FDOCT_MANUALAVG_REFERENCE, accumulated, &first, &period);
  if (emitted) *emitted = fdoct::manualavg_emissions(first, period, nbscans);
  if (accumulated_after) *accumulated_after = fdoct::manualavg_counter_after(first, period, accumulated, nbscans);
  return FDOCT_OK;
} FDOCT_CATCH(nullptr)

int fdoct_manualavg_begin(fdoct_handle h, int manualaverages, size_t count, int mode) try {
  if (manualaverages < 1 || manualaverages == INT32_MAX || !valid_mode(mode) || count < 1 || count > ((size_t)1 << 40))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_manualavg_begin: bad arguments");
  if (!h) return FDOCT_ERR_INVALID;
  DEVICE_SCOPE(h);
  forget(h);  // (waits for the kernels that still use the old accumulator)
  if (int rc = h->d_mavg.assign(h, count)) return rc;
  const hipError_t e = hipMemsetAsync(h->d_mavg, 0, count * sizeof(double), h->stream);  // main:933
  if (e != hipSuccess) {
    forget(h);
    return fail(h, FDOCT_ERR_DEVICE, std::string("fdoct_manualavg_begin: hipMemsetAsync: ") + hipGetErrorString(e));
  }
  h->mavg_count = count, h->mavg_m = manualaverages, h->mavg_mode = mode, h->mavg_accumulated = 0;  // main:567
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_manualavg_add(fdoct_handle h, const float* bscans, fdoct_memspace mem, int nbscans, float* out_mean, float* out_db,
                        fdoct_memspace out_mem, int out_capacity, int* emitted) try {
  // what needs no handle first: a bad call is refused the same way with and without a device
  if (!bscans || !valid_mem(mem) || !valid_mem(out_mem) || nbscans < 1 || out_capacity < 0)
    return fail(h, FDOCT_ERR_INVALID, "fdoct_manualavg_add: bad arguments");
  if (!h) return FDOCT_ERR_INVALID;
  if (!h->mavg_m || !h->d_mavg) return fail(h, FDOCT_ERR_STATE, "fdoct_manualavg_add: no accumulator (fdoct_manualavg_begin)");
  const size_t count = h->mavg_count;
  if ((size_t)nbscans > ((size_t)1 << 40) / count) return fail(h, FDOCT_ERR_INVALID, "fdoct_manualavg_add: the batch is too large");

  fdoct::ManualAvgArgs a;
  a.count = (long long)count, a.nb = nbscans, a.m = h->mavg_m, a.drop = h->mavg_mode == FDOCT_MANUALAVG_REFERENCE;
  fdoct::manualavg_schedule(a.m, a.drop, h->mavg_accumulated, &a.first, &a.period);
  const int emits = fdoct::manualavg_emissions(a.first, a.period, nbscans);
  const int after = fdoct::manualavg_counter_after(a.first, a.period, h->mavg_accumulated, nbscans);
  if (out_capacity < emits) return fail(h, FDOCT_ERR_INVALID, "fdoct_manualavg_add: out_capacity is below what fdoct_manualavg_plan says for this call");
  if (emits && !out_mean && !out_db) return fail(h, FDOCT_ERR_INVALID, "fdoct_manualavg_add: the call emits and has no output");
  const size_t in_bytes = count * nbscans * sizeof(float);
  const size_t cap_bytes = count * std::min((size_t)out_capacity, ((size_t)1 << 40) / count) * sizeof(float);  // (what the caller says the outputs hold)
  if (overlap(out_mean, cap_bytes, out_db, cap_bytes) ||
      (mem == out_mem && (overlap(bscans, in_bytes, out_mean, cap_bytes) || overlap(bscans, in_bytes, out_db, cap_bytes))))
    return fail(h, FDOCT_ERR_INVALID, "fdoct_manualavg_add: input and output buffers overlap");
  DEVICE_SCOPE(h);

  // only the emitted slots are written, so only they are staged: host slots past them keep what they hold
  const size_t out_bytes = count * emits * sizeof(float);
  StagePlan sp;
  const int in = sp.in(bscans, mem, in_bytes);
  const int mean = sp.out(emits ? out_mean : nullptr, out_mem, out_bytes), db = sp.out(emits ? out_db : nullptr, out_mem, out_bytes);
  if (int rc = stage_reserve(h, &sp)) return rc;
  a.in = sp.dev<const float>(in), a.acc = h->d_mavg, a.out_mean = sp.dev<float>(mean), a.out_db = sp.dev<float>(db);
  fdoct::manualavg_plan_launch(&a, h->num_cu);
  if (int rc = stage_upload(h, sp)) return rc;
  HIP_TRY(h, fdoct::launch_manualavg(a, h->stream));
  h->mavg_accumulated = after;  // the work is enqueued: the counter is the host's
  if (emitted) *emitted = emits;
  return stage_finish(h, sp);
} FDOCT_CATCH(h)

int fdoct_manualavg_state(fdoct_handle h, int* manualaverages, size_t* count, int* mode, int* accumulated, double* partial_host) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!h->mavg_m || !h->d_mavg) return fail(h, FDOCT_ERR_STATE, "fdoct_manualavg_state: no accumulator (fdoct_manualavg_begin)");
  if (partial_host) {
    DEVICE_SCOPE(h);
    HIP_TRY(h, hipMemcpyAsync(partial_host, h->d_mavg, h->mavg_count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  if (manualaverages) *manualaverages = h->mavg_m;
  if (count) *count = h->mavg_count;
  if (mode) *mode = h->mavg_mode;
  if (accumulated) *accumulated = h->mavg_accumulated;
  return FDOCT_OK;
} FDOCT_CATCH(h)

int fdoct_manualavg_end(fdoct_handle h) try {
  if (!h) return FDOCT_ERR_INVALID;
  if (!h->d_mavg) return FDOCT_OK;
  DEVICE_SCOPE(h);
  forget(h);
  return FDOCT_OK;
} FDOCT_CATCH(h)

}  // extern "C"
