// Out of host memory inside an entry point of include/fdoct.h is an error code, never an exception across the C ABI: the
// global operator new is replaced so that, once armed with k, the k-th allocation fails.  For k = 1, 2, ... until a call runs
// through without the failure firing, every call of the host-only table builders must return FDOCT_ERR_NOMEM (and this
// process stay alive); disarmed, the result must equal an unarmed call's bit for bit.  Built with g++ against
// libfdoct_hip.so by tests/test_abi.py.  Opens no device.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "fdoct.h"

static long g_armed = 0;  // > 0: the allocation that brings g_count to this number fails
static long g_count = 0;
static bool g_fired = false;

static bool fail_now() {
  if (g_armed <= 0 || ++g_count != g_armed) return false;
  g_fired = true;
  return true;
}
static void* get(std::size_t n, std::size_t align) {
  void* p = nullptr;
  if (align <= alignof(std::max_align_t)) p = std::malloc(n ? n : 1);
  else if (posix_memalign(&p, align, n ? n : 1) != 0) p = nullptr;
  return p;
}
static void* get_or_throw(std::size_t n, std::size_t align) {
  void* p = fail_now() ? nullptr : get(n, align);
  if (!p) throw std::bad_alloc();
  return p;
}
static void* get_or_null(std::size_t n, std::size_t align) noexcept { return fail_now() ? nullptr : get(n, align); }

// every replaceable form (C++17): plain, array, aligned, nothrow, and the sized / aligned deletes
void* operator new(std::size_t n) { return get_or_throw(n, 0); }
void* operator new[](std::size_t n) { return get_or_throw(n, 0); }
void* operator new(std::size_t n, std::align_val_t a) { return get_or_throw(n, static_cast<std::size_t>(a)); }
void* operator new[](std::size_t n, std::align_val_t a) { return get_or_throw(n, static_cast<std::size_t>(a)); }
void* operator new(std::size_t n, const std::nothrow_t&) noexcept { return get_or_null(n, 0); }
void* operator new[](std::size_t n, const std::nothrow_t&) noexcept { return get_or_null(n, 0); }
void* operator new(std::size_t n, std::align_val_t a, const std::nothrow_t&) noexcept { return get_or_null(n, static_cast<std::size_t>(a)); }
void* operator new[](std::size_t n, std::align_val_t a, const std::nothrow_t&) noexcept { return get_or_null(n, static_cast<std::size_t>(a)); }
void operator delete(void* p) noexcept { std::free(p); }
void operator delete[](void* p) noexcept { std::free(p); }
void operator delete(void* p, std::size_t) noexcept { std::free(p); }
void operator delete[](void* p, std::size_t) noexcept { std::free(p); }
void operator delete(void* p, std::align_val_t) noexcept { std::free(p); }
void operator delete[](void* p, std::align_val_t) noexcept { std::free(p); }
void operator delete(void* p, std::size_t, std::align_val_t) noexcept { std::free(p); }
void operator delete[](void* p, std::size_t, std::align_val_t) noexcept { std::free(p); }
void operator delete(void* p, const std::nothrow_t&) noexcept { std::free(p); }
void operator delete[](void* p, const std::nothrow_t&) noexcept { std::free(p); }
void operator delete(void* p, std::align_val_t, const std::nothrow_t&) noexcept { std::free(p); }
void operator delete[](void* p, std::align_val_t, const std::nothrow_t&) noexcept { std::free(p); }

// call(out) writes `bytes` bytes of results to out and returns the entry point's code
template <typename Call>
static bool sweep(const char* name, size_t bytes, Call call) {
  std::vector<unsigned char> want(bytes, 0), got(bytes, 0);
  if (call(want.data()) != FDOCT_OK) {
    std::printf("%s: the unarmed call failed\n", name);
    return false;
  }
  long failures = 0;
  for (long k = 1;; k++) {
    g_count = 0;
    g_fired = false;
    g_armed = k;
    const int rc = call(got.data());
    g_armed = 0;
    if (!g_fired) {  // the call made fewer than k allocations: it ran through
      if (rc != FDOCT_OK) {
        std::printf("%s: k = %ld, no allocation failed, code %d\n", name, k, rc);
        return false;
      }
      break;
    }
    if (rc != FDOCT_ERR_NOMEM || !std::strstr(fdoct_last_error(nullptr), "out of host memory")) {
      std::printf("%s: allocation %ld failed, code %d (%s) instead of FDOCT_ERR_NOMEM\n", name, k, rc, fdoct_last_error(nullptr));
      return false;
    }
    failures++;
  }
  if (!failures) {
    std::printf("%s: no allocation to fail\n", name);
    return false;
  }
  std::memset(got.data(), 0xa5, bytes);
  if (call(got.data()) != FDOCT_OK || std::memcmp(want.data(), got.data(), bytes) != 0) {
    std::printf("%s: after the sweep the result differs from the unarmed call's\n", name);
    return false;
  }
  std::printf("%s: %ld failed allocations, each FDOCT_ERR_NOMEM\n", name, failures);
  return true;
}

static bool resample_table(int width, int multiplier, int n) {
  char name[64];
  std::snprintf(name, sizeof name, "fdoct_build_resample_table(%d, %d, %d)", width, multiplier, n);
  return sweep(name, (size_t)n * (sizeof(double) + sizeof(int32_t)), [=](unsigned char* out) {
    return fdoct_build_resample_table(width, multiplier, n, 816e-9, 884e-9, reinterpret_cast<int32_t*>(out + (size_t)n * sizeof(double)),
                                      reinterpret_cast<double*>(out));
  });
}

int main() {
  bool ok = resample_table(2048, 1, 2048) && resample_table(640, 4, 2560);
  ok = ok && sweep("fdoct_build_window(2048)", 2048 * sizeof(double),
                   [](unsigned char* out) { return fdoct_build_window(2048, reinterpret_cast<double*>(out)); });
  if (!ok) return 1;
  std::printf("ok\n");
  return 0;
}
