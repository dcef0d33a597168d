// fdoct_stage.h -- the arguments of a side entry point that may lie in host memory, as a value: the call names each input and
// output before anything is enqueued, and the plan places the host-memory ones in one input and one output workspace (committed
// by fdoct_ctx.h's stage_reserve / stage_upload / stage_finish).  Plain C++ without HIP: tests/native/stage_check.cpp pins it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/fdoct.h"

namespace fdoct {

inline bool valid_mem(fdoct_memspace m) { return m == FDOCT_MEM_HOST || m == FDOCT_MEM_DEVICE; }
inline bool valid_layout(fdoct_layout l) { return l == FDOCT_LAYOUT_ROWMAJOR_HxD || l == FDOCT_LAYOUT_TRANSPOSED_DxH; }
inline size_t packed_pitch(size_t row_bytes) { return (row_bytes + 15) & ~(size_t)15; }  // rows of the library's workspaces
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return a && b && x < y + nb && y < x + na;
}
// A stage's depth range [first, first + count) of `depths` bins, count 0 meaning "to the last depth" (the Doppler and angiography
// bulk ranges, vibrometry's reference range): false where it does not lie in [0, depths), else *resolved is the count, > 0.
inline bool depth_range(int first, int count, int depths, int* resolved) {
  if (first < 0 || first >= depths || count < 0 || count > depths - first) return false;
  *resolved = count ? count : depths - first;
  return true;
}
// What a call with n outputs of bytes[i] bytes at out[i] (null: absent) and an input range (in null: none, or one in another memory
// space) refuses: the input lying on an output, or two outputs on each other.
enum Overlap { OVERLAP_NONE = 0, OVERLAP_INPUT, OVERLAP_OUTPUTS };
inline Overlap overlaps(const void* in, size_t in_bytes, const void* const* out, const size_t* bytes, int n) {
  for (int i = 0; i < n; i++) {
    if (overlap(in, in_bytes, out[i], bytes[i])) return OVERLAP_INPUT;
    for (int j = 0; j < i; j++)
      if (overlap(out[i], bytes[i], out[j], bytes[j])) return OVERLAP_OUTPUTS;
  }
  return OVERLAP_NONE;
}

struct StageItem {
  void *ptr = nullptr, *dev = nullptr;  // the caller's pointer (null: scratch if staged, else an output nobody reads); what the kernel takes (stage_reserve)
  bool staged = false, output = false;  // staged: lives at `offset` of a workspace (host memory on its way, or scratch) ...
  bool on_input = false;                // ... of the input workspace, for an output that lies on its staged input
  size_t row = 0, rows = 1, pitch = 0;  // bytes per row, rows, the caller's pitch
  size_t dev_pitch = 0, offset = 0;     // the pitch the kernel sees: the caller's own, or the packed one of staged rows
};

// Every adder returns its item's index.  The flat form is (p, mem, bytes); the 2-D form adds rows and the caller's pitch, and
// staged rows are packed_pitch(row) apart.  Any memory space but host reads as device memory: the caller's pointer and pitch pass
// through.  Arithmetic that would wrap size_t, or one item past kMaxItems, leaves rc set: the call is refused at reserve.
struct StagePlan {
  static constexpr size_t kMaxItems = 8, kAlign = 256;  // frames and up to seven further arguments; every staged item starts at a multiple of kAlign, whatever the others' sizes
  StageItem item[kMaxItems];
  int count = 0, rc = FDOCT_OK;
  size_t in_bytes = 0, out_bytes = 0;  // what the two workspaces must hold
  bool sync = false;  // an item is in host memory: the call returns with the stream drained (a call that copies an argument itself ors in)

  int in(const void* p, fdoct_memspace mem, size_t row, size_t rows = 1, size_t pitch = 0) { return add(const_cast<void*>(p), mem, row, rows, pitch, false, false); }
  int out(void* p, fdoct_memspace mem, size_t row, size_t rows = 1, size_t pitch = 0) { return add(p, mem, row, rows, pitch, true, false); }
  // an optional output the kernel writes anyway: null becomes scratch (with out: a null device pointer)
  int out_or_scratch(void* p, fdoct_memspace mem, size_t bytes) { return add(p, mem, bytes, 1, 0, true, true); }
  // the output of a kernel that may run in place on input i: with host memory on both sides, the input's own device copy
  int out_on(int i, void* p, fdoct_memspace mem, size_t pitch) {
    const size_t before = out_bytes;
    const int o = out(p, mem, item[i].row, item[i].rows, pitch);
    if (!rc && item[i].staged && item[o].staged) out_bytes = before, item[o].on_input = true, item[o].offset = item[i].offset;
    return o;
  }
  template <typename T> T* dev(int i) const { return static_cast<T*>(item[i].dev); }
  size_t pitch(int i) const { return item[i].dev_pitch; }

 private:
  int add(void* p, fdoct_memspace mem, size_t row, size_t rows, size_t pitch, bool output, bool scratch) {
    if (count == (int)kMaxItems) return rc = FDOCT_ERR_INVALID, 0;
    StageItem& it = item[count];
    it.ptr = p, it.output = output, it.row = row, it.rows = rows, it.pitch = it.dev_pitch = pitch ? pitch : row;
    const bool host = p && mem == FDOCT_MEM_HOST;
    sync = sync || host;
    if (host || (!p && scratch)) {
      size_t& total = output ? out_bytes : in_bytes;
      size_t bytes = 0, end = 0;
      it.staged = true, it.offset = total, it.dev_pitch = pitch ? packed_pitch(row) : row;
      const bool wraps = row > SIZE_MAX - 15 || __builtin_mul_overflow(it.dev_pitch, rows, &bytes) || __builtin_add_overflow(total, bytes, &end);
      if (wraps || end > SIZE_MAX - (kAlign - 1)) rc = FDOCT_ERR_INVALID;
      total = (end + kAlign - 1) & ~(kAlign - 1);
    }
    return count++;
  }
};

}  // namespace fdoct
