// stage_check.cpp -- the staging plan of the side entry points (fdoct_amd/csrc/fdoct_stage.h) over the plan type alone: where
// host-memory items land in the two workspaces, what device-memory items keep, scratch, the in-place pair, the packed pitch, the
// synchronise flag, the refusal of sizes that would wrap, the vibrometry and dispersion calls' layouts, and the overlap check and the
// depth range the stages share.  tests/test_abi.py builds it with g++ and expects "ok".
#include <cstdio>
#include <initializer_list>

#include "fdoct_stage.h"

using namespace fdoct;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("line %d: %s\n", __LINE__, #cond);             \
      failures++;                                                \
    }                                                            \
  } while (0)

static size_t item_bytes(const StageItem& it) { return it.dev_pitch * it.rows; }

// Every staged item starts at a multiple of 256, the items of one workspace do not overlap, and the totals cover the last one.
static void check_layout(const StagePlan& p) {
  for (int i = 0; i < p.count; i++) {
    const StageItem& a = p.item[i];
    if (!a.staged) continue;
    const bool a_in = !a.output || a.on_input;
    CHECK(a.offset % 256 == 0);
    CHECK(a.offset + item_bytes(a) <= (a_in ? p.in_bytes : p.out_bytes));
    for (int j = 0; j < i; j++) {
      const StageItem& b = p.item[j];
      if (!b.staged || a_in != (!b.output || b.on_input) || a.on_input || b.on_input) continue;
      CHECK(a.offset >= b.offset + item_bytes(b) || b.offset >= a.offset + item_bytes(a));
    }
  }
  CHECK(p.in_bytes % 256 == 0 && p.out_bytes % 256 == 0);
}

int main() {
  char buf[64] = {0};
  void* const a = buf;
  void* const b = buf + 16;
  void* const c = buf + 32;
  void* const d = buf + 48;

  {  // host memory on both sides, odd sizes: the binning's two inputs and two outputs
    StagePlan p;
    const int i0 = p.in(a, FDOCT_MEM_HOST, 2 * 8 * 32 * 4 + 4), i1 = p.in(b, FDOCT_MEM_HOST, 1001);
    const int o0 = p.out(c, FDOCT_MEM_HOST, 777), o1 = p.out(d, FDOCT_MEM_HOST, 3);
    CHECK(p.rc == FDOCT_OK && p.count == 4 && p.sync);
    CHECK(i0 == 0 && i1 == 1 && o0 == 2 && o1 == 3);
    for (int i : {i0, i1, o0, o1}) CHECK(p.item[i].staged);
    CHECK(p.item[i0].offset == 0 && p.item[i1].offset == 2304 && p.in_bytes == 2304 + 1024);
    CHECK(p.item[o0].offset == 0 && p.item[o1].offset == 1024 && p.out_bytes == 1024 + 256);
    CHECK(p.item[i0].ptr == a && p.item[o1].ptr == d && !p.item[i1].output && p.item[o0].output);
    check_layout(p);
  }
  {  // device items keep the caller's pointer and pitch and take nothing from the workspaces
    StagePlan p;
    const int i = p.in(a, FDOCT_MEM_DEVICE, 100, 7, 136), o = p.out(b, FDOCT_MEM_DEVICE, 4096);
    CHECK(p.rc == FDOCT_OK && !p.sync && p.in_bytes == 0 && p.out_bytes == 0);
    CHECK(!p.item[i].staged && p.item[i].ptr == a && p.item[i].dev_pitch == 136 && p.item[i].row == 100 && p.item[i].rows == 7);
    CHECK(!p.item[o].staged && p.item[o].ptr == b);
    // ... any memory space but host reads as device memory (fdoct_display's and fdoct_frontend's ABI)
    StagePlan q;
    q.in(a, (fdoct_memspace)7, 64);
    CHECK(q.rc == FDOCT_OK && !q.sync && !q.item[0].staged && q.in_bytes == 0);
  }
  {  // mixed: a device input beside a host output synchronises, and only the output is staged
    StagePlan p;
    const int i = p.in(a, FDOCT_MEM_DEVICE, 1 << 20), o = p.out(b, FDOCT_MEM_HOST, 24);
    CHECK(p.sync && !p.item[i].staged && p.item[o].staged && p.in_bytes == 0 && p.out_bytes == 256);
    check_layout(p);
  }
  {  // an absent optional output: scratch if the kernel writes it anyway, else a null pointer -- in either memory space
    for (fdoct_memspace mem : {FDOCT_MEM_HOST, FDOCT_MEM_DEVICE}) {
      StagePlan p;
      const int lo = p.out_or_scratch(nullptr, mem, 12), hi = p.out_or_scratch(a, mem, 12), no = p.out(nullptr, mem, 12);
      CHECK(p.rc == FDOCT_OK);
      CHECK(p.item[lo].staged && !p.item[lo].ptr && p.item[lo].offset == 0);
      CHECK(p.item[hi].staged == (mem == FDOCT_MEM_HOST) && p.item[hi].ptr == a);
      CHECK(!p.item[no].staged && !p.item[no].ptr);
      CHECK(p.out_bytes == (mem == FDOCT_MEM_HOST ? 512u : 256u) && p.sync == (mem == FDOCT_MEM_HOST));
      check_layout(p);
    }
    StagePlan p;  // scratch alone does not synchronise
    p.out_or_scratch(nullptr, FDOCT_MEM_HOST, 12);
    CHECK(!p.sync && p.out_bytes == 256);
  }
  {  // the 2-D form packs rows to (row + 15) & ~15, whatever the caller's pitch
    for (size_t row : {1u, 15u, 16u, 17u, 160u, 193u}) {
      StagePlan p;
      const int i = p.in(a, FDOCT_MEM_HOST, row, 5, row + 40), o = p.out(b, FDOCT_MEM_HOST, row, 3, row + 8);
      CHECK(p.item[i].dev_pitch == ((row + 15) & ~(size_t)15) && p.item[i].pitch == row + 40 && p.item[i].row == row);
      CHECK(p.item[o].dev_pitch == packed_pitch(row) && p.item[o].pitch == row + 8);
      CHECK(p.in_bytes >= 5 * packed_pitch(row) && p.out_bytes >= 3 * packed_pitch(row));
      check_layout(p);
    }
    StagePlan p;  // the flat form is one row, as long as it is
    p.in(a, FDOCT_MEM_HOST, 1001);
    CHECK(p.item[0].rows == 1 && p.item[0].row == 1001 && p.item[0].dev_pitch == 1001);
  }
  {  // the in-place pair: one device range with host memory on both sides, two items otherwise
    StagePlan p;
    const int i = p.in(a, FDOCT_MEM_HOST, 3 * 8, 20, 4 * 8), o = p.out_on(i, b, FDOCT_MEM_HOST, 5 * 8);
    CHECK(p.rc == FDOCT_OK && p.sync && p.item[o].staged && p.item[o].on_input && p.item[o].output);
    CHECK(p.item[o].offset == p.item[i].offset && p.item[o].dev_pitch == p.item[i].dev_pitch && p.item[o].rows == 20);
    CHECK(p.item[o].ptr == b && p.item[o].pitch == 5 * 8 && p.out_bytes == 0 && p.in_bytes == 768);  // (20 rows of 32 bytes)
    check_layout(p);
    StagePlan q;  // device rows in, host rows out: the output has its own range
    const int qi = q.in(a, FDOCT_MEM_DEVICE, 24, 20, 32), qo = q.out_on(qi, b, FDOCT_MEM_HOST, 24);
    CHECK(!q.item[qi].staged && q.item[qo].staged && !q.item[qo].on_input && q.in_bytes == 0 && q.out_bytes == 768);
    StagePlan r;  // host rows in, device rows out: the caller's pointer and pitch
    const int ri = r.in(a, FDOCT_MEM_HOST, 24, 20, 32), ro = r.out_on(ri, b, FDOCT_MEM_DEVICE, 40);
    CHECK(r.item[ri].staged && !r.item[ro].staged && r.item[ro].ptr == b && r.item[ro].dev_pitch == 40 && r.out_bytes == 0);
  }
  {  // sizes whose products or sums would wrap size_t are FDOCT_ERR_INVALID
    StagePlan p;
    p.in(a, FDOCT_MEM_HOST, SIZE_MAX - 100);
    CHECK(p.rc == FDOCT_ERR_INVALID);
    StagePlan q;
    q.in(a, FDOCT_MEM_HOST, SIZE_MAX / 2);
    CHECK(q.rc == FDOCT_OK);
    q.in(b, FDOCT_MEM_HOST, SIZE_MAX / 2);
    CHECK(q.rc == FDOCT_ERR_INVALID);
    StagePlan r;
    r.in(a, FDOCT_MEM_HOST, (size_t)1 << 40, (size_t)1 << 40, (size_t)1 << 40);
    CHECK(r.rc == FDOCT_ERR_INVALID);
    StagePlan s;
    s.out(a, FDOCT_MEM_HOST, SIZE_MAX - 3, 1, SIZE_MAX - 3);
    CHECK(s.rc == FDOCT_ERR_INVALID);
    StagePlan t;  // ... and so is a ninth item
    for (int k = 0; k < 8; k++) t.in(a, FDOCT_MEM_DEVICE, 1);
    CHECK(t.rc == FDOCT_OK);
    t.in(a, FDOCT_MEM_DEVICE, 1);
    CHECK(t.rc == FDOCT_ERR_INVALID && t.count == 8);
  }
  {  // vibrometry's shape: 4 x 3 x 5 pairs and the four outputs, all in host memory
    StagePlan p;
    const int in = p.in(a, FDOCT_MEM_HOST, 4 * 3 * 5 * 8);
    const int o[4] = {p.out(a, FDOCT_MEM_HOST, 120), p.out(b, FDOCT_MEM_HOST, 60), p.out(c, FDOCT_MEM_HOST, 60), p.out(d, FDOCT_MEM_HOST, 60)};
    CHECK(p.rc == FDOCT_OK && p.count == 5 && p.sync && p.item[in].staged && p.item[in].offset == 0 && p.in_bytes == 512);
    for (int k = 0; k < 4; k++) CHECK(p.item[o[k]].staged && p.item[o[k]].output && p.item[o[k]].offset == 256u * k);
    CHECK(p.out_bytes == 1024);
    check_layout(p);
  }
  {  // the dispersion search's shape: 2 x 16 pairs; sums, row sums and the winner (scratch where null), the table
    const size_t pairs = 2 * 16 * 8;
    StagePlan p;  // host memory
    p.in(a, FDOCT_MEM_HOST, pairs);
    const int o[4] = {p.out_or_scratch(a, FDOCT_MEM_HOST, 48), p.out_or_scratch(b, FDOCT_MEM_HOST, 96), p.out_or_scratch(c, FDOCT_MEM_HOST, 40),
                      p.out(d, FDOCT_MEM_HOST, 128)};
    CHECK(p.rc == FDOCT_OK && p.count == 5 && p.sync && p.item[0].staged && p.in_bytes == 256);
    for (int k = 0; k < 4; k++) CHECK(p.item[o[k]].staged && p.item[o[k]].offset == 256u * k);
    CHECK(p.item[o[2]].ptr == c && p.item[o[2]].row == 40 && p.out_bytes == 1024);
    check_layout(p);
    StagePlan q;  // device memory, no winner asked for: the winner alone is staged, as scratch
    q.in(a, FDOCT_MEM_DEVICE, pairs);
    const int qs = q.out_or_scratch(a, FDOCT_MEM_DEVICE, 48), qr = q.out_or_scratch(b, FDOCT_MEM_DEVICE, 96);
    const int qb = q.out_or_scratch(nullptr, FDOCT_MEM_DEVICE, 40), qt = q.out(d, FDOCT_MEM_DEVICE, 128);
    CHECK(q.rc == FDOCT_OK && !q.sync && q.in_bytes == 0 && q.out_bytes == 256);
    CHECK(!q.item[0].staged && !q.item[qs].staged && !q.item[qr].staged && !q.item[qt].staged && q.item[qt].ptr == d);
    CHECK(q.item[qb].staged && !q.item[qb].ptr && q.item[qb].offset == 0);
    check_layout(q);
    StagePlan r;  // host pairs, device outputs: the pairs alone are staged
    r.in(a, FDOCT_MEM_HOST, pairs);
    const int ro[4] = {r.out_or_scratch(a, FDOCT_MEM_DEVICE, 48), r.out_or_scratch(b, FDOCT_MEM_DEVICE, 96), r.out_or_scratch(c, FDOCT_MEM_DEVICE, 40),
                       r.out(d, FDOCT_MEM_DEVICE, 128)};
    CHECK(r.rc == FDOCT_OK && r.sync && r.item[0].staged && r.in_bytes == 256 && r.out_bytes == 0);
    for (int k : ro) CHECK(!r.item[k].staged);
    CHECK(r.item[ro[2]].ptr == c);
    check_layout(r);
  }
  {  // the checks the entry points share
    CHECK(valid_mem(FDOCT_MEM_HOST) && valid_mem(FDOCT_MEM_DEVICE) && !valid_mem((fdoct_memspace)7));
    CHECK(valid_layout(FDOCT_LAYOUT_ROWMAJOR_HxD) && valid_layout(FDOCT_LAYOUT_TRANSPOSED_DxH) && !valid_layout((fdoct_layout)9));
    CHECK(overlap(a, 17, b, 4) && !overlap(a, 16, b, 4) && !overlap(nullptr, 64, a, 4) && overlap(b, 4, a, 64));
    // ... and overlaps() over a call's outputs and its input: disjoint, the input on an output, two outputs, nulls left out
    const void* const out[3] = {b, c, d};
    const size_t n16[3] = {16, 16, 16}, n17[3] = {16, 17, 16};
    CHECK(overlaps(a, 16, out, n16, 3) == OVERLAP_NONE && overlaps(nullptr, 0, out, n16, 3) == OVERLAP_NONE);
    CHECK(overlaps(a, 17, out, n16, 3) == OVERLAP_INPUT && overlaps(d, 1, out, n16, 3) == OVERLAP_INPUT);
    CHECK(overlaps(a, 16, out, n17, 3) == OVERLAP_OUTPUTS && overlaps(nullptr, 64, out, n17, 3) == OVERLAP_OUTPUTS);
    const void* const same[3] = {b, nullptr, b};
    CHECK(overlaps(nullptr, 0, same, n16, 3) == OVERLAP_OUTPUTS);
    const void* const gaps[3] = {nullptr, c, nullptr};
    CHECK(overlaps(a, 64, gaps, n17, 3) == OVERLAP_INPUT && overlaps(a, 32, gaps, n17, 3) == OVERLAP_NONE && overlaps(nullptr, 64, gaps, n17, 3) == OVERLAP_NONE);
    CHECK(overlaps(a, 64, gaps, n17, 0) == OVERLAP_NONE);
    // ... and the depth range of the bulk and reference sums: inside [0, depths), a count of 0 reaching the last depth
    int n = -1;
    CHECK(!depth_range(-1, 1, 100, &n) && !depth_range(100, 0, 100, &n) && !depth_range(0, -1, 100, &n) && n == -1);
    CHECK(depth_range(30, 0, 100, &n) && n == 70);
    CHECK(depth_range(30, 70, 100, &n) && n == 70 && depth_range(99, 1, 100, &n) && n == 1 && depth_range(0, 0, 1, &n) && n == 1);
    n = -1;
    CHECK(!depth_range(30, 71, 100, &n) && !depth_range(99, 2, 100, &n) && !depth_range(0, 0, 0, &n) && n == -1);
  }
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
