// Prints make_host_call's decision (fdoct_amd/csrc/fdoct_hostcall.h) for a fixed grid of handles and calls, one line each: every
// field of the value, or the refusal and its text.  tests/test_abi.py compares the output with hostcall_check.expected, recorded
// from the arithmetic as it stood in fdoct_process and sim_last_frames before the decision became a value.  Host-only: no GPU and
// no library needed.
//
// Over nframes a combination prints both sides of every count at which the decision changes: every threshold, wherever the
// arithmetic puts it.
#include <cstdio>
#include <initializer_list>
#include <set>
#include <tuple>

#include "fdoct_hostcall.h"

using namespace fdoct;

struct Shape {
  const char* name;
  int W, H, D, binx, biny;
  size_t es;
};
static const Shape kShapes[] = {
    {"2048x1000u16", 2048, 1000, 1024, 1, 1, 2},  // C2's frames: 4 096 000 bytes
    {"1024x40u16", 1024, 40, 512, 1, 1, 2},
    {"160x120u8/2x2", 160, 120, 128, 2, 2, 1},    // 320 x 240 camera rows behind a 2 x 2 front end
    {"640x480bgr", 640, 480, 256, 1, 1, 3},       // a colour handle's 3-byte pixels
    {"4096x4096u16", 4096, 4096, 2048, 1, 1, 2},  // one frame (32 MiB) is larger than a chunk
};
static const char* kSim[] = {"asis", "strided", "gather"};
static const char* kPath[] = {"device", "single", "pipelined"};
enum Pin { ALL_PINNED, FRAMES_PAGEABLE, BSCAN_PAGEABLE, DB_PAGEABLE, DB_PAGEABLE_UNWANTED, kPins };
static const char* kPinNames[kPins] = {"pinned", "frames-pageable", "bscan-pageable", "db-pageable", "db-pageable-unwanted"};

static HostCallInputs inputs(const Shape& s, int A, int S, long long mb, fdoct_memspace in, fdoct_memspace out, int pin, size_t pad) {
  HostCallInputs i;
  i.W = s.W, i.H = s.H, i.D = s.D, i.A = A, i.sim_group = S, i.fe_binx = s.binx, i.fe_biny = s.biny;
  i.pixel_bytes = s.es;
  i.pitch_bytes = pad ? s.es * s.W * s.binx + pad : 0;
  i.frames = true;
  i.space = in, i.out_space = out;
  i.want_bscan = true, i.want_db = pin != DB_PAGEABLE_UNWANTED;
  i.frames_pinned = pin != FRAMES_PAGEABLE, i.bscan_pinned = pin != BSCAN_PAGEABLE, i.db_pinned = pin != DB_PAGEABLE && pin != DB_PAGEABLE_UNWANTED;
  i.chunk_mb = mb;
  return i;
}

static void print(const char* key, const HostCallInputs& in) {
  const HostCall c = make_host_call(in);
  std::printf("%s n=%d: ", key, in.nframes);
  if (c.rc) {
    std::printf("rc=%d %s\n", c.rc, c.why);
    return;
  }
  std::printf("%s %s first=%zu stride=%zu nframes=%d row=%zu pitch=%zu rpf=%lld in_rows=%lld out=%zu pageable=%d chunk=%zu fpc=%lld\n", kSim[(int)c.sim],
              kPath[(int)c.path], c.first_byte, c.frame_stride, c.nframes, c.row_bytes, c.pitch, c.rows_per_frame, c.in_rows, c.out_elems,
              c.pageable ? 1 : 0, c.chunk_bytes, c.frames_per_chunk);
}

// The accepted counts of one combination, up to kScan groups of S A frames: both sides of every count at which the decision changes --
// path, sim form, chunk size, frames per chunk -- and the last one.  `refusals`: the counts around one group first.
static void combination(const Shape& s, int A, int S, long long mb, fdoct_memspace in, fdoct_memspace out, int pin, size_t pad, bool refusals) {
  char key[160];
  int len = std::snprintf(key, sizeof key, "%s A=%d S=%d mb=%lld %c>%c %s", s.name, A, S, mb, in == FDOCT_MEM_HOST ? 'h' : 'd',
                          out == FDOCT_MEM_HOST ? 'h' : 'd', kPinNames[pin]);
  if (pad) std::snprintf(key + len, sizeof key - len, " pad=%zu", pad);
  HostCallInputs i = inputs(s, A, S, mb, in, out, pin, pad);
  const int g = S * A;
  std::set<int> ns = {g};
  if (refusals) ns.insert({0, 1, S, g + 1});
  const long long kScan = mb > 1 ? 330000 : 4000;  // (past 4 chunks of 100 000 MB of the smallest frames / of 16 MB)
  auto sig = [&](int n) {
    i.nframes = n;
    const HostCall c = make_host_call(i);
    return std::make_tuple(c.rc, (int)c.sim, (int)c.path, c.pageable, c.chunk_bytes, c.frames_per_chunk);
  };
  auto last = sig(g);
  for (long long k = 2; k <= kScan; k++) {
    const auto now = sig((int)(k * g));
    if (now != last) ns.insert((int)((k - 1) * g)), ns.insert((int)(k * g));
    last = now;
  }
  ns.insert((int)(kScan * g));
  for (int n : ns) {
    i.nframes = n;
    print(key, i);
  }
}

int main() {
  const fdoct_memspace Hm = FDOCT_MEM_HOST, Dm = FDOCT_MEM_DEVICE;
  // host memory on both sides: every shape, averages and sim group, all pinned and (the 16-bit shapes) the frames pageable
  for (const Shape& s : kShapes)
    for (int A : {1, 2, 3, 16})
      for (int S : {1, 3})
        for (int pin : {ALL_PINNED, FRAMES_PAGEABLE})
          if (pin == ALL_PINNED || s.es == 2) combination(s, A, S, 0, Hm, Hm, pin, 0, &s == kShapes && pin == ALL_PINNED);
  // ... with the chunk override
  for (const Shape& s : kShapes)
    for (long long mb : {1LL, 100000LL})
      for (int A : {1, 16})
        for (int S : {1, 3}) combination(s, A, S, mb, Hm, Hm, A == 1 ? ALL_PINNED : FRAMES_PAGEABLE, 0, false);
  // the other memory spaces: nothing to chunk, the sim variant gathers
  for (const Shape& s : {kShapes[1], kShapes[3]})
    for (int A : {1, 3})
      for (int S : {1, 3}) {
        combination(s, A, S, 0, Hm, Dm, FRAMES_PAGEABLE, 0, false);
        combination(s, A, S, 0, Dm, Hm, ALL_PINNED, 0, false);
        combination(s, A, S, 0, Dm, Dm, ALL_PINNED, 0, A == 3);
      }
  // one output buffer pageable, wanted and not; a padded pitch
  for (const Shape& s : {kShapes[0], kShapes[2]})
    for (int S : {1, 3}) {
      for (int pin : {BSCAN_PAGEABLE, DB_PAGEABLE, DB_PAGEABLE_UNWANTED}) combination(s, 1, S, 0, Hm, Hm, pin, 0, false);
      combination(s, 1, S, 0, Hm, Hm, ALL_PINNED, 48, false);
      combination(s, 1, S, 0, Dm, Dm, ALL_PINNED, 48, false);
    }
  {  // the refusals that do not depend on the batch
    HostCallInputs i = inputs(kShapes[0], 2, 1, 0, Hm, Hm, ALL_PINNED, 0);
    i.nframes = 3, i.pixel_bytes = 0;
    print("bad dtype, before the averages", i);
    i.pixel_bytes = 2, i.frames = false;
    print("null frames", i);
    i.frames = true, i.nframes = -1;
    print("a negative count", i);
  }
  {  // rows derived by hand from the code as it stood (tests/test_abi.py states them): C2's frames, host memory on both sides
    const Shape& c2 = kShapes[0];
    for (int n : {3, 4, 24, 25}) {
      HostCallInputs i = inputs(c2, 1, 1, 0, Hm, Hm, ALL_PINNED, 0);
      i.nframes = n;
      print("hand: C2 pinned", i);
    }
    for (int n : {15, 16}) {
      HostCallInputs i = inputs(c2, 1, 1, 0, Hm, Hm, DB_PAGEABLE, 0);
      i.nframes = n;
      print("hand: C2 one pageable", i);
    }
    for (int pin : {ALL_PINNED, FRAMES_PAGEABLE})
      for (int n : {3, 30}) {
        HostCallInputs i = inputs(c2, 3, 1, 0, Hm, Hm, pin, 0);
        i.nframes = n;
        print(pin == ALL_PINNED ? "hand: C2 A=3 pinned" : "hand: C2 A=3 pageable", i);
      }
    for (int A : {1, 2, 3, 16})
      for (int pin : {ALL_PINNED, FRAMES_PAGEABLE}) {
        HostCallInputs i = inputs(kShapes[4], A, 1, 0, Hm, Hm, pin, 0);
        i.nframes = 48;
        char key[64];
        std::snprintf(key, sizeof key, "hand: frame above the chunk A=%d %s", A, kPinNames[pin]);
        print(key, i);
      }
    // the sim variant, S = 3: 180 frames of 1024 x 40 u16 with 1 MB chunks; and the same batch into device outputs
    HostCallInputs i = inputs(kShapes[1], 1, 3, 1, Hm, Hm, ALL_PINNED, 0);
    i.nframes = 180;
    print("hand: sim host>host", i);
    i.out_space = Dm;
    print("hand: sim host>device", i);
  }
  return 0;
}
