// fdoct_route_value.h -- the route of a call as a value: which passes run in front of the chain, whether the 2 x 2 binning goes into
// the kernel, which kernel family takes the call and that family's launch (the fused family's from fdoct_launch.h; waves, LDS and
// grid of the wave-per-row and workgroup-per-row families), which device tables the call needs -- or why the call is refused
// (make_route).  Plain C++ without HIP, like the planner and the launch value: tests/native/route_check.cpp pins it without a GPU.
// choose_route (fdoct_route.cpp) builds the inputs from handle and call and carries the decision out.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/fdoct.h"
#include "fdoct_launch.h"
#include "fdoct_wave_rules.h"

namespace fdoct {

// Each family's device tables (fdoct_state.cpp: ensure_*_tables builds a set when it does not match the host state).
enum : unsigned { TABLES_FUSED = 1, TABLES_GENERIC = 2, TABLES_WAVE = 4 };

enum class PrePass {  // the pass that produces what the chain's kernel reads
  None,               // the caller's frames (or the front end's output) as they are
  F64Split,           // data_y doubles split once into two f32 planes, hi + lo (main:987)
  MovAvg,             // smoothmovavg (main:990-991), one f32 plane
  MovAvgF64,          // ... of doubles: the tap sums in double, two planes
  MovAvgF32Wide,      // ... of FLOAT frames likewise (their samples need not be integers)
};

// Everything the decision reads of the handle and of the call (pointers enter as addresses: only their alignment matters).
struct RouteInputs {
  int W = 0, H = 0, N = 0, D = 0, M = 1, A = 1;
  const Plan* plan = nullptr;   // the handle's adopted plan
  // reference frames and processing options
  int bg_rows = 1;              // background: one spectrum, or a full frame of H rows
  bool pi = false, dark = false, bandpass = false, rowwisenormalize = false;
  bool normalize = false;       // the whole-frame normalisation is on (the sim variant, or donotnormalize off)
  bool phase = false;           // a dispersion phase is set
  int movavgn = 0;
  // in front of the chain
  int fe_median = 0, fe_binx = 1, fe_biny = 1;
  int colour = -1;              // fdoct_set_colour_input: -1 mono frames, 0-2 a channel, 3 the sum
  // switches and overrides
  bool jit = true, staged = false;
  int plan_override = -1, block_override = 0, grid_override = 0, num_cu = 256;
  bool precise_div = true, force_general = false, tro_enabled = true;
  unsigned ring_cap = 0;        // FDOCT_TRO_RING (FusedLaunchInputs::ring_cap)
  // the call
  int dtype = FDOCT_U16;        // fdoct_dtype of the caller's frames
  uintptr_t frames_addr = 0;
  size_t pitch_bytes = 0;
  uintptr_t out_bscan_addr = 0, out_db_addr = 0;
  int layout = FDOCT_LAYOUT_ROWMAJOR_HxD;
  int nframes = 0;
  // the complex A-scan (enqueue_complex): the same checks and passes in front of the chain, the family restricted to the two whose
  // kernels write it -- the wave-per-row kernel compiled at run time with FDOCT_WAVE_OPT_CXOUT for every shape it takes, the
  // workgroup-per-row kernel for the rest -- whatever the handle's plan; rows only the long-row path takes are refused
  bool cx = false;
};

struct RouteDecision {
  int family = FDOCT_KERNEL_NONE;   // fdoct_kernel: who runs the chain
  bool frontend = false;            // medianBlur + binning pass over the raw frames first (main:953-958)
  bool colour = false;              // the colour stage first (webcam:1015-1038), median / binning included: the rest is routed as its output is
  PrePass pre = PrePass::None;
  int kdt = -1;                     // sample type the chain's kernel reads (FDOCT_K_*)
  size_t kpitch = 0;                // ... and its row pitch
  bool need_minmax = false;         // whole-frame min / max pre-pass (main:1128)
  bool transpose_pass = false;      // a transpose pass makes the D x H layout (the fused chain does not write it itself: fused.tro)
  bool bin2_in_kernel = false;      // FDOCT_KERNEL_WAVE_JIT: the 2 x 2 software binning inside the kernel's loads (the raw frames go to it as they are)
  int wave_opt = 0;                 // FDOCT_WAVE_OPT_* of that kernel
  FusedLaunch fused;                // the fused families: the launch (fdoct_launch.h)
  int waves = 0;                    // the wave-per-row families: waves per workgroup ...
  size_t lds = 0;                   // ... and, for the generic family too, dynamic LDS ...
  long long grid = 0;               // ... and workgroups
  unsigned tables = 0;              // TABLES_* the call needs on the device
  const char* note = nullptr;       // what the decision itself leaves in fdoct_jit_note (the long-row path's cliff), or null
  bool frames_lo() const { return pre == PrePass::F64Split || pre == PrePass::MovAvgF64 || pre == PrePass::MovAvgF32Wide; }  // a plane of low words goes along
};

// The one question the decision cannot answer from its inputs: does the run-time compiler deliver wave_kernel for the handle's
// geometry, samples of type kdt (FDOCT_K_*) and these FDOCT_WAVE_OPT_* bits?  Whoever answers keeps the kernel and the reason.
using CanCompile = bool (*)(void* ctx, int kdt, int wave_opt);

// The route of a call: FDOCT_OK and *out, or an error code with the refusal's text in *why (*out is then untouched; *why is written
// on refusal only).  Reads nothing but its arguments and asks can_compile only for kernels the call would run.
int make_route(const RouteInputs& in, CanCompile can_compile, void* ctx, RouteDecision* out, std::string* why);
// make_route's first refusals, which look at no option of the route: the complex call on long rows, a generic plan that carries an
// error, D > N, what a colour handle cannot take.  A call refused here has no route: choose_route leaves fdoct_jit_note as it was.
int route_precheck(const RouteInputs& in, std::string* why);

int kernel_dtype(int dt);     // FDOCT_K_* of an fdoct_dtype the kernels read as it is, else -1
size_t dtype_size(int dt);    // bytes per sample of an fdoct_dtype, 0 for none
// rows of the front end's workspaces: packed, 16-byte-pitched
inline size_t frontend_pitch(int w, size_t es) { return ((size_t)w * es + 15) & ~(size_t)15; }
// What a colour stage can do (`who` prefixes the message): 8-bit frames only, no median in front of the sum (cv::medianBlur
// rejects CV_64F: there is no reference behaviour to match).
int colour_refusal(const char* who, int channelnum, int dtype, int mediann, std::string* why);

}  // namespace fdoct
