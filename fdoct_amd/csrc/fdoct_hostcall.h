// fdoct_hostcall.h -- what fdoct_process / fdoct_process_async decide about a call on the host, as a value made before anything is
// enqueued: the refusals that need no route, how the sim variant's frames are taken, the geometry of the batch, and whether host
// buffers are pipelined in chunks (fdoct_pipeline.cpp), staged in one shot (fdoct_stage.h) or not there at all.  Plain C++ without
// HIP: tests/native/hostcall_check.cpp pins it against hostcall_check.expected.
#pragma once
#include <algorithm>
#include <cstddef>

#include "../../include/fdoct.h"

namespace fdoct {

struct HostCallInputs {
  int W = 0, H = 0, D = 0, A = 1, sim_group = 1, fe_binx = 1, fe_biny = 1;  // of the handle
  size_t pixel_bytes = 0, pitch_bytes = 0;  // frame_pixel_bytes (0 = bad dtype); the pitch as passed (0 = packed rows)
  bool frames = false;                      // the frames pointer is not null
  int nframes = 0;
  fdoct_memspace space = FDOCT_MEM_DEVICE, out_space = FDOCT_MEM_DEVICE;
  bool want_bscan = false, want_db = false;
  bool frames_pinned = true, bscan_pinned = true, db_pinned = true;  // (read with host memory on both sides only)
  long long chunk_mb = 0;                   // FDOCT_HOST_CHUNK_MB, a tuning aid (tools/pcie_chunk.py): 0 = none
};
enum class SimFrames { AsIs, Strided, Gather };
enum class HostPath { Device, SingleShot, Pipelined };

struct HostCall {
  int rc = FDOCT_OK;
  const char* why = "";  // the refusal's text
  // The sim variant with averages = S > 1 (sim:936-947) keeps the LAST of every S frames: frame g S + S - 1 of group g, nframes / S
  // of them, first_byte into the batch and frame_stride apart.  Strided: the pipeline's chunks read them where they lie.  Gather:
  // one strided copy packs them into ws_sim first (no host batch worth chunking), and the call goes on device-resident frames.
  SimFrames sim = SimFrames::AsIs;
  HostPath path = HostPath::Device;  // Device: no argument in host memory; SingleShot: those that are go through a StagePlan
  size_t first_byte = 0, frame_stride = 0;  // of the frames the chain takes, in the caller's memory
  int nframes = 0;                          // ... and how many
  size_t row_bytes = 0, pitch = 0;          // a row's samples; rows are `pitch` apart in the caller's memory
  long long rows_per_frame = 0, in_rows = 0;  // raw camera rows when a front end is set
  size_t out_elems = 0;                     // floats per output
  bool pageable = false;                    // host memory on both sides and a buffer that is not pinned
  size_t chunk_bytes = 0;
  long long frames_per_chunk = 0;           // whole averaging groups: more than chunk_bytes where a group is
};

// Host buffers on both sides: the batch is cut into chunks of whole averaging groups and pipelined (process_pipelined).  Chunk
// size and the batch that is worth chunking, from tools/pcie_chunk.py (profiles/r06_pcie_chunk.txt, M A-scans/s on C2's frames;
// round 5 had 32 MB chunks and two of them as the threshold).  Pinned buffers: 16 MB chunks for batches of ~100 MB and more,
// 8 MB below, two chunks are worth it (15 / 31 / 62 / 125 MB in: 7.3 / 8.6 / 9.5 / 10.1 against 6.3 / 6.6 / 8.3 / 9.6).
// Pageable buffers (staged by the copy threads): 16 MB chunks, four of them or the single shot (62 / 125 / 250 MB in:
// 6.9-7.1 / 8.3 / 8.5-9.1 against 6.2-6.5 / 6.6-7.4 / 8.5-8.7; 8 MB chunks lose to the single shot at 31 MB).
inline HostCall make_host_call(const HostCallInputs& in) {
  HostCall c;
  auto refuse = [&c](const char* why) { return c.rc = FDOCT_ERR_INVALID, c.why = why, c; };
  if (!in.frames || in.nframes <= 0) return refuse("no frames");
  if (!in.pixel_bytes) return refuse("bad dtype");
  const int S = in.sim_group > 1 ? in.sim_group : 1;
  if (in.nframes % S || in.nframes / S % in.A) return refuse("nframes must be a multiple of averages");
  const bool in_host = in.space == FDOCT_MEM_HOST, out_host = in.out_space == FDOCT_MEM_HOST;
  c.nframes = in.nframes / S;
  c.row_bytes = in.pixel_bytes * (size_t)in.W * in.fe_binx;
  c.pitch = in.pitch_bytes ? in.pitch_bytes : c.row_bytes;
  c.rows_per_frame = (long long)in.H * in.fe_biny, c.in_rows = c.nframes * c.rows_per_frame;
  c.out_elems = (size_t)(c.nframes / in.A) * in.H * in.D;
  const size_t frame_bytes = c.row_bytes * (size_t)c.rows_per_frame, frame_pitch = c.pitch * (size_t)c.rows_per_frame;
  c.first_byte = (size_t)(S - 1) * frame_pitch, c.frame_stride = (size_t)S * frame_pitch;
  c.pageable = in_host && out_host && (!in.frames_pinned || (in.want_bscan && !in.bscan_pinned) || (in.want_db && !in.db_pinned));
  c.chunk_bytes = c.pageable || frame_bytes * (size_t)c.nframes >= ((size_t)96 << 20) ? (size_t)16 << 20 : (size_t)8 << 20;
  if (in.chunk_mb > 0) c.chunk_bytes = (size_t)in.chunk_mb << 20;
  c.frames_per_chunk = std::max<long long>((long long)(c.chunk_bytes / std::max<size_t>(frame_bytes, 1)) / in.A, 1) * in.A;
  const bool pipelined = in_host && out_host && c.nframes >= (c.pageable ? 4 : 2) * c.frames_per_chunk;
  c.sim = S == 1 ? SimFrames::AsIs : pipelined ? SimFrames::Strided : SimFrames::Gather;
  const bool staged = (in_host && c.sim != SimFrames::Gather) || out_host;
  c.path = pipelined ? HostPath::Pipelined : staged ? HostPath::SingleShot : HostPath::Device;
  return c;
}

}  // namespace fdoct
