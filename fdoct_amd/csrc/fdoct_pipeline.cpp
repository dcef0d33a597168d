// fdoct_pipeline.cpp -- fdoct_process with host buffers on both sides and a batch worth chunking (fdoct_hostcall.h decides that):
// the three-stream pipeline over the handle's chunk slots, and the copy threads that feed it from pageable memory.
#include "fdoct_ctx.h"

namespace fdoct_impl {

static bool host_staging_enabled(const fdoct_ctx* h) {
  bool on = h->host_staging != 0;
  if (const char* e = std::getenv("FDOCT_HOST_STAGING")) on = on && std::atoi(e) != 0;
  return on;
}

// Is this host pointer pinned (hipHostMalloc / hipHostRegister), i.e. can a DMA engine reach it without the runtime's bounce
// buffer?  Pageable memory is "unregistered" to the runtime (an error from hipPointerGetAttributes on older runtimes).
bool host_pointer_is_pinned(const void* p) {
  hipPointerAttribute_t a;
  std::memset(&a, 0, sizeof a);
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

// The copy threads of a handle (fdoct_hostcopy.h), started with the first batch that needs them.  An explicit count
// (fdoct_set_host_staging(h, n) or FDOCT_HOST_COPY_THREADS) is taken as given.  Left to the library: half of the hardware
// threads this process may use, eight at most, the caller's thread among them -- and NO staging below four, because one or two threads
// copy more slowly than the runtime's own bounce path (MI355X host, 64 frames of 2048 x 1000 u16 per call, result array
// reused: 3.2-3.4 / 5.9-6.0 / 8.4-8.7 / 8.4-9.4 M A-scans/s with 1 / 2 / 4 / 8 threads against 6.0-6.4 M from the runtime and 10.5 M from pinned
// buffers; profiles/r06_pcie_rate.txt).
int copy_thread_count(const fdoct_ctx* h) {  // 0: pageable buffers are not staged
  if (!host_staging_enabled(h)) return 0;
  int n = h->host_staging > 0 ? h->host_staging : 0;
  if (!n)
    if (const char* e = std::getenv("FDOCT_HOST_COPY_THREADS")) n = std::atoi(e);
  if (n <= 0) {
    n = std::min(8, (int)std::thread::hardware_concurrency() / 2);
    if (n < 4) return 0;
  }
  return std::min(n, 64);
}

static HostCopyPool* copy_pool(fdoct_ctx* h) {
  const int n = copy_thread_count(h);
  if (!n) return nullptr;
  if (!h->copy_pool) h->copy_pool.reset(new (std::nothrow) HostCopyPool(n));
  return h->copy_pool.get();
}

// Host buffers in, host buffers out, more than one chunk of work: the batch is cut into chunks of whole averaging
// groups and pipelined over three streams -- chunk c+1 uploads while chunk c computes and chunk c-1 downloads (the
// two PCIe directions and the kernels overlap when the caller's buffers are pinned, e.g. from fdoct_host_alloc;
// pageable buffers still work, the runtime then stages them and the host thread serialises the copies).
int process_pipelined(fdoct_ctx* h, const HostCall& call, const void* batch, fdoct_dtype dtype, float* out_bscan, float* out_db,
                      fdoct_layout layout) {
  const unsigned char* frames = static_cast<const unsigned char*>(batch) + call.first_byte;
  const int nframes = call.nframes, frames_per_chunk = (int)call.frames_per_chunk;  // (at least two chunks: it fits)
  const size_t src_pitch = call.pitch, row_bytes = call.row_bytes, frame_stride = call.frame_stride, rows_per_frame = (size_t)call.rows_per_frame;
  std::unique_ptr<fdoct_ctx, void (*)(fdoct_ctx*)> drain_on_failure(h, drain);  // every return but the last: nothing stays in flight
  int rc;
  const bool packed_batch = frame_stride == (size_t)rows_per_frame * src_pitch;  // one 2-D copy moves a whole chunk
  // Pageable buffers go through the handle's pinned slots (fdoct_hostcopy.h); pinned ones are the DMA engines' to read and write.
  HostCopyPool* pool = copy_pool(h);
  bool stage_in = pool && !host_pointer_is_pinned(frames);
  bool stage_mag = pool && out_bscan && !host_pointer_is_pinned(out_bscan);
  bool stage_db = pool && out_db && !host_pointer_is_pinned(out_db);
  struct Landed {  // a chunk whose downloads go to (or sit in) the pinned slots and still have to reach the caller's buffers
    size_t o0 = 0, elems = 0;
    bool live = false;
  } landed[2];
  auto hand_over = [&](int b) -> int {
    if (!landed[b].live) return FDOCT_OK;
    HIP_TRY(h, hipEventSynchronize(h->pe_out[b]));
    if (stage_mag) pool->copy(out_bscan + landed[b].o0, h->pin_mag[b], landed[b].elems * 4);
    if (stage_db) pool->copy(out_db + landed[b].o0, h->pin_db[b], landed[b].elems * 4);
    landed[b].live = false;
    return FDOCT_OK;
  };
  if (!h->s_in) {
    HIP_TRY(h, hipStreamCreateWithFlags(&h->s_in, hipStreamNonBlocking));
    HIP_TRY(h, hipStreamCreateWithFlags(&h->s_out, hipStreamNonBlocking));
    for (int b = 0; b < 2; b++) {
      HIP_TRY(h, hipEventCreateWithFlags(&h->pe_in[b], hipEventDisableTiming));
      HIP_TRY(h, hipEventCreateWithFlags(&h->pe_k[b], hipEventDisableTiming));
      HIP_TRY(h, hipEventCreateWithFlags(&h->pe_out[b], hipEventDisableTiming));
    }
  }
  const size_t packed = packed_pitch(row_bytes);
  const size_t out_per_group = (size_t)h->H * h->D;  // output floats per averaging group: chunks are whole groups (H D / A per input
                                                     // frame is not an integer in general -- 251 lines, 18 bins, 16 averages)
  const hipStream_t s_k = h->stream;
  h->record_now = false;
  {
    // The pinned slots, sized for the first (the largest) chunk, before anything is enqueued: a host that will not pin that
    // much memory (a locked-memory limit) gets the runtime's own bounce copies for that buffer, not an error.
    const int nf0 = std::min(frames_per_chunk, nframes);
    const size_t in0 = packed * (size_t)nf0 * (size_t)rows_per_frame, out0 = (size_t)(nf0 / h->A) * out_per_group * 4;
    const std::string err_before = h->err;
    for (int b = 0; b < 2; b++) {
      if (stage_in && h->pin_in[b].reserve(h, in0)) stage_in = false;
      if (stage_mag && h->pin_mag[b].reserve(h, out0)) stage_mag = false;
      if (stage_db && h->pin_db[b].reserve(h, out0)) stage_db = false;
    }
    h->err = err_before;
  }
  uint64_t sum_in = 0, sum_out = 0;  // fdoct_get_timing reports the whole batch, not the last chunk
  for (int f0 = 0, c = 0; f0 < nframes; f0 += frames_per_chunk, c++) {
    const int b = c & 1;
    const int nf = std::min(frames_per_chunk, nframes - f0);
    const size_t in_rows = (size_t)nf * rows_per_frame;
    const size_t out_elems = (size_t)(nf / h->A) * out_per_group;
    if ((rc = h->pl_in[b].reserve(h, packed * in_rows))) return rc;
    if (out_bscan && (rc = h->pl_mag[b].reserve(h, out_elems * 4))) return rc;
    if (out_db && (rc = h->pl_db[b].reserve(h, out_elems * 4))) return rc;
    const unsigned char* src = frames + (size_t)f0 * frame_stride;
    // a packed batch moves as one 2-D copy of the chunk's rows, a strided one frame by frame
    const int pieces = packed_batch ? 1 : nf;
    const size_t piece_rows = packed_batch ? in_rows : (size_t)rows_per_frame;
    if (stage_in) {
      if (c >= 2) HIP_TRY(h, hipEventSynchronize(h->pe_in[b]));           // chunk c-2's upload has left this pinned slot
      for (int q = 0; q < pieces; q++)
        pool->copy2d(static_cast<unsigned char*>(h->pin_in[b]) + (size_t)q * piece_rows * packed, packed, src + (size_t)q * frame_stride, src_pitch,
                     row_bytes, piece_rows);
    }
    if (c >= 2) HIP_TRY(h, hipStreamWaitEvent(h->s_in, h->pe_k[b], 0));   // chunk c-2 has consumed this input slot
    if (stage_in) {
      HIP_TRY(h, hipMemcpyAsync(h->pl_in[b], h->pin_in[b], packed * in_rows, hipMemcpyHostToDevice, h->s_in));
    } else {
      for (int q = 0; q < pieces; q++)
        HIP_TRY(h, hipMemcpy2DAsync(static_cast<unsigned char*>(h->pl_in[b]) + (size_t)q * piece_rows * packed, packed, src + (size_t)q * frame_stride,
                                    src_pitch, row_bytes, piece_rows, hipMemcpyHostToDevice, h->s_in));
    }
    HIP_TRY(h, hipEventRecord(h->pe_in[b], h->s_in));
    HIP_TRY(h, hipStreamWaitEvent(s_k, h->pe_in[b], 0));
    if (c >= 2) HIP_TRY(h, hipStreamWaitEvent(s_k, h->pe_out[b], 0));     // chunk c-2 has left this output slot
    if ((rc = enqueue(h, h->pl_in[b], dtype, nf, packed, out_bscan ? h->pl_mag[b] : nullptr, out_db ? h->pl_db[b] : nullptr, layout)))
      return rc;
    sum_in += h->timing.bytes_in;
    sum_out += h->timing.bytes_out;
    HIP_TRY(h, hipEventRecord(h->pe_k[b], s_k));
    HIP_TRY(h, hipStreamWaitEvent(h->s_out, h->pe_k[b], 0));
    const size_t o0 = (size_t)(f0 / h->A) * out_per_group;
    // chunk c-2's images leave the pinned slots (while chunk c uploads and computes) before chunk c's download may land there
    if ((rc = hand_over(b))) return rc;
    if (out_bscan) HIP_TRY(h, hipMemcpyAsync(stage_mag ? h->pin_mag[b] : out_bscan + o0, h->pl_mag[b], out_elems * 4, hipMemcpyDeviceToHost, h->s_out));
    if (out_db) HIP_TRY(h, hipMemcpyAsync(stage_db ? h->pin_db[b] : out_db + o0, h->pl_db[b], out_elems * 4, hipMemcpyDeviceToHost, h->s_out));
    HIP_TRY(h, hipEventRecord(h->pe_out[b], h->s_out));
    landed[b].o0 = o0;
    landed[b].elems = out_elems;
    landed[b].live = stage_mag || stage_db;
  }
  HIP_TRY(h, hipStreamSynchronize(h->s_out));
  HIP_TRY(h, hipStreamSynchronize(s_k));
  for (int b = 0; b < 2; b++)
    if ((rc = hand_over(b))) return rc;
  h->timing.bytes_in = sum_in;
  h->timing.bytes_out = sum_out;
  (void)drain_on_failure.release();
  return FDOCT_OK;
}

}  // namespace fdoct_impl
