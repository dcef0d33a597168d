// fdoct_prepass_launch.inc -- the launchers of the kernels of fdoct_prepass_kernels.inc (declared in fdoct_kernels.h).  Included by
// fdoct_kernels.hip behind the fused dispatch: the kernel templates are instantiated here, and the order of a translation
// unit's kernels in the code object follows it.
int minmax_partial_count(int nframes) { return nframes * MINMAX_PARTS; }

hipError_t launch_minmax(const void* frames, int dtype, long long pitch_bytes, int W, int H, int nframes,
                         const float* yd, int yd_2d, float2* out, float2* partial, hipStream_t st) {
  const int es = dtype == FDOCT_K_U16 ? 2 : 1;
  if (!yd && partial && (dtype == FDOCT_K_U16 || dtype == FDOCT_K_U8) && (W * es) % 16 == 0 && pitch_bytes % 16 == 0 &&
      (reinterpret_cast<uintptr_t>(frames) % 16) == 0) {
    // frames ride in gridDim.y (<= 65535 per launch): longer batches go in slices
    for (int f0 = 0; f0 < nframes; f0 += 65535) {
      const int nf = nframes - f0 < 65535 ? nframes - f0 : 65535;
      const dim3 g(MINMAX_PARTS, nf), b(256);
      const void* fr = static_cast<const unsigned char*>(frames) + (long long)f0 * H * pitch_bytes;
      float2* part = partial + (size_t)f0 * MINMAX_PARTS;
      if (dtype == FDOCT_K_U16)
        hipLaunchKernelGGL(minmax_fast_kernel<uint16_t>, g, b, 0, st, fr, pitch_bytes, W * es / 16, H, part);
      else
        hipLaunchKernelGGL(minmax_fast_kernel<uint8_t>, g, b, 0, st, fr, pitch_bytes, W * es / 16, H, part);
    }
    hipLaunchKernelGGL(minmax_finish_kernel, dim3((nframes + 255) / 256), dim3(256), 0, st, partial, MINMAX_PARTS, nframes, out);
    return hipGetLastError();
  }
  dim3 g(nframes), b(1024);
  switch (dtype) {
    case FDOCT_K_U16: hipLaunchKernelGGL(minmax_kernel<uint16_t>, g, b, 0, st, frames, pitch_bytes, W, H, yd, yd_2d, out); break;
    case FDOCT_K_U8: hipLaunchKernelGGL(minmax_kernel<uint8_t>, g, b, 0, st, frames, pitch_bytes, W, H, yd, yd_2d, out); break;
    case FDOCT_K_F32: hipLaunchKernelGGL(minmax_kernel<float>, g, b, 0, st, frames, pitch_bytes, W, H, yd, yd_2d, out); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_transpose(const float* in, float* out, int rows, int cols, int groups, hipStream_t st) {
  // groups ride in gridDim.z and row tiles in gridDim.y (<= 65535 each per launch): more go in slices
  const int ytiles = (rows + 31) / 32;
  if (ytiles > 65535) return hipErrorInvalidValue;  // > 2 M rows per B-scan
  const bool wide = rows % 4 == 0 && cols % 4 == 0 && ((uintptr_t)in % 16 == 0) && ((uintptr_t)out % 16 == 0);
  for (int g0 = 0; wide && g0 < groups; g0 += 65535) {
    const int ng = groups - g0 < 65535 ? groups - g0 : 65535;
    const size_t off = (size_t)g0 * rows * cols;
    hipLaunchKernelGGL(transpose64_kernel, dim3((cols + 63) / 64, (rows + 63) / 64, ng), dim3(256), 0, st, in + off, out + off, rows, cols);
  }
  if (wide) return hipGetLastError();
  for (int g0 = 0; g0 < groups; g0 += 65535) {
    const int ng = groups - g0 < 65535 ? groups - g0 : 65535;
    const size_t off = (size_t)g0 * rows * cols;
    dim3 b(32, 8), g((cols + 31) / 32, ytiles, ng);
    hipLaunchKernelGGL(transpose_kernel, g, b, 0, st, in + off, out + off, rows, cols);
  }
  return hipGetLastError();
}

hipError_t launch_f64_split(const double* in, long long pitch_elems, float* hi, float* lo, int W, long long rows, hipStream_t st) {
  hipLaunchKernelGGL(f64_split_kernel, dim3(2048), dim3(256), 0, st, in, pitch_elems, hi, lo, W, rows);
  return hipGetLastError();
}

