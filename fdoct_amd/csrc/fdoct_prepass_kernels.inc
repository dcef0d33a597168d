// fdoct_prepass_kernels.inc -- the small kernels in front of and behind the fused chain: whole-frame min / max, the transpose
// pass and the f64 -> two f32 planes split.  Included by fdoct_kernels.hip (inside namespace fdoct) in the one translation
// unit that is not a per-plan one; their launchers are in fdoct_prepass_launch.inc.
// Whole-frame min/max (main:1128-1129) of the raw samples, one float2 per frame.
template <typename IN_T>
__global__ void minmax_kernel(const void* frames, long long pitch_bytes, int W, int H, const float* yd,
                              int yd_2d, float2* out) {
  const int f = blockIdx.x;
  const unsigned char* base = static_cast<const unsigned char*>(frames) + (long long)f * H * pitch_bytes;
  float mn = INFINITY, mx = -INFINITY;
  for (int r = 0; r < H; r++) {
    const IN_T* row = reinterpret_cast<const IN_T*>(base + (long long)r * pitch_bytes);
    for (int i = threadIdx.x; i < W; i += blockDim.x) {
      float x = (float)row[i];
      if (yd) x -= yd[(yd_2d ? (size_t)r * W : 0) + i];
      mn = fminf(mn, x);
      mx = fmaxf(mx, x);
    }
  }
  __shared__ float smn[16], smx[16];
  mn = group_min<64>(mn);
  mx = group_max<64>(mx);
  if ((threadIdx.x & 63) == 0) {
    smn[threadIdx.x >> 6] = mn;
    smx[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) {
      mn = fminf(mn, smn[w]);
      mx = fmaxf(mx, smx[w]);
    }
    out[f] = make_float2(mn, mx);
  }
}

// The same for plain integer camera frames (no dark frame, 16-byte-aligned rows): a streaming reduction with
// 16-byte loads and packed 16-bit min/max, MINMAX_PARTS workgroups per frame, then one thread per frame folds the
// partial results.  HBM-bound: one read of the batch.
constexpr int MINMAX_PARTS = 16;
typedef unsigned short us2 __attribute__((ext_vector_type(2)));

template <typename IN_T>
__global__ __launch_bounds__(256) void minmax_fast_kernel(const void* frames, long long pitch_bytes, int row_vecs, int H,
                                                           float2* partial) {
  const int f = blockIdx.y;
  const unsigned char* base = static_cast<const unsigned char*>(frames) + (long long)f * H * pitch_bytes;
  us2 mn = (us2){0xffff, 0xffff}, mx = (us2){0, 0};
  auto fold = [&](unsigned w) {
    if constexpr (sizeof(IN_T) == 2) {
      const us2 x = __builtin_bit_cast(us2, w);
      mn = __builtin_elementwise_min(mn, x);
      mx = __builtin_elementwise_max(mx, x);
    } else {  // four bytes: even and odd ones as two 16-bit pairs
      const us2 x0 = __builtin_bit_cast(us2, w & 0x00ff00ffu), x1 = __builtin_bit_cast(us2, (w >> 8) & 0x00ff00ffu);
      mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(x0, x1));
      mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(x0, x1));
    }
  };
  for (int r = blockIdx.x; r < H; r += gridDim.x) {
    const uint4* row = reinterpret_cast<const uint4*>(base + (long long)r * pitch_bytes);
    for (int v = threadIdx.x; v < row_vecs; v += blockDim.x) {
      const uint4 q = row[v];
      fold(q.x);
      fold(q.y);
      fold(q.z);
      fold(q.w);
    }
  }
  unsigned lo = mn.x < mn.y ? mn.x : mn.y, hi = mx.x > mx.y ? mx.x : mx.y;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned l2 = __shfl_xor(lo, m, 64), h2 = __shfl_xor(hi, m, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  __shared__ unsigned slo[4], shi[4];
  if ((threadIdx.x & 63) == 0) {
    slo[threadIdx.x >> 6] = lo;
    shi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) {
      lo = slo[w] < lo ? slo[w] : lo;
      hi = shi[w] > hi ? shi[w] : hi;
    }
    partial[(size_t)f * gridDim.x + blockIdx.x] = make_float2((float)lo, (float)hi);
  }
}

__global__ void minmax_finish_kernel(const float2* partial, int parts, int nframes, float2* out) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nframes) return;
  float2 r = partial[(size_t)f * parts];
  for (int i = 1; i < parts; i++) {
    const float2 p = partial[(size_t)f * parts + i];
    r.x = fminf(r.x, p.x);
    r.y = fmaxf(r.y, p.y);
  }
  out[f] = r;
}

// (rows x cols) -> (cols x rows) per group, through a 32x33 LDS tile.
__global__ void transpose_kernel(const float* in, float* out, int rows, int cols) {
  __shared__ float tile[32][33];
  const size_t goff = (size_t)blockIdx.z * rows * cols;
  int x = blockIdx.x * 32 + threadIdx.x;
  int y0 = blockIdx.y * 32;
  for (int j = threadIdx.y; j < 32; j += blockDim.y) {
    int y = y0 + j;
    if (x < cols && y < rows) tile[j][threadIdx.x] = in[goff + (size_t)y * cols + x];
  }
  __syncthreads();
  int ox = blockIdx.y * 32 + threadIdx.x;  // row index of input
  int oy0 = blockIdx.x * 32;
  for (int j = threadIdx.y; j < 32; j += blockDim.y) {
    int oy = oy0 + j;  // col index of input
    if (ox < rows && oy < cols) out[goff + (size_t)oy * rows + ox] = tile[threadIdx.x][j];
  }
}

// The same for rows and cols that are multiples of 4 (every B-scan of the bench and of the shipped configurations): a
// 64 x 64 tile, 16 bytes per lane on both sides -- a wave reads 4 rows x 256 bytes and writes 4 output rows x 256 bytes,
// non-temporal (each byte is touched once).  Tile rows are padded to 65 floats: the column reads of the second phase
// (rows 4 r4 + i of column c) land two lanes per bank.
__global__ void __launch_bounds__(256) transpose64_kernel(const float* in, float* out, int rows, int cols) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  __shared__ float tile[64][65];
  const size_t goff = (size_t)blockIdx.z * rows * cols;
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 64;  // tile origin: column, row of the input
  const int q = threadIdx.x & 15, p = threadIdx.x >> 4;  // 16 lanes x 16 bytes across, 16 lines down per pass
#pragma unroll
  for (int pass = 0; pass < 4; pass++) {
    const int y = y0 + p + 16 * pass, x = x0 + 4 * q;
    if (y < rows && x < cols) {
      const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(in + goff + (size_t)y * cols + x));
      float* t = &tile[p + 16 * pass][4 * q];
      t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
    }
  }
  __syncthreads();
#pragma unroll
  for (int pass = 0; pass < 4; pass++) {
    const int c = p + 16 * pass;           // input column = output row
    const int oy = x0 + c, ox = y0 + 4 * q;  // output row, first of four output columns (= input rows)
    if (oy < cols && ox < rows) {
      const f4v v = {tile[4 * q][c], tile[4 * q + 1][c], tile[4 * q + 2][c], tile[4 * q + 3][c]};
      __builtin_nontemporal_store(v, reinterpret_cast<f4v*>(out + goff + (size_t)oy * rows + ox));
    }
  }
}

// data_y as the reference holds it, CV_64F (main:987, 1125): split once into two f32 planes, x = hi + lo to 2^-48 of x.  The
// kernels that take f32 frames carry lo into the division by the background next to hi (FusedArgs::frames_lo), so that a
// frame of non-integer samples is not rounded at the size of the DC level (camera frames are integers: lo is 0 there).
__global__ void f64_split_kernel(const double* in, long long pitch_elems, float* hi, float* lo, int W, long long rows) {
  const long long n = rows * W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / W;
    const int c = (int)(i - r * W);
    const double x = in[r * pitch_elems + c];
    const float h = (float)x;
    hi[i] = h;
    const double l = x - (double)h;
    lo[i] = (l == l && h - h == 0.f) ? (float)l : 0.f;   // (inf / nan: no low word)
  }
}
