// Classification training tail for gfx950 (CDNA4): what torch autograd does behind the train-mode Classify head
// (ultralytics/nn/modules/head.py:1523-1529: linear(drop(pool(conv(x)).flatten(1))), raw logits) and v8ClassificationLoss
// (utils/loss.py:873-880: F.cross_entropy(preds, batch["cls"], reduction="mean")).
//
//   upa_global_avgpool_fwd      pooled[b, c] = (1 / HW) * sum_p x[b, p, c]                     (nn.AdaptiveAvgPool2d(1) + flatten)
//   upa_global_avgpool_bwd      dy[b, p, c] (+)= dpooled[b, c] / HW
//   upa_cross_entropy_fwd_bwd   loss = mean_r (logsumexp(z_r) - z_r[t_r]),  dz = (softmax(z) - onehot) * scale / rows
//   upa_linear_bwd              dW (+)= dy^T x,  db (+)= sum_m dy,  dx = dy W               (nn.Linear backward, plain (n, k) weight)
//
// These launches are small (bs 32 at 224 x 224: 160 KB of pooled rows, two 82 MFLOP products): every kernel is the plain form - one
// thread per output packet, a serial f32 chain over the reduced index - so that every sum has ONE fixed order that depends on nothing
// but the shapes.  No atomics anywhere: two calls, and a graph replay, are bit-identical.
//   * avgpool_fwd: a workgroup of 256 owns one image and 32 channel packets (16 bytes each on the vector path, one element on the scalar
//     path); its 8 pixel slices walk pixels s, s + 8, .. in order, meet in LDS and are added in slice order, then ONE divide by HW.
//     Any HW: the slices loop.
//   * cross_entropy: one workgroup of 256 per row, classes striped over it (any nc >= 1).  max, then sum of exp(z - max) (per thread
//     in class order, xor butterfly per wave, waves in order), then the gradient; the row loss goes to the workspace and a second
//     one-wave launch adds the rows (lane l: rows l, l + 64, ..; then the 64 lanes in order) and divides by rows.
//   * linear_bwd: explicit fmaf chains in index order (m for dW / db, n for dx), 4 consecutive k per thread: 16-byte packets of the
//     activation rows x / dx, element accesses of w / dw (views of the trainer's flat buffers, aligned to a float only).
#include "common.h"

#include <math.h>

namespace {

constexpr int POOL_SLICES = 8;   // pixel slices of an avgpool_fwd workgroup
constexpr int POOL_PACKETS = 32; // channel packets of an avgpool_fwd workgroup

template <typename T, int V> struct Packet;  // V elements of T <-> V floats
template <> struct Packet<float, 4> {
  __device__ static void load(const char* p, float* v) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  }
  __device__ static void store(char* p, const float* v) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
};
template <> struct Packet<float, 1> {
  __device__ static void load(const char* p, float* v) { v[0] = *reinterpret_cast<const float*>(p); }
  __device__ static void store(char* p, const float* v) { *reinterpret_cast<float*>(p) = v[0]; }
};
template <> struct Packet<bf16_t, 8> {
  __device__ static void load(const char* p, float* v) {
    const u32x4 t = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(t[i] << 16);
      v[2 * i + 1] = __uint_as_float(t[i] & 0xFFFF0000u);
    }
  }
  __device__ static void store(char* p, const float* v) {
    *reinterpret_cast<u32x4*>(p) = u32x4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
  }
};
template <> struct Packet<bf16_t, 1> {
  __device__ static void load(const char* p, float* v) { v[0] = bf16_to_f32(*reinterpret_cast<const bf16_t*>(p)); }
  __device__ static void store(char* p, const float* v) { *reinterpret_cast<bf16_t*>(p) = f32_to_bf16(v[0]); }
};

// grid (ceil(c / (32 V)), n), block 256 = 8 slices x 32 packets
template <typename T, int V>
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const char* __restrict__ x, int hw, int c, int ldx, float* __restrict__ pooled,
                                                          int ldp) {
  __shared__ float red[POOL_SLICES][POOL_PACKETS * V];
  const int pk = threadIdx.x % POOL_PACKETS, slice = threadIdx.x / POOL_PACKETS;
  const int ch = (blockIdx.x * POOL_PACKETS + pk) * V;
  const int img = blockIdx.y;
  float s[V];
#pragma unroll
  for (int e = 0; e < V; ++e) s[e] = 0.f;
  if (ch < c) {
    const char* base = x + ((size_t)img * hw * ldx + ch) * sizeof(T);
    for (int p = slice; p < hw; p += POOL_SLICES) {
      float v[V];
      Packet<T, V>::load(base + (size_t)p * ldx * sizeof(T), v);
#pragma unroll
      for (int e = 0; e < V; ++e) s[e] += v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) red[slice][pk * V + e] = s[e];
  __syncthreads();
  if (slice == 0 && ch < c) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float t = red[0][pk * V + e];
#pragma unroll
      for (int j = 1; j < POOL_SLICES; ++j) t += red[j][pk * V + e];
      pooled[(size_t)img * ldp + ch + e] = t / (float)hw;
    }
  }
}

// one thread per (pixel, channel packet): dy (+)= dpooled / HW, rounded to T once
template <typename T, int V>
__global__ void avgpool_bwd_kernel(const float* __restrict__ dpooled, int ldp, int n, int hw, int c, char* __restrict__ dy, int lddy,
                                   int accumulate) {
  const int cg = c / V;
  const long total = (long)n * hw * cg;
  const float fhw = (float)hw;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long px = idx / cg;
    const int g = (int)(idx - px * cg);
    const int img = (int)(px / hw);
    char* dst = dy + ((size_t)px * lddy + (size_t)g * V) * sizeof(T);
    const float* src = dpooled + (size_t)img * ldp + (size_t)g * V;
    float v[V], o[V];
    if (accumulate) Packet<T, V>::load(dst, o);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      v[e] = src[e] / fhw;
      if (accumulate) v[e] = o[e] + v[e];
    }
    Packet<T, V>::store(dst, v);
  }
}

// ---- cross-entropy ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_max(float v, float* red) {  // 256 threads; red: 4 floats
  for (int s = 32; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
  __syncthreads();  // earlier readers of red are done
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_sum(float v, float* red) {
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void cross_entropy_rows_kernel(const float* __restrict__ logits, int rows, int nc, int ldl,
                                                                 const int32_t* __restrict__ targets, const float* __restrict__ scale_dev,
                                                                 float* __restrict__ dlogits, int ldd, float* __restrict__ row_loss) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const float* z = logits + row * (size_t)ldl;
  float* dz = dlogits + row * (size_t)ldd;
  const int t = targets[row];
  const float scale = scale_dev ? *scale_dev : 1.0f;
  for (int i = nc + tid; i < ldd; i += 256) dz[i] = 0.0f;  // pad columns
  if (t < 0 || t >= nc) {  // a label outside the classes: nothing is indexed with it, the row is NaN so the mistake shows
    const float qnan = __uint_as_float(0x7FC00000u);
    for (int i = tid; i < nc; i += 256) dz[i] = qnan;
    if (tid == 0) row_loss[row] = qnan;
    return;
  }
  float m = -INFINITY;
  for (int i = tid; i < nc; i += 256) m = fmaxf(m, z[i]);
  m = block_max(m, red);
  float s = 0.0f;
  for (int i = tid; i < nc; i += 256) s += expf(z[i] - m);
  s = block_sum(s, red);
  const float frows = (float)rows;
  for (int i = tid; i < nc; i += 256) {
    const float p = expf(z[i] - m) / s;
    const float g = (p - (i == t ? 1.0f : 0.0f)) / frows;
    dz[i] = g * scale;
  }
  if (tid == 0) row_loss[row] = (m + logf(s)) - z[t];
}

__global__ __launch_bounds__(64) void cross_entropy_mean_kernel(const float* __restrict__ row_loss, int rows, float* __restrict__ loss) {
  __shared__ float part[64];
  float s = 0.0f;
  for (int r = threadIdx.x; r < rows; r += 64) s += row_loss[r];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = part[0];
    for (int l = 1; l < 64; ++l) t += part[l];
    *loss = t / (float)rows;
  }
}

// ---- nn.Linear backward ------------------------------------------------------------------------------------------------------------
// thread = (output n, 4 consecutive k): dW[n, k..k+3] (+)= sum_m dy[m, n] x[m, k..k+3]; the k = 0 thread of a row also owns db[n]
__global__ __launch_bounds__(256) void linear_wgrad_kernel(const float* __restrict__ x, int m, int k, int ldx, const float* __restrict__ dy,
                                                           int n, int lddy, float* __restrict__ dw, float* __restrict__ db, int accumulate) {
  const int k4 = k >> 2;
  const long total = (long)n * k4;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int row = (int)(idx / k4), kg = (int)(idx - (long)row * k4);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    for (int i = 0; i < m; ++i) {
      const float d = dy[(size_t)i * lddy + row];
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (size_t)i * ldx + kg * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(d, xv[e], acc[e]);
      bsum += d;
    }
    float* out = dw + (size_t)row * k + kg * 4;  // element stores: dw is a view of a flat gradient buffer at any float offset
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = accumulate ? out[e] + acc[e] : acc[e];
    if (kg == 0 && db) db[row] = accumulate ? db[row] + bsum : bsum;
  }
}

// thread = (row m, 4 consecutive k): dx[m, k..k+3] = sum_n dy[m, n] W[n, k..k+3]
__global__ __launch_bounds__(256) void linear_dgrad_kernel(const float* __restrict__ dy, int m, int n, int lddy, const float* __restrict__ w,
                                                           int k, float* __restrict__ dx, int lddx) {
  const int k4 = k >> 2;
  const long total = (long)m * k4;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int row = (int)(idx / k4), kg = (int)(idx - (long)row * k4);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* d = dy + (size_t)row * lddy;
    for (int j = 0; j < n; ++j) {
      const float dj = d[j];
      const float* wv = w + (size_t)j * k + kg * 4;  // element loads: w is a view of the flat parameter buffer at any float offset
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(dj, wv[e], acc[e]);
    }
    *reinterpret_cast<f32x4*>(dx + (size_t)row * lddx + kg * 4) = acc;
  }
}

int blocks_for(long total, int cap = 4096) {
  long g = (total + 255) / 256;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

int check_pool(const char* what, const void* a, const void* b, int n, int h, int w, int c, int ld, int ldp, int dtype) {
  UPA_CHECK_ARG(a && b, "%s: null pointer", what);
  UPA_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0, "%s: bad shape", what);
  UPA_CHECK_ARG(n <= 65535 && (long long)h * w <= (1 << 24), "%s: n > 65535 or h * w > 2^24", what);
  UPA_CHECK_ARG(ld >= c && ldp >= c, "%s: pixel stride < c or pooled stride < c", what);
  if (dtype != UPA_F32 && dtype != UPA_BF16) {
    upa_set_error("%s: dtype must be F32 | BF16", what);
    return UPA_EUNSUPPORTED;
  }
  return UPA_OK;
}

}  // namespace

extern "C" int upa_global_avgpool_fwd(const void* x, int n, int h, int w, int c, int ldx, float* pooled, int ldp, int dtype, void* stream) {
  if (int rc = check_pool("global_avgpool_fwd", x, pooled, n, h, w, c, ldx, ldp, dtype)) return rc;
  const int es = upa_elem_size(dtype), E = 16 / es;
  UPA_CHECK_ARG((uintptr_t)x % es == 0 && (uintptr_t)pooled % 4 == 0, "global_avgpool_fwd: misaligned pointer");
  const bool vec = c % E == 0 && ldx % E == 0 && (uintptr_t)x % 16 == 0;  // 16-byte packets where the pitch allows
  const int V = vec ? E : 1;
  const dim3 grid((unsigned)cdiv(c, POOL_PACKETS * V), (unsigned)n);
  const hipStream_t s = (hipStream_t)stream;
  const char* xp = (const char*)x;
  if (dtype == UPA_BF16) {
    if (vec) hipLaunchKernelGGL((avgpool_fwd_kernel<bf16_t, 8>), grid, dim3(256), 0, s, xp, h * w, c, ldx, pooled, ldp);
    else hipLaunchKernelGGL((avgpool_fwd_kernel<bf16_t, 1>), grid, dim3(256), 0, s, xp, h * w, c, ldx, pooled, ldp);
  } else {
    if (vec) hipLaunchKernelGGL((avgpool_fwd_kernel<float, 4>), grid, dim3(256), 0, s, xp, h * w, c, ldx, pooled, ldp);
    else hipLaunchKernelGGL((avgpool_fwd_kernel<float, 1>), grid, dim3(256), 0, s, xp, h * w, c, ldx, pooled, ldp);
  }
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_global_avgpool_bwd(const float* dpooled, int ldp, int n, int h, int w, int c, void* dy, int lddy, int accumulate,
                                      int dtype, void* stream) {
  if (int rc = check_pool("global_avgpool_bwd", dpooled, dy, n, h, w, c, lddy, ldp, dtype)) return rc;
  const int es = upa_elem_size(dtype), E = 16 / es;
  UPA_CHECK_ARG((uintptr_t)dy % es == 0 && (uintptr_t)dpooled % 4 == 0, "global_avgpool_bwd: misaligned pointer");
  const bool vec = c % E == 0 && lddy % E == 0 && (uintptr_t)dy % 16 == 0;
  const int V = vec ? E : 1;
  const long total = (long)n * h * w * (c / V);
  const dim3 grid((unsigned)blocks_for(total));
  const hipStream_t s = (hipStream_t)stream;
  char* yp = (char*)dy;
  const int acc = accumulate ? 1 : 0;
  if (dtype == UPA_BF16) {
    if (vec) hipLaunchKernelGGL((avgpool_bwd_kernel<bf16_t, 8>), grid, dim3(256), 0, s, dpooled, ldp, n, h * w, c, yp, lddy, acc);
    else hipLaunchKernelGGL((avgpool_bwd_kernel<bf16_t, 1>), grid, dim3(256), 0, s, dpooled, ldp, n, h * w, c, yp, lddy, acc);
  } else {
    if (vec) hipLaunchKernelGGL((avgpool_bwd_kernel<float, 4>), grid, dim3(256), 0, s, dpooled, ldp, n, h * w, c, yp, lddy, acc);
    else hipLaunchKernelGGL((avgpool_bwd_kernel<float, 1>), grid, dim3(256), 0, s, dpooled, ldp, n, h * w, c, yp, lddy, acc);
  }
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" size_t upa_cross_entropy_workspace_bytes(int rows) { return (size_t)(rows > 0 ? rows : 0) * sizeof(float); }

extern "C" int upa_cross_entropy_fwd_bwd(const float* logits, int rows, int nc, int ldl, const int32_t* targets, const float* loss_scale,
                                         float* loss, float* dlogits, int ldd, void* workspace, size_t workspace_bytes, void* stream) {
  UPA_CHECK_ARG(logits && targets && loss && dlogits && workspace, "cross_entropy_fwd_bwd: null pointer");
  UPA_CHECK_ARG(rows >= 1 && nc >= 1, "cross_entropy_fwd_bwd: rows < 1 or nc < 1 (rows = %d, nc = %d)", rows, nc);
  UPA_CHECK_ARG(ldl >= nc && ldd >= nc, "cross_entropy_fwd_bwd: ldl < nc or ldd < nc");
  UPA_CHECK_ARG(workspace_bytes >= upa_cross_entropy_workspace_bytes(rows), "cross_entropy_fwd_bwd: workspace of %zu bytes, needs %zu",
                workspace_bytes, upa_cross_entropy_workspace_bytes(rows));
  UPA_CHECK_ARG((uintptr_t)logits % 4 == 0 && (uintptr_t)dlogits % 4 == 0 && (uintptr_t)targets % 4 == 0 && (uintptr_t)workspace % 4 == 0 &&
                    (uintptr_t)loss % 4 == 0 && (!loss_scale || (uintptr_t)loss_scale % 4 == 0),
                "cross_entropy_fwd_bwd: misaligned pointer");
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cross_entropy_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, logits, rows, nc, ldl, targets, loss_scale, dlogits,
                     ldd, (float*)workspace);
  hipLaunchKernelGGL(cross_entropy_mean_kernel, dim3(1), dim3(64), 0, s, (const float*)workspace, rows, loss);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_linear_bwd(const float* x, int m, int k, int ldx, const float* dy, int n, int lddy, const float* w, float* dw, float* db,
                              float* dx, int lddx, int accumulate, void* stream) {
  UPA_CHECK_ARG(x && dy && w && dw, "linear_bwd: null pointer");
  UPA_CHECK_ARG(m >= 1 && k >= 1 && n >= 1, "linear_bwd: bad shape (m = %d, k = %d, n = %d)", m, k, n);
  UPA_CHECK_ARG(ldx >= k && lddy >= n && (!dx || lddx >= k), "linear_bwd: ldx < k, lddy < n or lddx < k");
  if (k % 4 != 0 || ldx % 4 != 0 || (dx && lddx % 4 != 0)) {
    upa_set_error("linear_bwd: k, ldx and lddx must be multiples of 4 (16-byte rows; k = %d, ldx = %d, lddx = %d)", k, ldx, dx ? lddx : 0);
    return UPA_EUNSUPPORTED;
  }
  UPA_CHECK_ARG((uintptr_t)x % 16 == 0 && (!dx || (uintptr_t)dx % 16 == 0) && (uintptr_t)w % 4 == 0 && (uintptr_t)dw % 4 == 0 &&
                    (uintptr_t)dy % 4 == 0 && (!db || (uintptr_t)db % 4 == 0),
                "linear_bwd: x and dx must be 16-byte aligned, the other pointers 4-byte aligned");
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(linear_wgrad_kernel, dim3((unsigned)blocks_for((long)n * (k / 4))), dim3(256), 0, s, x, m, k, ldx, dy, n, lddy, dw, db,
                     accumulate ? 1 : 0);
  if (dx)
    hipLaunchKernelGGL(linear_dgrad_kernel, dim3((unsigned)blocks_for((long)m * (k / 4))), dim3(256), 0, s, dy, m, n, lddy, w, k, dx, lddx);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}
