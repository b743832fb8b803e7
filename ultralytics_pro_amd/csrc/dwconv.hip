// Depthwise 3x3 convolution: DWConv (ultralytics/nn/modules/conv.py:411-425, Conv with groups = gcd(c1, c2) = C) with its BatchNorm
// folded on the host, y = act(sum_taps w[tap][c] * x[pixel + tap][c] + b[c]).  YOLO11 uses it in the non-legacy Detect class branch
// (nn/modules/head.py:98-110) and as `pe` of v10_Attention (block.py:1709); the `pe` form is fused into csrc/psa.hip.
//
// 9 MACs per output element: the kernel is bound by the activation bytes.  A thread owns V consecutive channels (one 16-byte
// vector: 8 bf16 or 4 f32) of one output pixel; consecutive threads take consecutive channel groups, then consecutive pixels, so a
// wave reads whole pixel rows and the x +- 1 neighbours of one thread are its neighbours' centre reads: the 3x3 neighbourhood is
// served from L1 / L2, HBM sees each input row about once per output row.  Channel counts that are not a multiple of V (or
// misaligned views) run the same code with V = 1.
#include "bn_math.h"
#include "common.h"

namespace {

template <typename T, int V>
__device__ __forceinline__ void load_v(const T* p, float (&o)[V]) {
  if constexpr (V == 1) {
    o[0] = ElemTraits<T>::load(p);
  } else if constexpr (sizeof(T) == 4) {
    static_assert(V == 4, "f32 vectors are 4 wide");
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = v[j];
  } else {
    static_assert(V == 8, "bf16 vectors are 8 wide");
    const u32x4 v = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[2 * j] = __uint_as_float(v[j] << 16);
      o[2 * j + 1] = __uint_as_float(v[j] & 0xffff0000u);
    }
  }
}

template <typename T, int V>
__device__ __forceinline__ void store_v(T* p, const float (&o)[V]) {
  if constexpr (V == 1) {
    if constexpr (sizeof(T) == 4) *p = o[0];
    else *p = f32_to_bf16(o[0]);
  } else if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<f32x4*>(p) = f32x4{o[0], o[1], o[2], o[3]};
  } else {
    *reinterpret_cast<u32x4*>(p) = u32x4{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
  }
}

template <int V>
__device__ __forceinline__ void load_w(const float* p, float (&o)[V]) {
  if constexpr (V == 1) {
    o[0] = *p;
  } else {
#pragma unroll
    for (int j = 0; j < V; j += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + j);
      o[j] = v[0], o[j + 1] = v[1], o[j + 2] = v[2], o[j + 3] = v[3];
    }
  }
}

}  // namespace

// wt: (9, c) f32, tap-major (tap = ky * 3 + kx), so a thread's V weights of one tap are one or two 16-byte loads.
// Grid: x over the (pixel, channel group) items of one output row, y over the n * oh output rows (32-bit indexing throughout).
template <typename T, int V, int S>
__global__ __launch_bounds__(256) void dwconv3_kernel(const T* __restrict__ x, int n, int h, int w, int c, int ldx, const float* __restrict__ wt,
                                                      const float* __restrict__ bias, T* __restrict__ y, int oh, int ow, int ldy, int act) {
  const int cg = c / V, per_row = ow * cg;
  for (int row = blockIdx.y; row < n * oh; row += gridDim.y) {
    const int b = row / oh, oy = row - b * oh;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < per_row; i += gridDim.x * 256) {
      const int ox = i / cg, c0 = (i - ox * cg) * V;
      float acc[V];
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * S - 1 + ky;
        if (iy < 0 || iy >= h) continue;
        const T* xr = x + ((size_t)b * h + iy) * w * (size_t)ldx + c0;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = ox * S - 1 + kx;
          if (ix < 0 || ix >= w) continue;
          float xv[V], wv[V];
          load_v<T, V>(xr + (size_t)ix * ldx, xv);
          load_w<V>(wt + (ky * 3 + kx) * c + c0, wv);
#pragma unroll
          for (int j = 0; j < V; ++j) acc[j] = fmaf(xv[j], wv[j], acc[j]);
        }
      }
      float bv[V];
      load_w<V>(bias + c0, bv);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = apply_act(acc[j] + bv[j], act);
      store_v<T, V>(y + (((size_t)b * oh + oy) * ow + ox) * (size_t)ldy + c0, acc);
    }
  }
}

template <typename T, int V>
static int launch_dwconv3(const void* x, int n, int h, int w, int c, int ldx, const float* wt, const float* bias, void* y, int ldy, int stride,
                          int act, hipStream_t s) {
  const int oh = (h + 2 - 3) / stride + 1, ow = (w + 2 - 3) / stride + 1;
  const long long per_row = (long long)ow * (c / V), rows = (long long)n * oh;
  if (per_row > 0x7fffffffll || rows > 0x7fffffffll) {
    upa_set_error("dwconv2d: %lld rows x %lld items", rows, per_row);
    return UPA_EUNSUPPORTED;
  }
  const dim3 grid((unsigned)((per_row + 255) / 256 < 4096 ? (per_row + 255) / 256 : 4096), (unsigned)(rows < 65535 ? rows : 65535));
  if (stride == 1)
    hipLaunchKernelGGL((dwconv3_kernel<T, V, 1>), grid, dim3(256), 0, s, (const T*)x, n, h, w, c, ldx, wt, bias, (T*)y, oh, ow, ldy, act);
  else
    hipLaunchKernelGGL((dwconv3_kernel<T, V, 2>), grid, dim3(256), 0, s, (const T*)x, n, h, w, c, ldx, wt, bias, (T*)y, oh, ow, ldy, act);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_dwconv2d(const void* x, int n, int h, int w, int c, int ldx, const float* weight, const float* bias, void* y, int ldy,
                            int k, int stride, int pad, int act, int dtype, void* stream) {
  UPA_CHECK_ARG(x && weight && bias && y, "dwconv2d: null pointer");
  UPA_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0 && ldx >= c && ldy >= c, "dwconv2d: bad shape n=%d h=%d w=%d c=%d ldx=%d ldy=%d", n, h, w,
                c, ldx, ldy);
  if (k != 3 || pad != 1 || (stride != 1 && stride != 2) || (act != UPA_ACT_NONE && act != UPA_ACT_SILU) ||
      (dtype != UPA_F32 && dtype != UPA_BF16)) {
    upa_set_error("dwconv2d: k=%d stride=%d pad=%d act=%d dtype=%d outside the supported form (k 3, pad 1, stride 1|2, act none|SiLU, "
                  "f32|bf16)", k, stride, pad, act, dtype);
    return UPA_EUNSUPPORTED;
  }
  const int es = upa_elem_size(dtype);
  const int oh = (h + 2 - 3) / stride + 1, ow = (w + 2 - 3) / stride + 1;
  {  // the output must not overlap the input: a thread's neighbours read pixels other threads write
    const char *xa = (const char*)x, *ya = (const char*)y;
    const size_t xb = (((size_t)n * h * w - 1) * ldx + c) * es, yb = (((size_t)n * oh * ow - 1) * ldy + c) * es;
    UPA_CHECK_ARG(xa + xb <= ya || ya + yb <= xa, "dwconv2d: output view overlaps the input");
  }
  hipStream_t s = (hipStream_t)stream;
  const int V = 16 / es;
  const bool vec = c % V == 0 && ldx % V == 0 && ldy % V == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0 &&
                   ((uintptr_t)weight % 16) == 0 && ((uintptr_t)bias % 16) == 0;
  if (dtype == UPA_BF16)
    return vec ? launch_dwconv3<bf16_t, 8>(x, n, h, w, c, ldx, weight, bias, y, ldy, stride, act, s)
               : launch_dwconv3<bf16_t, 1>(x, n, h, w, c, ldx, weight, bias, y, ldy, stride, act, s);
  return vec ? launch_dwconv3<float, 4>(x, n, h, w, c, ldx, weight, bias, y, ldy, stride, act, s)
             : launch_dwconv3<float, 1>(x, n, h, w, c, ldx, weight, bias, y, ldy, stride, act, s);
}

// ---- training forms (stride 1, pad 1, no bias, no activation; BatchNorm runs on batch statistics through upa_bn_stats / upa_bn_act_fwd) -----
// The weight and its gradient are f32 in the module's own layout (C, 1, 3, 3): w[c * 9 + kh * 3 + kw].  A thread owns one 16-byte channel
// vector of one pixel, as above; its 9 V weights are scalar loads (stride 9 floats), read once per thread.
//   forward  z[p][c]   = sum_taps w[c][kh][kw] x[p + (kh - 1, kw - 1)][c]
//   dx       dx[p][c] (+)= sum_taps w[c][kh][kw] dz[p - (kh - 1, kw - 1)][c]            (the correlation with the flipped taps)
//   dw       dw[c][kh][kw] (+)= sum_p dz[p][c] x[p + (kh - 1, kw - 1)][c]: every thread keeps 9 V f32 partial sums over its pixels (pixel
//            p of a workgroup's slice goes to thread row p % PB), the PB thread rows of a workgroup are added in row order through LDS,
//            the workgroups' partials (ws: [workgroup][c][9] f32) are added in workgroup order by a second launch - one order, fixed by
//            (n, h, w, c), no atomics.
// All sums are f32 fmaf chains in both storage modes; the only rounding to bf16 is at the store of z / dx.
constexpr int DWT_MAX_WG = 128;  // workgroups (partials per channel) of the weight-gradient pass

// FLIP = false: z = dwconv(x); FLIP = true: the data gradient (src = dz).  ACC: dst += (read in the storage type, added in f32).
template <typename T, int V, bool FLIP, bool ACC>
__global__ __launch_bounds__(256) void dwconv3_train_kernel(const T* __restrict__ src, int n, int h, int w, int c, int lds_, const float* __restrict__ wt,
                                                            T* __restrict__ dst, int ldd) {
  const int cg = c / V, per_row = w * cg;
  for (int row = blockIdx.y; row < n * h; row += gridDim.y) {
    const int b = row / h, oy = row - b * h;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < per_row; i += gridDim.x * 256) {
      const int ox = i / cg, c0 = (i - ox * cg) * V;
      float acc[V];
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy - 1 + ky;
        if (iy < 0 || iy >= h) continue;
        const T* xr = src + ((size_t)b * h + iy) * w * (size_t)lds_ + c0;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = ox - 1 + kx;
          if (ix < 0 || ix >= w) continue;
          const int tap = FLIP ? (2 - ky) * 3 + (2 - kx) : ky * 3 + kx;
          float xv[V];
          load_v<T, V>(xr + (size_t)ix * lds_, xv);
#pragma unroll
          for (int j = 0; j < V; ++j) acc[j] = fmaf(xv[j], wt[(size_t)(c0 + j) * 9 + tap], acc[j]);
        }
      }
      T* dp = dst + (((size_t)b * h + oy) * w + ox) * (size_t)ldd + c0;
      if constexpr (ACC) {
        float old[V];
        load_v<T, V>(dp, old);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += old[j];
      }
      store_v<T, V>(dp, acc);
    }
  }
}

// Weight-gradient partials.  Grid (workgroups over pixels, chunks of 256 channel groups); thread (pl, g): channel group g of the chunk,
// pixels pl, pl + PB, ... of the workgroup's contiguous pixel slice [bx * per, bx * per + per).
template <typename T, int V>
__global__ __launch_bounds__(256) void dwconv3_wgrad_partial_kernel(const T* __restrict__ x, const T* __restrict__ dz, int n, int h, int w, int c,
                                                                    int ldx, int lddz, float* __restrict__ ws, long long per) {
  __shared__ float red[256 * V];
  const int cg = c / V;
  const int g0 = blockIdx.y * 256, cgl = min(256, cg - g0), PB = 256 / cgl;
  const int tid = threadIdx.x, pl = tid / cgl, g = tid - pl * cgl;
  const bool active = pl < PB;
  const int c0 = (g0 + g) * V;
  const long long NP = (long long)n * h * w;
  const long long p0 = (long long)blockIdx.x * per, p1 = p0 + per < NP ? p0 + per : NP;
  float acc[9][V];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[t][j] = 0.f;
  if (active) {
    for (long long p = p0 + pl; p < p1; p += PB) {
      const long long row = p / w;
      const int ox = (int)(p - row * w), oy = (int)(row % h);
      float g_[V];
      load_v<T, V>(dz + (size_t)p * lddz + c0, g_);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy - 1 + ky;
        if (iy < 0 || iy >= h) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = ox - 1 + kx;
          if (ix < 0 || ix >= w) continue;
          float xv[V];
          load_v<T, V>(x + (size_t)(p + (long long)(ky - 1) * w + (kx - 1)) * ldx + c0, xv);
#pragma unroll
          for (int j = 0; j < V; ++j) acc[ky * 3 + kx][j] = fmaf(g_[j], xv[j], acc[ky * 3 + kx][j]);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < V; ++j) red[tid * V + j] = acc[t][j];
    __syncthreads();
    if (pl == 0) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float a = acc[t][j];
        for (int q = 1; q < PB; ++q) a += red[(q * cgl + g) * V + j];
        ws[((size_t)blockIdx.x * c + c0 + j) * 9 + t] = a;
      }
    }
  }
}

__global__ __launch_bounds__(256) void dwconv3_wgrad_combine_kernel(const float* __restrict__ ws, int nwg, int c9, float* __restrict__ dw, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= c9) return;
  float a = 0.f;
  for (int b = 0; b < nwg; ++b) a += ws[(size_t)b * c9 + i];
  dw[i] = accumulate ? dw[i] + a : a;
}

static int dwt_check(const char* what, int n, int h, int w, int c, int dtype) {
  if (!(n > 0 && h > 0 && w > 0 && c > 0)) {
    upa_set_error("%s: bad shape n=%d h=%d w=%d c=%d", what, n, h, w, c);
    return UPA_EINVAL;
  }
  if (dtype != UPA_F32 && dtype != UPA_BF16) {
    upa_set_error("%s: dtype %d", what, dtype);
    return UPA_EUNSUPPORTED;
  }
  const int V = 16 / upa_elem_size(dtype);
  if (c % V != 0) {
    upa_set_error("%s: c = %d is not a multiple of the 16-byte vector (%d)", what, c, V);
    return UPA_EINVAL;
  }
  if ((long long)w * (c / V) > 0x7fffffffll || (long long)n * h > 0x7fffffffll || c > 0x7fffffff / 9) {
    upa_set_error("%s: shape too large", what);
    return UPA_EUNSUPPORTED;
  }
  return UPA_OK;
}

static bool dwt_view_ok(const void* p, int ld, int c, int V) { return ld >= c && ld % V == 0 && ((uintptr_t)p % 16) == 0; }
static size_t dwt_view_bytes(int n, int h, int w, int c, int ld, int es) { return (((size_t)n * h * w - 1) * ld + c) * es; }
static bool dwt_overlap(const void* a, size_t ab, const void* b, size_t bb) {
  const char *x = (const char*)a, *y = (const char*)b;
  return !(x + ab <= y || y + bb <= x);
}

template <typename T, int V, bool FLIP>
static int launch_dwt(const void* src, int n, int h, int w, int c, int lds_, const float* wt, void* dst, int ldd, int acc, hipStream_t s) {
  const long long per_row = (long long)w * (c / V), rows = (long long)n * h;
  const dim3 grid((unsigned)((per_row + 255) / 256 < 4096 ? (per_row + 255) / 256 : 4096), (unsigned)(rows < 65535 ? rows : 65535));
  if (acc)
    hipLaunchKernelGGL((dwconv3_train_kernel<T, V, FLIP, true>), grid, dim3(256), 0, s, (const T*)src, n, h, w, c, lds_, wt, (T*)dst, ldd);
  else
    hipLaunchKernelGGL((dwconv3_train_kernel<T, V, FLIP, false>), grid, dim3(256), 0, s, (const T*)src, n, h, w, c, lds_, wt, (T*)dst, ldd);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_dwconv2d_train_fwd(const void* x, int n, int h, int w, int c, int ldx, const float* w_c133, void* z, int ldz, int dtype,
                                      void* stream) {
  UPA_CHECK_ARG(x && w_c133 && z, "dwconv2d_train_fwd: null pointer");
  const int rc = dwt_check("dwconv2d_train_fwd", n, h, w, c, dtype);
  if (rc != UPA_OK) return rc;
  const int es = upa_elem_size(dtype), V = 16 / es;
  UPA_CHECK_ARG(dwt_view_ok(x, ldx, c, V) && dwt_view_ok(z, ldz, c, V), "dwconv2d_train_fwd: views need ld >= c, ld %% %d == 0 and 16-byte alignment", V);
  UPA_CHECK_ARG(!dwt_overlap(x, dwt_view_bytes(n, h, w, c, ldx, es), z, dwt_view_bytes(n, h, w, c, ldz, es)),
                "dwconv2d_train_fwd: output view overlaps the input");
  hipStream_t s = (hipStream_t)stream;
  return dtype == UPA_BF16 ? launch_dwt<bf16_t, 8, false>(x, n, h, w, c, ldx, w_c133, z, ldz, 0, s)
                           : launch_dwt<float, 4, false>(x, n, h, w, c, ldx, w_c133, z, ldz, 0, s);
}

extern "C" size_t upa_dwconv2d_bwd_workspace_bytes(int c) { return c > 0 ? (size_t)DWT_MAX_WG * c * 9 * sizeof(float) : 0; }

extern "C" int upa_dwconv2d_bwd(const void* x, const void* dz, int n, int h, int w, int c, int ldx, int lddz, const float* w_c133, void* dx, int lddx,
                                int accumulate_dx, float* dw_c133, int accumulate_dw, void* ws, size_t ws_bytes, int dtype, void* stream) {
  UPA_CHECK_ARG(dz && (dx || dw_c133), "dwconv2d_bwd: null pointer");
  UPA_CHECK_ARG(!dx || w_c133, "dwconv2d_bwd: dx needs the weight");
  UPA_CHECK_ARG(!dw_c133 || (x && ws), "dwconv2d_bwd: dw needs x and a workspace");
  const int rc = dwt_check("dwconv2d_bwd", n, h, w, c, dtype);
  if (rc != UPA_OK) return rc;
  const int es = upa_elem_size(dtype), V = 16 / es;
  UPA_CHECK_ARG(dwt_view_ok(dz, lddz, c, V) && (!dx || dwt_view_ok(dx, lddx, c, V)) && (!dw_c133 || dwt_view_ok(x, ldx, c, V)),
                "dwconv2d_bwd: views need ld >= c, ld %% %d == 0 and 16-byte alignment", V);
  UPA_CHECK_ARG(!dw_c133 || ws_bytes >= upa_dwconv2d_bwd_workspace_bytes(c), "dwconv2d_bwd: workspace of %zu bytes, %zu needed", ws_bytes,
                upa_dwconv2d_bwd_workspace_bytes(c));
  UPA_CHECK_ARG(!dx || !dwt_overlap(dz, dwt_view_bytes(n, h, w, c, lddz, es), dx, dwt_view_bytes(n, h, w, c, lddx, es)),
                "dwconv2d_bwd: dx overlaps dz");
  hipStream_t s = (hipStream_t)stream;
  if (dw_c133) {  // first: reads x, which dx may share a buffer with (another channel slice)
    const long long NP = (long long)n * h * w;
    const int cg = c / V, chunks = cdiv(cg, 256);
    const int PBmin = 256 / (cg < 256 ? cg : 256);
    long long nwg = (NP + PBmin - 1) / PBmin;
    if (nwg > DWT_MAX_WG) nwg = DWT_MAX_WG;
    const long long per = (NP + nwg - 1) / nwg;
    nwg = (NP + per - 1) / per;  // no empty workgroup: every partial row the combine reads is written
    const dim3 grid((unsigned)nwg, (unsigned)chunks);
    if (dtype == UPA_BF16)
      hipLaunchKernelGGL((dwconv3_wgrad_partial_kernel<bf16_t, 8>), grid, dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)dz, n, h, w, c, ldx, lddz,
                         (float*)ws, per);
    else
      hipLaunchKernelGGL((dwconv3_wgrad_partial_kernel<float, 4>), grid, dim3(256), 0, s, (const float*)x, (const float*)dz, n, h, w, c, ldx, lddz,
                         (float*)ws, per);
    UPA_LAUNCH_CHECK();
    hipLaunchKernelGGL(dwconv3_wgrad_combine_kernel, dim3((unsigned)cdiv(c * 9, 256)), dim3(256), 0, s, (const float*)ws, (int)nwg, c * 9, dw_c133,
                       accumulate_dw);
    UPA_LAUNCH_CHECK();
  }
  if (dx) {
    return dtype == UPA_BF16 ? launch_dwt<bf16_t, 8, true>(dz, n, h, w, c, lddz, w_c133, dx, lddx, accumulate_dx, s)
                             : launch_dwt<float, 4, true>(dz, n, h, w, c, lddz, w_c133, dx, lddx, accumulate_dx, s);
  }
  return UPA_OK;
}

// ---- DWConv = depthwise 3x3 + BatchNorm(batch statistics) + SiLU | none, fused for training (conv.py:411-425 in train mode; the class
// branch of the non-legacy Detect head, head.py:98-110) -------------------------------------------------------------------------------
// Both kernels tile a map the same way.  A workgroup owns one image, one band of DWB_R rows and one chunk of channel vectors, and walks
// the band in tiles of DWB_T columns.  Per tile it stages the (DWB_R + 2) x (DWB_T + 2) halo window in LDS once - zeros outside the
// image - so every input element leaves HBM / L2 once per band it touches (1.25 x for the rows shared by two bands) instead of nine
// times, and the nine taps are LDS reads.  Thread (slot, g): channel vector g of the chunk, pixels slot, slot + slots, ... of the window;
// its 9 V weights stay in registers.  Everything a workgroup sums over pixels (the statistics, the weight gradient) is kept per thread
// in f32, added over the slots in slot order through LDS, and leaves as ONE partial row per workgroup; a second launch adds the rows in
// workgroup order.  The number of workgroups is n * ceil(h / DWB_R) * chunks: sized by the shape alone.
//   LDS, forward:  180 window pixels x <= 16 vectors x 16 B                                  = 46080 B
//   LDS, backward: 180 x <= 40 channels x (4 B dz in f32 + 4 | 2 B x)                        = 57600 B (f32), 43200 B (bf16)
// A thread's 16-byte vector is one ds_read_b128 / ds_write_b128; consecutive threads of a slot take consecutive vectors.
constexpr int DWB_T = 16, DWB_R = 8, DWB_WP = DWB_T + 2, DWB_HP = (DWB_R + 2) * DWB_WP;
constexpr int DWB_FWD_CG = 16;  // channel vectors per workgroup, forward
constexpr int DWB_BWD_CH = 40;  // channels per workgroup, backward (dz is kept in f32)

namespace {

template <typename T, int V>
__device__ __forceinline__ void unpack_v(const u32x4& v, float (&o)[V]) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = __uint_as_float(v[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[2 * j] = __uint_as_float(v[j] << 16);
      o[2 * j + 1] = __uint_as_float(v[j] & 0xffff0000u);
    }
  }
}

// the value a store of `a` leaves in memory
template <typename T>
__device__ __forceinline__ float stored(float a) {
  if constexpr (sizeof(T) == 4) return a;
  else return bf16_to_f32(f32_to_bf16(a));
}

}  // namespace

// z = dwconv(x), the same fmaf chain as dwconv3_train_kernel (tap order ky, kx; a tap outside the image adds fmaf(0, w, acc) = acc),
// and rows[workgroup][2][c] = the sums and sums of squares of the values it stored.
template <typename T, int V>
__global__ __launch_bounds__(256) void dwconv3_bn_fwd_kernel(const T* __restrict__ x, int h, int w, int c, int ldx, const float* __restrict__ wt,
                                                             T* __restrict__ z, int ldz, float* __restrict__ rows, int CC, int bands) {
  extern __shared__ __attribute__((aligned(16))) char dwb_sm[];
  u32x4* tile = reinterpret_cast<u32x4*>(dwb_sm);
  const int cg = c / V;
  const int g0 = blockIdx.y * CC, cgl = min(CC, cg - g0), slots = 256 / cgl;
  const int tid = threadIdx.x, slot = tid / cgl, g = tid - slot * cgl;
  const bool active = slot < slots;
  const int c0 = (g0 + g) * V;
  const int b = blockIdx.x / bands, y0 = (blockIdx.x - b * bands) * DWB_R;
  float wv[9][V], s0[V], s1[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s0[j] = s1[j] = 0.f;
  if (active) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int j = 0; j < V; ++j) wv[t][j] = wt[(size_t)(c0 + j) * 9 + t];
  }
  for (int x0 = 0; x0 < w; x0 += DWB_T) {
    __syncthreads();  // the previous tile's reads are done
    if (active) {
      for (int hp = slot; hp < DWB_HP; hp += slots) {
        const int hy = hp / DWB_WP, hx = hp - hy * DWB_WP;
        const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (iy >= 0 && iy < h && ix >= 0 && ix < w) v = *reinterpret_cast<const u32x4*>(x + (((size_t)b * h + iy) * w + ix) * (size_t)ldx + c0);
        tile[hp * cgl + g] = v;
      }
    }
    __syncthreads();
    if (active) {
      for (int ip = slot; ip < DWB_R * DWB_T; ip += slots) {
        const int ty = ip / DWB_T, tx = ip - ty * DWB_T;
        const int oy = y0 + ty, ox = x0 + tx;
        if (oy >= h || ox >= w) continue;
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            float xv[V];
            unpack_v<T, V>(tile[((ty + ky) * DWB_WP + tx + kx) * cgl + g], xv);
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = fmaf(xv[j], wv[ky * 3 + kx][j], acc[j]);
          }
        store_v<T, V>(z + (((size_t)b * h + oy) * w + ox) * (size_t)ldz + c0, acc);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float r = stored<T>(acc[j]);
          s0[j] += r;
          s1[j] = fmaf(r, r, s1[j]);
        }
      }
    }
  }
  __syncthreads();
  float* red = reinterpret_cast<float*>(dwb_sm);  // [slot][g][2][V]
  if (active) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      red[((slot * cgl + g) * 2) * V + j] = s0[j];
      red[((slot * cgl + g) * 2 + 1) * V + j] = s1[j];
    }
  }
  __syncthreads();
  if (slot == 0) {
    float* row = rows + (size_t)blockIdx.x * 2 * c;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float a0 = s0[j], a1 = s1[j];
      for (int q = 1; q < slots; ++q) {
        a0 += red[((q * cgl + g) * 2) * V + j];
        a1 += red[((q * cgl + g) * 2 + 1) * V + j];
      }
      row[c0 + j] = a0;
      row[c + c0 + j] = a1;
    }
  }
}

struct DwBwdParams {
  const void* x; const void* z; const void* dy; void* dx;
  int h, w, c, ldx, ldz, lddy, lddx;
  const float* wt; const float* mean; const float* var; const float* gamma; const float* beta;
  const double* s0; const double* s1;  // sum(du), sum(du * xhat) of upa_bn_bwd_sums
  float eps, inv; int act, accumulate_dx;
  float* ws;  // [workgroup][c][9] weight-gradient partials
  int CC, bands;
};

// dz = gamma rstd (du - (s0 + xhat s1) / npix), du = dy act'(gamma xhat + beta) - the expression of bn_apply_kernel (train.hip) - formed
// for the whole halo window in LDS and kept in f32; dx (+)= the correlation of dz with the flipped taps (tap order of
// dwconv3_train_kernel<FLIP>), dw partials = sum over the tile's own pixels of dz * shifted x (tap order of dwconv3_wgrad_partial_kernel).
template <typename T, int V>
__global__ __launch_bounds__(256) void dwconv3_bn_bwd_kernel(const DwBwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char dwb_sm[];
  const int c = p.c, h = p.h, w = p.w;
  const int cg = c / V;
  const int g0 = blockIdx.y * p.CC, cgl = min(p.CC, cg - g0), slots = 256 / cgl;
  const int tid = threadIdx.x, slot = tid / cgl, g = tid - slot * cgl;
  const bool active = slot < slots;
  const int c0 = (g0 + g) * V;
  const int b = blockIdx.x / p.bands, y0 = (blockIdx.x - b * p.bands) * DWB_R;
  float* dzs = reinterpret_cast<float*>(dwb_sm);                                              // [window pixel][cgl][V] f32
  const int dz_bytes = max(DWB_HP * cgl * V * 4, 256 * V * 4);                                // (the reduction below reuses it)
  u32x4* xs = reinterpret_cast<u32x4*>(dwb_sm + dz_bytes);                                    // [window pixel][cgl] 16 B
  const T* x = (const T*)p.x; const T* z = (const T*)p.z; const T* dy = (const T*)p.dy; T* dx = (T*)p.dx;
  float wv[9][V], acc[9][V], mean[V], rstd[V], gam[V], bet[V], k0[V], k1[V];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[t][j] = 0.f;
  if (active) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int ch = c0 + j;
      mean[j] = p.mean[ch]; rstd[j] = 1.0f / sqrtf(p.var[ch] + p.eps); gam[j] = p.gamma[ch]; bet[j] = p.beta[ch];
      k0[j] = (float)p.s0[ch]; k1[j] = (float)p.s1[ch];
#pragma unroll
      for (int t = 0; t < 9; ++t) wv[t][j] = p.wt[(size_t)ch * 9 + t];
    }
  }
  const bool silu = p.act == UPA_ACT_SILU;
  for (int x0 = 0; x0 < w; x0 += DWB_T) {
    __syncthreads();
    if (active) {
      for (int hp = slot; hp < DWB_HP; hp += slots) {
        const int hy = hp / DWB_WP, hx = hp - hy * DWB_WP;
        const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
        u32x4 xr = {0u, 0u, 0u, 0u};
        float d[V];
#pragma unroll
        for (int j = 0; j < V; ++j) d[j] = 0.f;
        if (iy >= 0 && iy < h && ix >= 0 && ix < w) {
          const size_t px = ((size_t)b * h + iy) * w + ix;
          xr = *reinterpret_cast<const u32x4*>(x + px * (size_t)p.ldx + c0);
          float zv[V], gv[V];
          load_v<T, V>(z + px * (size_t)p.ldz + c0, zv);
          load_v<T, V>(dy + px * (size_t)p.lddy + c0, gv);
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float xh = (zv[j] - mean[j]) * rstd[j];
            float du = gv[j];
            if (silu) du *= silu_grad<sizeof(T) == 2>(gam[j] * xh + bet[j]);
            d[j] = gam[j] * rstd[j] * (du - (k0[j] + xh * k1[j]) * p.inv);
          }
        }
        xs[hp * cgl + g] = xr;
#pragma unroll
        for (int j = 0; j < V; j += 4) *reinterpret_cast<f32x4*>(dzs + (size_t)(hp * cgl + g) * V + j) = f32x4{d[j], d[j + 1], d[j + 2], d[j + 3]};
      }
    }
    __syncthreads();
    if (active) {
      for (int ip = slot; ip < DWB_R * DWB_T; ip += slots) {
        const int ty = ip / DWB_T, tx = ip - ty * DWB_T;
        const int oy = y0 + ty, ox = x0 + tx;
        if (oy >= h || ox >= w) continue;
        float gz[V], a[V];
        load_w<V>(dzs + (size_t)(((ty + 1) * DWB_WP + tx + 1) * cgl + g) * V, gz);
#pragma unroll
        for (int j = 0; j < V; ++j) a[j] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int q = ((ty + ky) * DWB_WP + tx + kx) * cgl + g;
            float dn[V], xn[V];
            load_w<V>(dzs + (size_t)q * V, dn);
            unpack_v<T, V>(xs[q], xn);
#pragma unroll
            for (int j = 0; j < V; ++j) {
              a[j] = fmaf(dn[j], wv[8 - (ky * 3 + kx)][j], a[j]);
              acc[ky * 3 + kx][j] = fmaf(gz[j], xn[j], acc[ky * 3 + kx][j]);
            }
          }
        if (dx) {
          T* dp = dx + (((size_t)b * h + oy) * w + ox) * (size_t)p.lddx + c0;
          if (p.accumulate_dx) {
            float old[V];
            load_v<T, V>(dp, old);
#pragma unroll
            for (int j = 0; j < V; ++j) a[j] += old[j];
          }
          store_v<T, V>(dp, a);
        }
      }
    }
  }
  float* red = dzs;  // [thread][V]
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    __syncthreads();
    if (active) {
#pragma unroll
      for (int j = 0; j < V; ++j) red[tid * V + j] = acc[t][j];
    }
    __syncthreads();
    if (slot == 0) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float s = acc[t][j];
        for (int q = 1; q < slots; ++q) s += red[(q * cgl + g) * V + j];
        p.ws[((size_t)blockIdx.x * c + c0 + j) * 9 + t] = s;
      }
    }
  }
}

static int dwb_chunk(int cg, int max_cg) {  // channel vectors per workgroup: the fewest chunks that fit, of equal size
  const int chunks = cdiv(cg, max_cg);
  return cdiv(cg, chunks);
}
static long long dwb_wgs(int n, int h) { return (long long)n * cdiv(h, DWB_R); }

// The checks the two fused entries share (after dwt_check): npix >= 2 (train-mode BatchNorm needs more than one value per channel), the
// limits of the element-wise passes they reuse, the workgroup count.
static int dwb_check(const char* what, int n, int h, int w, int c, int act, int dtype) {
  if (act != UPA_ACT_NONE && act != UPA_ACT_SILU) {
    upa_set_error("%s: act %d (none | SiLU)", what, act);
    return UPA_EUNSUPPORTED;
  }
  if ((long long)n * h * w < 2) {
    upa_set_error("%s: BatchNorm in train mode needs more than one value per channel (n*h*w = %lld)", what, (long long)n * h * w);
    return UPA_EINVAL;
  }
  const int V = 16 / upa_elem_size(dtype);
  if (c > 256 * V || dwb_wgs(n, h) > 0x7fffffffll / (9ll * c)) {
    upa_set_error("%s: c = %d / %lld row bands outside the fused form", what, c, dwb_wgs(n, h));
    return UPA_EUNSUPPORTED;
  }
  return UPA_OK;
}

extern "C" size_t upa_dwconv2d_bn_act_fwd_workspace_bytes(int n, int h, int w, int c) {
  return n > 0 && h > 0 && w > 0 && c > 0 ? (size_t)dwb_wgs(n, h) * 2 * c * sizeof(float) : 0;
}

extern "C" int upa_bn_act_fwd(const void* z, long npix, int c, int ldz, const float* mean, const float* var, const float* gamma,
                              const float* beta, float eps, int act, void* y, int ldy, const void* residual, int ldr, int dtype, void* stream);

extern "C" int upa_dwconv2d_bn_act_fwd(const void* x, int n, int h, int w, int c, int ldx, const float* w_c133, void* z, int ldz, float momentum,
                                       float* mean, float* var, float* running_mean, float* running_var, const float* gamma, const float* beta,
                                       float eps, int act, void* y, int ldy, void* ws, size_t ws_bytes, int dtype, void* stream) {
  UPA_CHECK_ARG(x && w_c133 && z && mean && var && gamma && beta && y && ws, "dwconv2d_bn_act_fwd: null pointer");
  int rc = dwt_check("dwconv2d_bn_act_fwd", n, h, w, c, dtype);
  if (rc == UPA_OK) rc = dwb_check("dwconv2d_bn_act_fwd", n, h, w, c, act, dtype);
  if (rc != UPA_OK) return rc;
  const int es = upa_elem_size(dtype), V = 16 / es;
  UPA_CHECK_ARG(dwt_view_ok(x, ldx, c, V) && dwt_view_ok(z, ldz, c, V) && dwt_view_ok(y, ldy, c, V),
                "dwconv2d_bn_act_fwd: views need ld >= c, ld %% %d == 0 and 16-byte alignment", V);
  const size_t xb = dwt_view_bytes(n, h, w, c, ldx, es), zb = dwt_view_bytes(n, h, w, c, ldz, es), yb = dwt_view_bytes(n, h, w, c, ldy, es);
  UPA_CHECK_ARG(!dwt_overlap(x, xb, z, zb) && !dwt_overlap(x, xb, y, yb) && !dwt_overlap(z, zb, y, yb),
                "dwconv2d_bn_act_fwd: x, z and y must not overlap");
  const size_t need = upa_dwconv2d_bn_act_fwd_workspace_bytes(n, h, w, c);
  UPA_CHECK_ARG(((uintptr_t)ws % 16) == 0 && ws_bytes >= need, "dwconv2d_bn_act_fwd: workspace of %zu bytes, %zu needed (16-byte aligned)", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const int cg = c / V, CC = dwb_chunk(cg, DWB_FWD_CG), bands = cdiv(h, DWB_R);
  const dim3 grid((unsigned)dwb_wgs(n, h), (unsigned)cdiv(cg, CC));
  const size_t lds = (size_t)(DWB_HP * CC * 16 > 256 * V * 8 ? DWB_HP * CC * 16 : 256 * V * 8);
  if (dtype == UPA_BF16)
    hipLaunchKernelGGL((dwconv3_bn_fwd_kernel<bf16_t, 8>), grid, dim3(256), lds, s, (const bf16_t*)x, h, w, c, ldx, w_c133, (bf16_t*)z, ldz, (float*)ws,
                       CC, bands);
  else
    hipLaunchKernelGGL((dwconv3_bn_fwd_kernel<float, 4>), grid, dim3(256), lds, s, (const float*)x, h, w, c, ldx, w_c133, (float*)z, ldz, (float*)ws,
                       CC, bands);
  UPA_LAUNCH_CHECK();
  // The two entries below run after z and ws are written.  Every argument check they make (null pointers, c, ld, alignment, act, dtype,
  // npix >= 2) is a subset of the ones made above, so they cannot refuse here; a check added to either must be repeated above, or a
  // refusal would no longer leave every buffer untouched.
  const long npix = (long)n * h * w;
  rc = upa_bn_finalize_rows((const float*)ws, (int)grid.x, c, npix, c, momentum, mean, var, running_mean, running_var, stream);
  if (rc != UPA_OK) return rc;
  return upa_bn_act_fwd(z, npix, c, ldz, mean, var, gamma, beta, eps, act, y, ldy, nullptr, 0, dtype, stream);
}

extern "C" size_t upa_dwconv_bn_act_bwd_workspace_bytes(int n, int h, int w, int c) {
  return n > 0 && h > 0 && w > 0 && c > 0 ? (size_t)dwb_wgs(n, h) * c * 9 * sizeof(float) : 0;
}

// dx may be another channel slice of a buffer x, z or dy lives in (same pitch, disjoint channels); any other overlap is a race between
// the workgroup that writes a pixel and the neighbours that read it
static bool dwb_dx_clash(const void* dx, int lddx, const void* a, int lda, int n, int h, int w, int c, int es) {
  if (!dwt_overlap(dx, dwt_view_bytes(n, h, w, c, lddx, es), a, dwt_view_bytes(n, h, w, c, lda, es))) return false;
  if (lddx != lda) return true;
  const long long pitch = (long long)lda * es, d = (const char*)dx - (const char*)a;
  const long long r = ((d % pitch) + pitch) % pitch;  // dx's first channel inside a's pixel
  return !(r >= (long long)c * es && r + (long long)c * es <= pitch);
}

extern "C" int upa_dwconv_bn_act_bwd(const void* x, int n, int h, int w, int c, int ldx, const void* z, const void* dy, int ldz, int lddy,
                                     const float* mean, const float* var, const float* gamma, const float* beta, float eps, int act, float* dgamma,
                                     float* dbeta, double* red_ws, const float* w_c133, float* dw_c133, int accumulate_dw, void* dx, int lddx,
                                     int accumulate_dx, void* ws, size_t ws_bytes, int dtype, void* stream) {
  UPA_CHECK_ARG(x && z && dy && mean && var && gamma && beta && dgamma && dbeta && red_ws && w_c133 && dw_c133 && ws,
                "dwconv_bn_act_bwd: null pointer");
  int rc = dwt_check("dwconv_bn_act_bwd", n, h, w, c, dtype);
  if (rc == UPA_OK) rc = dwb_check("dwconv_bn_act_bwd", n, h, w, c, act, dtype);
  if (rc != UPA_OK) return rc;
  const int es = upa_elem_size(dtype), V = 16 / es;
  UPA_CHECK_ARG(dwt_view_ok(x, ldx, c, V) && dwt_view_ok(z, ldz, c, V) && dwt_view_ok(dy, lddy, c, V) && (!dx || dwt_view_ok(dx, lddx, c, V)),
                "dwconv_bn_act_bwd: views need ld >= c, ld %% %d == 0 and 16-byte alignment", V);
  UPA_CHECK_ARG(!dx || !(dwb_dx_clash(dx, lddx, x, ldx, n, h, w, c, es) || dwb_dx_clash(dx, lddx, z, ldz, n, h, w, c, es) ||
                         dwb_dx_clash(dx, lddx, dy, lddy, n, h, w, c, es)),
                "dwconv_bn_act_bwd: dx overlaps x, z or dy");
  const size_t need = upa_dwconv_bn_act_bwd_workspace_bytes(n, h, w, c);
  UPA_CHECK_ARG(((uintptr_t)ws % 16) == 0 && ws_bytes >= need, "dwconv_bn_act_bwd: workspace of %zu bytes, %zu needed (16-byte aligned)", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const long npix = (long)n * h * w;
  const double* fin = upa_bn_bwd_sums(z, dy, npix, c, ldz, lddy, mean, var, gamma, beta, eps, act, dgamma, dbeta, 1, red_ws, dtype, s);
  UPA_LAUNCH_CHECK();
  DwBwdParams p{};
  p.x = x; p.z = z; p.dy = dy; p.dx = dx; p.h = h; p.w = w; p.c = c; p.ldx = ldx; p.ldz = ldz; p.lddy = lddy; p.lddx = lddx;
  p.wt = w_c133; p.mean = mean; p.var = var; p.gamma = gamma; p.beta = beta; p.s0 = fin; p.s1 = fin + c; p.eps = eps;
  p.inv = 1.0f / (float)npix; p.act = act; p.accumulate_dx = accumulate_dx; p.ws = (float*)ws;
  const int cg = c / V;
  p.CC = dwb_chunk(cg, DWB_BWD_CH / V); p.bands = cdiv(h, DWB_R);
  const dim3 grid((unsigned)dwb_wgs(n, h), (unsigned)cdiv(cg, p.CC));
  const int dzb = DWB_HP * p.CC * V * 4 > 256 * V * 4 ? DWB_HP * p.CC * V * 4 : 256 * V * 4;
  const size_t lds = (size_t)dzb + (size_t)DWB_HP * p.CC * 16;
  if (dtype == UPA_BF16) hipLaunchKernelGGL((dwconv3_bn_bwd_kernel<bf16_t, 8>), grid, dim3(256), lds, s, p);
  else hipLaunchKernelGGL((dwconv3_bn_bwd_kernel<float, 4>), grid, dim3(256), lds, s, p);
  UPA_LAUNCH_CHECK();
  hipLaunchKernelGGL(dwconv3_wgrad_combine_kernel, dim3((unsigned)cdiv(c * 9, 256)), dim3(256), 0, s, (const float*)ws, (int)grid.x, c * 9, dw_c133,
                     accumulate_dw);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}
