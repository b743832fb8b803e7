// Depthwise 3x3 convolution: DWConv (ultralytics/nn/modules/conv.py:411-425, Conv with groups = gcd(c1, c2) = C) with its BatchNorm
// folded on the host, y = act(sum_taps w[tap][c] * x[pixel + tap][c] + b[c]).  YOLO11 uses it in the non-legacy Detect class branch
// (nn/modules/head.py:98-110) and as `pe` of v10_Attention (block.py:1709); the `pe` form is fused into csrc/psa.hip.
//
// 9 MACs per output element: the kernel is bound by the activation bytes.  A thread owns V consecutive channels (one 16-byte
// vector: 8 bf16 or 4 f32) of one output pixel; consecutive threads take consecutive channel groups, then consecutive pixels, so a
// wave reads whole pixel rows and the x +- 1 neighbours of one thread are its neighbours' centre reads: the 3x3 neighbourhood is
// served from L1 / L2, HBM sees each input row about once per output row.  Channel counts that are not a multiple of V (or
// misaligned views) run the same code with V = 1.
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
