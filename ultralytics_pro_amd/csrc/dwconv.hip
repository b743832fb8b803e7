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
