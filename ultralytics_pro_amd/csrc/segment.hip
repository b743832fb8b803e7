// Instance segmentation: the Proto upsampling conv, the mask-coefficient layout, the coefficient gather behind NMS and the
// mask assembly (ultralytics/nn/modules/block.py:257-276 Proto, nn/modules/head.py:790-837 Segment, utils/nms.py:74-122,
// utils/ops.py:489-583 crop_mask / process_mask / process_mask_native / scale_masks).
//
//  - upa_conv_transpose2x2: nn.ConvTranspose2d(k = 2, s = 2, p = 0) with bias as ONE GEMM, (pixels x Cin) . (Cin x 4 Cout), whose
//    column q = tap * Cout + co is stored to output pixel (2y + tap / 2, 2x + tap % 2).  bf16 on v_mfma_f32_16x16x32_bf16, f32 on the
//    exact-f32 v_mfma_f32_16x16x4_f32; both accumulate in f32.
//  - upa_process_mask: per (detection row, output tile) a workgroup computes the proto-resolution mask values the tile's bilinear
//    taps read (nm-deep dot products, one-pixel halo) into LDS, crops them with crop_mask's float comparisons, resamples with
//    torch's upsample_bilinear2d rule (align_corners = False, source index clamped at 0), thresholds at > 0 and writes bytes.
#include "common.h"
#include "mask_dot.h"

namespace {

// ---- ConvTranspose2d(2, 2) ---------------------------------------------------------------------------------------------------------
// Block = 4 waves = 64 pixels x 64 GEMM columns; wave w owns pixels [16 w, 16 w + 16) of the block and four 16-column MFMA tiles.
// Operands come straight from global memory (the packed weight slab of a block is 64 x Kp, reused by every block: L2 resident).
// Packed weight: row q = tap * cout + co (4 cout rows), Kp = cin rounded up to the MFMA depth, zero filled; element (q, ci).
constexpr int CT_KB16 = 32;  // bf16 MFMA depth
constexpr int CT_KF32 = 4;   // f32 MFMA depth

template <bool BF16>
__global__ __launch_bounds__(256) void convt2x2_kernel(const void* __restrict__ xv, int npix, int h, int w, int cin, int ldx,
                                                       const void* __restrict__ wpv, int kp, const float* __restrict__ bias,
                                                       void* __restrict__ yv, int cout, int ldy) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int p = blockIdx.x * 64 + wave * 16 + r;  // this lane's A row (pixel)
  const int q0 = blockIdx.y * 64;                 // first GEMM column of the block
  const int ncol = 4 * cout;
  const bool prow = p < npix;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (BF16) {
    const bf16_t* x = (const bf16_t*)xv + (size_t)(prow ? p : 0) * ldx;
    const bf16_t* wp = (const bf16_t*)wpv;
    for (int k0 = 0; k0 < kp; k0 += CT_KB16) {
      const int k = k0 + 8 * g;  // this lane's 8 consecutive k (the same k slots for A and B: any slot order gives the same sum)
      u32x4 a = u32x4{0u, 0u, 0u, 0u};
      if (prow && k < cin) a = *reinterpret_cast<const u32x4*>(x + k);  // cin % 8 == 0: a group is all in or all out
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int q = q0 + 16 * t + r;
        u32x4 b = u32x4{0u, 0u, 0u, 0u};
        if (q < ncol) b = *reinterpret_cast<const u32x4*>(wp + (size_t)q * kp + k);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&a), *reinterpret_cast<const bf16x8*>(&b),
                                                         acc[t], 0, 0, 0);
      }
    }
  } else {
    const float* x = (const float*)xv + (size_t)(prow ? p : 0) * ldx;
    const float* wp = (const float*)wpv;
    for (int k0 = 0; k0 < kp; k0 += CT_KF32) {
      const int k = k0 + g;
      const float a = (prow && k < cin) ? x[k] : 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int q = q0 + 16 * t + r;
        const float b = q < ncol ? wp[(size_t)q * kp + k] : 0.f;
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t], 0, 0, 0);
      }
    }
  }
  // D[row = 4 g + v][col = r] of each tile: pixel blockIdx.x * 64 + wave * 16 + 4 g + v, column q0 + 16 t + r
  const int hw = h * w, oh = 2 * h, ow = 2 * w;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int q = q0 + 16 * t + r;
    if (q >= ncol) continue;
    const int tap = q / cout, co = q - tap * cout;
    const float bv = bias[co];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int pp = blockIdx.x * 64 + wave * 16 + 4 * g + v;
      if (pp >= npix) continue;
      const int n = pp / hw, rem = pp - n * hw, yy = rem / w, xx = rem - yy * w;
      const size_t o = (((size_t)n * oh + 2 * yy + (tap >> 1)) * ow + 2 * xx + (tap & 1)) * (size_t)ldy + co;
      const float val = acc[t][v] + bv;
      if constexpr (BF16) ((bf16_t*)yv)[o] = f32_to_bf16(val);
      else ((float*)yv)[o] = val;
    }
  }
}

// ---- mask coefficients: NHWC level map -> (B, C, A) rows at anchor offset a0 --------------------------------------------------------
template <typename T>
__global__ void coef_rows_kernel(const T* __restrict__ x, int n, int hw, int c, int ldx, float* __restrict__ out, long img_stride,
                                 int a_total, int a0) {
  const long total = (long)n * c * hw;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int pix = (int)(i % hw);  // consecutive threads: consecutive anchors of one channel row (coalesced stores)
    const long rest = i / hw;
    const int ch = (int)(rest % c), b = (int)(rest / c);
    out[b * img_stride + (long)ch * a_total + a0 + pix] = ElemTraits<T>::load(x + ((size_t)b * hw + pix) * ldx + ch);
  }
}

// ---- coefficient rows of the kept detections --------------------------------------------------------------------------------------
__global__ void gather_extra_kernel(const float* __restrict__ extra, int b, int ne, int a, const int32_t* __restrict__ keep,
                                    const int32_t* __restrict__ counts, int max_det, const float* __restrict__ det, float* __restrict__ out,
                                    int ldo) {
  const int cols = ne + (det ? 6 : 0);
  const long total = (long)b * max_det * cols;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int col = (int)(i % cols);
    const long row = i / cols;
    const int img = (int)(row / max_det), j = (int)(row % max_det);
    float v = 0.f;
    if (j < counts[img]) {
      if (det && col < 6) {
        v = det[row * 6 + col];
      } else {
        const int k = col - (det ? 6 : 0);
        const int idx = keep[row];
        if (idx >= 0 && idx < a) v = extra[((long)img * ne + k) * a + idx];
      }
    }
    out[row * ldo + col] = v;
  }
}

// ---- mask assembly --------------------------------------------------------------------------------------------------------------
constexpr int PM_LDS = 8192;  // proto-resolution values of one tile window (floats)
constexpr int PM_NM = 128;    // coefficient depth limit
constexpr int PM_B = 1024;    // batch limit (per-image row offsets live in LDS)

struct PMArgs {
  const void* protos;
  int ldp, mh, mw, nm, bf16;
  const float* coef;
  long coef_img;
  int coef_ld;
  const float* det;
  long det_img;
  int det_ld;
  const int32_t* counts;
  int b;
  int H, W, mode;  // mode 0: crop at proto resolution (boxes x (cx, cy)), then resample; 1: resample, then crop in output coordinates
  float cx, cy;
  int top, left, wh, ww;  // source window of the proto map
  float sy, sx;           // window / output size (torch's area_pixel_compute_scale)
  int th, tw, tiles_x, tiles;
  uint8_t* masks;
  int32_t* nonempty;
  int capacity;
  int32_t* total;
};

// torch upsample_bilinear2d source index (align_corners = False): max(scale (d + 0.5) - 0.5, 0), i0 = floor, i1 = i0 + (i0 < n - 1)
__host__ __device__ inline void bil_idx(float scale, int d, int n, int& i0, int& i1, float& l1) {
  float s = scale * ((float)d + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  if (i0 > n - 1) i0 = n - 1;
  i1 = i0 + (i0 < n - 1 ? 1 : 0);
  l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

__global__ __launch_bounds__(256) void process_mask_kernel(PMArgs A) {
  __shared__ float win[PM_LDS];
  __shared__ float coef[PM_NM];
  __shared__ int base[PM_B + 1];
  __shared__ float box[4];
  const int tid = threadIdx.x;
  if (tid == 0) {  // exclusive prefix sum of the counts (on the device: the launch is graph-capturable)
    int s = 0;
    for (int i = 0; i < A.b; ++i) {
      base[i] = s;
      s += A.counts[i];
    }
    base[A.b] = s;
    if (blockIdx.x == 0 && blockIdx.y == 0) *A.total = s;
  }
  __syncthreads();
  const int rows = min(base[A.b], A.capacity);
  const int tile = blockIdx.x;
  const int ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
  const int y0 = ty * A.th, x0 = tx * A.tw;
  const int y1 = min(y0 + A.th, A.H), x1 = min(x0 + A.tw, A.W);
  // source window rows / columns the tile's bilinear taps read (monotonic in the output index)
  int ys0, ys1, xs0, xs1, dummy;
  float fl;
  bil_idx(A.sy, y0, A.wh, ys0, dummy, fl);
  bil_idx(A.sy, y1 - 1, A.wh, dummy, ys1, fl);
  bil_idx(A.sx, x0, A.ww, xs0, dummy, fl);
  bil_idx(A.sx, x1 - 1, A.ww, dummy, xs1, fl);
  const int wr = ys1 - ys0 + 1, wc = xs1 - xs0 + 1;
  if (wr * wc > PM_LDS) return;  // unreachable: the host checks every tile's window with this same arithmetic (pm_window_fits)
  const int pitch = A.tw / 16;   // 16-pixel groups per tile row
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    int img = 0;
    while (row >= base[img + 1]) ++img;
    const int j = row - base[img];
    const float* cr = A.coef + img * A.coef_img + (long)j * A.coef_ld;
    const float* dr = A.det + img * A.det_img + (long)j * A.det_ld;
    __syncthreads();  // the previous row is done with win / coef / box
    for (int k = tid; k < A.nm; k += 256) coef[k] = cr[k];
    if (tid < 4) box[tid] = dr[tid];
    __syncthreads();
    const float bx1 = box[0], by1 = box[1], bx2 = box[2], by2 = box[3];
    // crop_mask's comparison form on `boxes * ratios` (f32 products, ops.py:527-531, :510-513)
    const float cx1 = bx1 * A.cx, cy1 = by1 * A.cy, cx2 = bx2 * A.cx, cy2 = by2 * A.cy;
    for (int i = tid; i < wr * wc; i += 256) {
      const int wy = i / wc, wx = i - wy * wc;
      const int py = A.top + ys0 + wy, px = A.left + xs0 + wx;
      float acc;  // masks_in @ protos: k ascending, one fma per term (mask_dot.h)
      if (A.bf16) acc = mask_dot_bf16(coef, (const bf16_t*)A.protos + ((size_t)img * A.mh * A.mw + (size_t)py * A.mw + px) * A.ldp, A.nm);
      else acc = mask_dot_f32(coef, (const float*)A.protos + ((size_t)img * A.mh * A.mw + (size_t)py * A.mw + px) * A.ldp, A.nm);
      if (A.mode == 0) acc = mask_in_crop((float)px, (float)py, cx1, cy1, cx2, cy2) ? acc : 0.f;
      win[i] = acc;
    }
    __syncthreads();
    uint8_t* mrow = A.masks + (size_t)row * A.H * A.W;
    bool any = false;
    for (int gi = tid; gi < (A.th * pitch); gi += 256) {
      const int gy = gi / pitch, gx = gi - gy * pitch;
      const int y = y0 + gy, xb = x0 + 16 * gx;
      if (y >= y1 || xb >= x1) continue;
      int i0, i1;
      float ly1;
      bil_idx(A.sy, y, A.wh, i0, i1, ly1);
      const float ly0 = 1.f - ly1;
      const float* r0 = win + (i0 - ys0) * wc;
      const float* r1 = win + (i1 - ys0) * wc;
      const float fy = (float)y;
      const bool yin = A.mode == 0 || (fy >= by1 && fy < by2);
      unsigned word[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int x = xb + e;
        int j0, j1;
        float lx1;
        bil_idx(A.sx, x < x1 ? x : x1 - 1, A.ww, j0, j1, lx1);  // past the tile: any in-window taps, the bit is masked off
        const float lx0 = 1.f - lx1;
        const float v = ly0 * (lx0 * r0[j0 - xs0] + lx1 * r0[j1 - xs0]) + ly1 * (lx0 * r1[j0 - xs0] + lx1 * r1[j1 - xs0]);
        const float fx = (float)x;
        const bool in = yin && (A.mode == 0 || (fx >= bx1 && fx < bx2));
        const unsigned bit = (x < x1 && in && v > 0.f) ? 1u : 0u;
        word[e >> 2] |= bit << (8 * (e & 3));
      }
      any |= (word[0] | word[1] | word[2] | word[3]) != 0u;
      uint8_t* o = mrow + (size_t)y * A.W + xb;
      if (xb + 16 <= A.W && (((uintptr_t)o) & 15) == 0) {
        *reinterpret_cast<u32x4*>(o) = u32x4{word[0], word[1], word[2], word[3]};
      } else {
        for (int e = 0; e < 16 && xb + e < A.W; ++e) o[e] = (uint8_t)((word[e >> 2] >> (8 * (e & 3))) & 0xffu);
      }
    }
    if (any) A.nonempty[row] = 1;  // every writer stores the same value
  }
}

// the largest source window (rows x columns) over all tiles of a th x tw tiling, computed with the kernel's own index arithmetic
static long pm_max_window(float sy, float sx, int wh, int ww, int H, int W, int th, int tw) {
  int d, a, b;
  float fl;
  long mr = 0, mc = 0;
  for (int y0 = 0; y0 < H; y0 += th) {
    bil_idx(sy, y0, wh, a, d, fl);
    bil_idx(sy, (y0 + th < H ? y0 + th : H) - 1, wh, d, b, fl);
    if (b - a + 1 > mr) mr = b - a + 1;
  }
  for (int x0 = 0; x0 < W; x0 += tw) {
    bil_idx(sx, x0, ww, a, d, fl);
    bil_idx(sx, (x0 + tw < W ? x0 + tw : W) - 1, ww, d, b, fl);
    if (b - a + 1 > mc) mc = b - a + 1;
  }
  return mr * mc;
}

// ---- crop_mask (comparison form) and the bilinear resize of scale_masks, on float masks ---------------------------------------------
__global__ void crop_mask_kernel(const float* __restrict__ m, int n, int h, int w, const float* __restrict__ boxes, int box_ld,
                                 float* __restrict__ out) {
  const long total = (long)n * h * w;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int x = (int)(i % w);
    const long r = i / w;
    const int y = (int)(r % h), k = (int)(r / h);
    const float* b = boxes + (long)k * box_ld;
    const float fx = (float)x, fy = (float)y;
    const bool in = fx >= b[0] && fx < b[2] && fy >= b[1] && fy < b[3];
    out[i] = m[i] * (in ? 1.f : 0.f);  // masks * bool: -0 / NaN propagate as in the reference
  }
}

__global__ void resize_bilinear_kernel(const float* __restrict__ x, int planes, int h, int w, int top, int left, int wh, int ww,
                                       float sy, float sx, float* __restrict__ y, int oh, int ow) {
  const long total = (long)planes * oh * ow;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ox = (int)(i % ow);
    const long r = i / ow;
    const int oy = (int)(r % oh), pl = (int)(r / oh);
    int i0, i1, j0, j1;
    float ly1, lx1;
    bil_idx(sy, oy, wh, i0, i1, ly1);
    bil_idx(sx, ox, ww, j0, j1, lx1);
    const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const float* p = x + (long)pl * h * w;
    const float* r0 = p + (long)(top + i0) * w + left;
    const float* r1 = p + (long)(top + i1) * w + left;
    y[i] = ly0 * (lx0 * r0[j0] + lx1 * r0[j1]) + ly1 * (lx0 * r1[j0] + lx1 * r1[j1]);
  }
}

__global__ void copy_rows_kernel(const float* __restrict__ src, long rows, int cols, long lds, float* __restrict__ dst, long ldd) {
  const long total = rows * cols;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / cols;
    const int c = (int)(i - r * cols);
    dst[r * ldd + c] = src[r * lds + c];
  }
}

static unsigned grid_of(long total) { return (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192); }

}  // namespace

// ---- entry points ------------------------------------------------------------------------------------------------------------------

extern "C" size_t upa_conv_transpose2x2_packed_weight_bytes(int cin, int cout, int dtype) {
  if (cin <= 0 || cout <= 0) return 0;
  const int kb = dtype == UPA_BF16 ? CT_KB16 : CT_KF32;
  const size_t kp = (size_t)cdiv(cin, kb) * kb;
  return kp * 4 * (size_t)cout * upa_elem_size(dtype);
}

extern "C" int upa_pack_conv_transpose2x2_weight(const float* w, int cin, int cout, int dtype, void* out) {
  UPA_CHECK_ARG(w && out && cin > 0 && cout > 0, "pack_conv_transpose2x2_weight: bad args");
  UPA_CHECK_ARG(dtype == UPA_F32 || dtype == UPA_BF16, "pack_conv_transpose2x2_weight: dtype %d", dtype);
  const int kb = dtype == UPA_BF16 ? CT_KB16 : CT_KF32;
  const int kp = cdiv(cin, kb) * kb;
  for (int tap = 0; tap < 4; ++tap)
    for (int co = 0; co < cout; ++co)
      for (int k = 0; k < kp; ++k) {
        const float v = k < cin ? w[((size_t)k * cout + co) * 4 + tap] : 0.f;  // W[ci][co][i][j], tap = 2 i + j
        const size_t o = ((size_t)tap * cout + co) * kp + k;
        if (dtype == UPA_BF16) {
          unsigned u;
          memcpy(&u, &v, 4);
          u += 0x7fffu + ((u >> 16) & 1u);  // round to nearest even (weights are finite)
          ((bf16_t*)out)[o] = (bf16_t)(u >> 16);
        } else {
          ((float*)out)[o] = v;
        }
      }
  return UPA_OK;
}

extern "C" int upa_conv_transpose2x2(const void* x, int n, int h, int w, int cin, int ldx, const void* w_packed, const float* bias, void* y,
                                     int cout, int ldy, int dtype, void* stream) {
  UPA_CHECK_ARG(x && w_packed && bias && y, "conv_transpose2x2: null pointer");
  UPA_CHECK_ARG(n > 0 && h > 0 && w > 0 && cin > 0 && cout > 0 && ldx >= cin && ldy >= cout,
                "conv_transpose2x2: bad shape n=%d h=%d w=%d cin=%d ldx=%d cout=%d ldy=%d", n, h, w, cin, ldx, cout, ldy);
  if (dtype != UPA_F32 && dtype != UPA_BF16) {
    upa_set_error("conv_transpose2x2: dtype %d outside f32 | bf16", dtype);
    return UPA_EUNSUPPORTED;
  }
  const int es = upa_elem_size(dtype), vec = 16 / es;
  UPA_CHECK_ARG(cin % vec == 0 && ldx % vec == 0 && cout % vec == 0 && ldy % vec == 0 && ((uintptr_t)x % 16) == 0,
                "conv_transpose2x2: channel counts / strides must be multiples of 16 bytes");
  const long long npix = (long long)n * h * w;
  if (npix > 0x7fffffffll || (long long)n * 4 * h * w * ldy > (1ll << 40)) {
    upa_set_error("conv_transpose2x2: %lld pixels", npix);
    return UPA_EUNSUPPORTED;
  }
  const int kb = dtype == UPA_BF16 ? CT_KB16 : CT_KF32;
  const int kp = cdiv(cin, kb) * kb;
  const dim3 grid((unsigned)cdiv((int)npix, 64), (unsigned)cdiv(4 * cout, 64));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UPA_BF16)
    hipLaunchKernelGGL(convt2x2_kernel<true>, grid, dim3(256), 0, s, x, (int)npix, h, w, cin, ldx, w_packed, kp, bias, y, cout, ldy);
  else
    hipLaunchKernelGGL(convt2x2_kernel<false>, grid, dim3(256), 0, s, x, (int)npix, h, w, cin, ldx, w_packed, kp, bias, y, cout, ldy);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_mask_coef_rows(const void* x, int n, int h, int w, int c, int ldx, int dtype, float* out, int c_total, int c0, int a_total,
                                  int a0, void* stream) {
  UPA_CHECK_ARG(x && out, "mask_coef_rows: null pointer");
  UPA_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0 && ldx >= c && c0 >= 0 && c0 + c <= c_total && a0 >= 0 && a0 + h * w <= a_total,
                "mask_coef_rows: bad shape n=%d h=%d w=%d c=%d ldx=%d c0=%d c_total=%d a0=%d a_total=%d", n, h, w, c, ldx, c0, c_total, a0,
                a_total);
  if (dtype != UPA_F32 && dtype != UPA_BF16) {
    upa_set_error("mask_coef_rows: dtype %d", dtype);
    return UPA_EUNSUPPORTED;
  }
  const long total = (long)n * c * h * w;
  const unsigned grid = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  const long img = (long)c_total * a_total;
  float* o = out + (long)c0 * a_total;
  if (dtype == UPA_BF16)
    hipLaunchKernelGGL(coef_rows_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, n, h * w, c, ldx, o, img,
                       a_total, a0);
  else
    hipLaunchKernelGGL(coef_rows_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)x, n, h * w, c, ldx, o, img,
                       a_total, a0);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_nms_gather_extra(const float* extra, int b, int ne, int a, const int32_t* keep, const int32_t* counts, int max_det,
                                    const float* det, float* out, int ldo, void* stream) {
  UPA_CHECK_ARG(extra && keep && counts && out, "nms_gather_extra: null pointer");
  UPA_CHECK_ARG(b > 0 && ne > 0 && a > 0 && max_det > 0 && ldo >= ne + (det ? 6 : 0), "nms_gather_extra: bad shape b=%d ne=%d a=%d max_det=%d ldo=%d",
                b, ne, a, max_det, ldo);
  const long total = (long)b * max_det * (ne + (det ? 6 : 0));
  const unsigned grid = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(gather_extra_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, extra, b, ne, a, keep, counts, max_det, det, out, ldo);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_process_mask(const void* protos, int b, int mh, int mw, int nm, int ldp, int dtype, const float* coef, int coef_ld,
                                const float* det, int det_ld, int max_det, const int32_t* counts, int out_h, int out_w, int mode,
                                float crop_sx, float crop_sy, int top, int left, int bottom, int right, unsigned char* masks,
                                int32_t* nonempty, int capacity, int32_t* total, void* stream) {
  UPA_CHECK_ARG(protos && coef && det && counts && total, "process_mask: null pointer");
  UPA_CHECK_ARG(b > 0 && mh > 0 && mw > 0 && nm > 0 && ldp >= nm && coef_ld >= nm && det_ld >= 4 && max_det > 0 && out_h > 0 && out_w > 0 &&
                capacity >= 0 && (capacity == 0 || (masks && nonempty)),
                "process_mask: bad shape b=%d mh=%d mw=%d nm=%d ldp=%d max_det=%d out=%dx%d capacity=%d", b, mh, mw, nm, ldp, max_det, out_h,
                out_w, capacity);
  UPA_CHECK_ARG(0 <= top && top < bottom && bottom <= mh && 0 <= left && left < right && right <= mw,
                "process_mask: bad source window [%d:%d, %d:%d] of a %dx%d proto map", top, bottom, left, right, mh, mw);
  if ((dtype != UPA_F32 && dtype != UPA_BF16) || (mode != 0 && mode != 1) || nm > PM_NM || b > PM_B) {
    upa_set_error("process_mask: dtype %d mode %d nm %d b %d outside the supported form (f32 | bf16, mode 0 | 1, nm <= %d, b <= %d)", dtype,
                  mode, nm, b, PM_NM, PM_B);
    return UPA_EUNSUPPORTED;
  }
  const int vec = 16 / upa_elem_size(dtype);
  UPA_CHECK_ARG(nm % vec == 0 && ldp % vec == 0 && ((uintptr_t)protos % 16) == 0, "process_mask: proto channels must be 16-byte groups");
  PMArgs A;
  A.protos = protos, A.ldp = ldp, A.mh = mh, A.mw = mw, A.nm = nm, A.bf16 = dtype == UPA_BF16;
  A.coef = coef, A.coef_ld = coef_ld, A.coef_img = (long)max_det * coef_ld;
  A.det = det, A.det_ld = det_ld, A.det_img = (long)max_det * det_ld;
  A.counts = counts, A.b = b, A.H = out_h, A.W = out_w, A.mode = mode, A.cx = crop_sx, A.cy = crop_sy;
  A.top = top, A.left = left, A.wh = bottom - top, A.ww = right - left;
  A.sy = (float)A.wh / (float)out_h, A.sx = (float)A.ww / (float)out_w;
  A.masks = masks, A.nonempty = nonempty, A.capacity = capacity, A.total = total;
  // the largest tile whose every source window fits in LDS (exact: the kernel's index arithmetic, run on the host)
  static const int cand[][2] = {{32, 128}, {16, 128}, {16, 64}, {8, 64}, {8, 32}, {4, 32}, {4, 16}, {2, 16}, {1, 16}};
  int th = 0, tw = 0;
  for (const auto& c : cand) {
    if (pm_max_window(A.sy, A.sx, A.wh, A.ww, out_h, out_w, c[0], c[1]) <= PM_LDS) {
      th = c[0], tw = c[1];
      break;
    }
  }
  if (th == 0) {
    upa_set_error("process_mask: a %dx%d proto window over a %dx%d output does not fit the tile buffer", A.wh, A.ww, out_h, out_w);
    return UPA_EUNSUPPORTED;
  }
  A.th = th, A.tw = tw, A.tiles_x = cdiv(out_w, tw), A.tiles = A.tiles_x * cdiv(out_h, th);
  const long long plane = (long long)out_h * out_w;
  if ((long long)A.tiles > 0x7fffffffll || plane * (long long)(capacity > 0 ? capacity : 1) > (1ll << 40)) {
    upa_set_error("process_mask: output too large");
    return UPA_EUNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  if (capacity > 0) upa_zero_words(nonempty, capacity, s);
  const int gy = capacity < 1 ? 1 : (capacity < 1024 ? capacity : 1024);
  hipLaunchKernelGGL(process_mask_kernel, dim3((unsigned)A.tiles, (unsigned)gy), dim3(256), 0, s, A);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_crop_mask(const float* masks, int n, int h, int w, const float* boxes, int box_ld, float* out, void* stream) {
  UPA_CHECK_ARG(masks && boxes && out && n >= 0 && h > 0 && w > 0 && box_ld >= 4, "crop_mask: bad args n=%d h=%d w=%d box_ld=%d", n, h, w,
                box_ld);
  const long total = (long)n * h * w;
  if (total == 0) return UPA_OK;
  hipLaunchKernelGGL(crop_mask_kernel, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, masks, n, h, w, boxes, box_ld, out);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_resize_bilinear(const float* x, int planes, int h, int w, int top, int left, int bottom, int right, float* y, int out_h,
                                   int out_w, void* stream) {
  UPA_CHECK_ARG(x && y && planes >= 0 && h > 0 && w > 0 && out_h > 0 && out_w > 0, "resize_bilinear: bad shape");
  UPA_CHECK_ARG(0 <= top && top < bottom && bottom <= h && 0 <= left && left < right && right <= w,
                "resize_bilinear: bad window [%d:%d, %d:%d] of %dx%d", top, bottom, left, right, h, w);
  const long total = (long)planes * out_h * out_w;
  if (total == 0) return UPA_OK;
  const int wh = bottom - top, ww = right - left;
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, x, planes, h, w, top, left, wh, ww,
                     (float)wh / (float)out_h, (float)ww / (float)out_w, y, out_h, out_w);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_copy_rows(const float* src, long rows, int cols, long lds, float* dst, long ldd, void* stream) {
  UPA_CHECK_ARG(src && dst && rows >= 0 && cols >= 0 && lds >= cols && ldd >= cols, "copy_rows: bad shape");
  const long total = rows * cols;
  if (total == 0) return UPA_OK;
  hipLaunchKernelGGL(copy_rows_kernel, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, src, rows, cols, lds, dst, ldd);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}
