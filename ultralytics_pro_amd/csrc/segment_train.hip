// Segmentation training: the backward of Proto's ConvTranspose2d(c_, c_, 2, 2, 0, bias = True) (ultralytics/nn/modules/block.py:257-276)
// and the mask loss of v8SegmentationLoss with its gradients (utils/loss.py:622-709 calculate_segmentation_loss + single_mask_loss,
// utils/ops.py:510-513 crop_mask's comparison branch).
//
//  - upa_conv_transpose2x2_bwd.  With q = tap * cout + co (tap = 2 i + j) and U[p][q] = dy[n, 2 y + i, 2 x + j, co] (the pixel-unshuffle
//    gather of dy, p = (n, y, x)):
//      dx[p][ci]  = sum_q U[p][q] W[ci][co][i][j]     one GEMM (pixels x 4 cout) . (4 cout x cin), 64 x 64 tiles, K = 4 cout
//      dW[q][ci]  = sum_p U[p][q] x[p][ci]            one GEMM (4 cout x pixels) . (pixels x cin), 64 x 64 tiles, split over K = pixels:
//                                                     f32 partials per split, combined in split order (one order: deterministic)
//      db[co]     = sum over all pixels of dy         upa_channel_sum
//    bf16 operands on v_mfma_f32_16x16x32_bf16 (the f32 master weight is rounded to bf16 as the forward packing rounds it), f32 on the
//    exact-f32 v_mfma_f32_16x16x4_f32; both accumulate in f32.  Operands come straight from global memory.
//  - upa_mask_loss.  Four passes, no floating-point atomics:
//      1. per image: the foreground anchors compacted in anchor order into records (box in mask units, 1 / (mh mw area), mask id,
//         coefficient row); rows of the other anchors of the coefficient-gradient maps are zeroed by a pass of their own;
//      2. per foreground anchor: one workgroup walks the box, pred = coef . proto, BCE-with-logits against masks == mask_id, kept
//         where crop_mask's comparisons hold; its loss term and its coefficient gradient are reduced in one fixed order;
//      3. per (image, 64-pixel tile): dproto accumulated in registers over the image's records whose box meets the tile, stored once;
//      4. the item: the terms summed in one fixed order, / foreground count, * gain.
#include "common.h"

extern "C" int upa_channel_sum(const void* z, long npix, int c, int ldz, float* out, int accumulate, double* ws, int dtype, void* stream);
extern "C" size_t upa_channel_reduce_workspace_bytes(int c);

namespace {

// ---- ConvTranspose2d(2, 2) backward ------------------------------------------------------------------------------------------------
constexpr int CTB_MAX_SPLITS = 64;

__device__ __forceinline__ size_t dy_pixel(int p, int hw, int w, int tap) {  // pixel index of U[p][tap * cout + .] in dy's (n, 2h, 2w) grid
  const int n = p / hw, rem = p - n * hw, yy = rem / w, xx = rem - yy * w;
  const int h = hw / w;
  return ((size_t)n * 2 * h + 2 * yy + (tap >> 1)) * (size_t)(2 * w) + 2 * xx + (tap & 1);
}

// dx: block = 4 waves = 64 pixels x 64 input channels; wave w owns pixels [16 w, 16 w + 16) and four 16-channel MFMA tiles.
template <bool BF16>
__global__ __launch_bounds__(256) void convt2x2_dgrad_kernel(const void* __restrict__ dyv, int npix, int h, int w, int cout, int lddy,
                                                             const float* __restrict__ wt /* (cin, cout, 2, 2) */, int cin,
                                                             void* dxv, int lddx, int accumulate) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int p = blockIdx.x * 64 + wave * 16 + r;
  const int c0 = blockIdx.y * 64;
  const bool prow = p < npix;
  const int hw = h * w, K = 4 * cout;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (BF16) {
    const bf16_t* dy = (const bf16_t*)dyv;
    for (int k0 = 0; k0 < K; k0 += 32) {  // cout % 8 == 0: K % 32 == 0 and a lane's 8 k share one tap
      const int k = k0 + 8 * g;
      const int tap = k / cout, co = k - tap * cout;
      u32x4 a = u32x4{0u, 0u, 0u, 0u};
      if (prow) a = *reinterpret_cast<const u32x4*>(dy + dy_pixel(p, hw, w, tap) * (size_t)lddy + co);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int ci = c0 + 16 * t + r;
        u32x4 b = u32x4{0u, 0u, 0u, 0u};
        if (ci < cin) {
          const float* wp = wt + ((size_t)ci * cout + co) * 4 + tap;
          b[0] = pack_bf16x2(wp[0], wp[4]);
          b[1] = pack_bf16x2(wp[8], wp[12]);
          b[2] = pack_bf16x2(wp[16], wp[20]);
          b[3] = pack_bf16x2(wp[24], wp[28]);
        }
        acc[t] = mfma32(a, b, acc[t]);
      }
    }
  } else {
    const float* dy = (const float*)dyv;
    for (int k0 = 0; k0 < K; k0 += 4) {  // cout % 4 == 0: K % 16 == 0
      const int k = k0 + g;
      const int tap = k / cout, co = k - tap * cout;
      const float a = prow ? dy[dy_pixel(p, hw, w, tap) * (size_t)lddy + co] : 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int ci = c0 + 16 * t + r;
        const float b = ci < cin ? wt[((size_t)ci * cout + co) * 4 + tap] : 0.f;
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t], 0, 0, 0);
      }
    }
  }
  // D[row = 4 g + v][col = r]: pixel blockIdx.x * 64 + wave * 16 + 4 g + v, channel c0 + 16 t + r
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int ci = c0 + 16 * t + r;
    if (ci >= cin) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int pp = blockIdx.x * 64 + wave * 16 + 4 * g + v;
      if (pp >= npix) continue;
      const size_t o = (size_t)pp * lddx + ci;
      if constexpr (BF16) {
        bf16_t* dx = (bf16_t*)dxv;
        dx[o] = f32_to_bf16(acc[t][v] + (accumulate ? bf16_to_f32(dx[o]) : 0.f));
      } else {
        float* dx = (float*)dxv;
        dx[o] = acc[t][v] + (accumulate ? dx[o] : 0.f);
      }
    }
  }
}

// dW partials: block = 4 waves = 64 GEMM rows q x 64 input channels over the pixels [z * kc, (z + 1) * kc); wave w owns rows
// [16 w, 16 w + 16) and four 16-channel tiles.  part[z][q][ci].
template <bool BF16>
__global__ __launch_bounds__(256) void convt2x2_wgrad_kernel(const void* __restrict__ xv, int npix, int h, int w, int cin, int ldx,
                                                             const void* __restrict__ dyv, int cout, int lddy, int kc,
                                                             float* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int ncol = 4 * cout;
  const int q = blockIdx.x * 64 + wave * 16 + r;  // this lane's A row
  const int c0 = blockIdx.y * 64;
  const int kb = blockIdx.z * kc, ke = min(kb + kc, npix);
  const bool qrow = q < ncol;
  const int tap = qrow ? q / cout : 0, co = qrow ? q - tap * cout : 0;
  const int hw = h * w;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (BF16) {
    const bf16_t* x = (const bf16_t*)xv;
    const bf16_t* dy = (const bf16_t*)dyv;
    for (int k0 = kb; k0 < ke; k0 += 32) {
      unsigned short av[8], bv[4][8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {  // this lane's 8 k slots (pixels): the same slots for A and B
        const int p = k0 + 8 * g + e;
        const bool ok = p < ke;
        av[e] = (ok && qrow) ? dy[dy_pixel(p, hw, w, tap) * (size_t)lddy + co] : (unsigned short)0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int ci = c0 + 16 * t + r;
          bv[t][e] = (ok && ci < cin) ? x[(size_t)p * ldx + ci] : (unsigned short)0;
        }
      }
      u32x4 a;
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = (unsigned)av[2 * e] | ((unsigned)av[2 * e + 1] << 16);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        u32x4 b;
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = (unsigned)bv[t][2 * e] | ((unsigned)bv[t][2 * e + 1] << 16);
        acc[t] = mfma32(a, b, acc[t]);
      }
    }
  } else {
    const float* x = (const float*)xv;
    const float* dy = (const float*)dyv;
    for (int k0 = kb; k0 < ke; k0 += 4) {
      const int p = k0 + g;
      const bool ok = p < ke;
      const float a = (ok && qrow) ? dy[dy_pixel(p, hw, w, tap) * (size_t)lddy + co] : 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int ci = c0 + 16 * t + r;
        const float b = (ok && ci < cin) ? x[(size_t)p * ldx + ci] : 0.f;
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t], 0, 0, 0);
      }
    }
  }
  float* out = part + (size_t)blockIdx.z * ncol * cin;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int ci = c0 + 16 * t + r;
    if (ci >= cin) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int qq = blockIdx.x * 64 + wave * 16 + 4 * g + v;
      if (qq < ncol) out[(size_t)qq * cin + ci] = acc[t][v];
    }
  }
}

// dW[ci][co][i][j] (+)= sum over the splits, in split order
__global__ void convt2x2_wgrad_combine_kernel(const float* __restrict__ part, int splits, int cin, int cout, float* dw, int accumulate) {
  const int total = cin * cout * 4;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  const int tap = o & 3, rest = o >> 2, co = rest % cout, ci = rest / cout;
  const size_t src = (size_t)(tap * cout + co) * cin + ci, step = (size_t)4 * cout * cin;
  float s = 0.f;
  for (int z = 0; z < splits; ++z) s += part[z * step + src];
  dw[o] = accumulate ? dw[o] + s : s;
}

// the forward entry's packed weight (csrc/segment.hip: row q = tap * cout + co, kp = cin rounded up to the MFMA depth, zero filled)
// from the f32 master weight on the device: the weights change at every optimizer step
template <bool BF16>
__global__ void convt2x2_pack_kernel(const float* __restrict__ wt, int cin, int cout, int kp, void* __restrict__ out) {
  const long total = (long)4 * cout * kp;
  for (long o = blockIdx.x * 256L + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
    const int k = (int)(o % kp);
    const int q = (int)(o / kp), tap = q / cout, co = q - tap * cout;
    const float v = k < cin ? wt[((size_t)k * cout + co) * 4 + tap] : 0.f;
    if constexpr (BF16) ((bf16_t*)out)[o] = f32_to_bf16(v);
    else ((float*)out)[o] = v;
  }
}

int ctb_splits(int cin, int cout, long long npix, int kdepth, int* kc_out) {
  const int tiles = cdiv(4 * cout, 64) * cdiv(cin, 64);
  int cap = 512 / tiles;
  cap = cap < 1 ? 1 : cap > CTB_MAX_SPLITS ? CTB_MAX_SPLITS : cap;
  int splits = (int)((npix + 127) / 128);  // at least 128 pixels per split
  splits = splits < 1 ? 1 : splits > cap ? cap : splits;
  int kc = (int)((npix + splits - 1) / splits);
  kc = cdiv(kc, kdepth) * kdepth;
  splits = (int)((npix + kc - 1) / kc);
  if (kc_out) *kc_out = kc;
  return splits;
}

size_t ctb_reduce_bytes(int cout) { return (upa_channel_reduce_workspace_bytes(cout) + 255) / 256 * 256; }

// ---- mask loss -----------------------------------------------------------------------------------------------------------------------
constexpr int ML_NM = 128;     // coefficient depth limit (upa_process_mask's)
constexpr int ML_LEVELS = 3;
constexpr int ML_KQ = 4;       // lanes that share one pixel's dot product: lane q takes k = q, q + 4, ...
constexpr int ML_KPT = ML_NM / ML_KQ;  // k values per lane

struct MaskLevels {
  const void* coef[ML_LEVELS];
  void* dcoef[ML_LEVELS];
  int h[ML_LEVELS], w[ML_LEVELS], ld[ML_LEVELS], ldd[ML_LEVELS], a0[ML_LEVELS];
  int nl, A, B;
};

struct FgRec {        // one foreground anchor
  float x1, y1, x2, y2;  // its gt box in mask units
  float wgt;             // 1 / (mh * mw * area), area = the box's normalised w * h
  int mid;               // the value that marks its instance in the overlap mask
  int lvl;
  int anchor;            // index within the image's anchors
  long long off;         // element offset of its coefficient row within its level's map (the same pixel in the gradient map: offd)
  long long offd;
};

__device__ __forceinline__ void ml_decode(const MaskLevels& L, int a, int& lvl, int& pix) {
  lvl = 0;
#pragma unroll
  for (int l = 1; l < ML_LEVELS; ++l)
    if (l < L.nl && a >= L.a0[l]) lvl = l;
  pix = a - L.a0[lvl];
}

__device__ __forceinline__ int ml_gt_of(const int32_t* assign, int stride, const int* n_gt, int max_gt, int B_A_index, int b) {
  const int g = assign[(size_t)B_A_index * stride];
  const int ng = min(n_gt[b], max_gt);
  return (g >= 0 && g < ng) ? g : -1;
}

// 1. one workgroup per image: compact the foreground anchors in anchor order
__global__ __launch_bounds__(256) void ml_compact_kernel(const MaskLevels L, const int32_t* __restrict__ assign, int stride,
                                                         const float* __restrict__ gt, const int* __restrict__ n_gt, int max_gt,
                                                         const int32_t* __restrict__ mask_id, int mh, int mw, float imgh, float imgw,
                                                         FgRec* __restrict__ recs, int* __restrict__ nfg) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ int cnt[256];
  __shared__ int base;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int a0 = 0; a0 < L.A; a0 += 256) {
    const int a = a0 + tid;
    const int g = a < L.A ? ml_gt_of(assign, stride, n_gt, max_gt, b * L.A + a, b) : -1;
    cnt[tid] = g >= 0 ? 1 : 0;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive scan
      const int v = tid >= o ? cnt[tid - o] : 0;
      __syncthreads();
      cnt[tid] += v;
      __syncthreads();
    }
    if (g >= 0) {
      const int slot = base + cnt[tid] - 1;
      const float* gb = gt + ((size_t)b * max_gt + g) * 5;
      // loss.py:683-689: target_bboxes / imgsz[[1, 0, 1, 0]], area = w * h of that, * (mask_w, mask_h, mask_w, mask_h)
      const float nx1 = gb[1] / imgw, ny1 = gb[2] / imgh, nx2 = gb[3] / imgw, ny2 = gb[4] / imgh;
      const float area = (nx2 - nx1) * (ny2 - ny1);
      FgRec rc;
      rc.x1 = nx1 * (float)mw; rc.y1 = ny1 * (float)mh; rc.x2 = nx2 * (float)mw; rc.y2 = ny2 * (float)mh;
      rc.wgt = 1.0f / (float)(mh * mw) / area;
      rc.mid = mask_id[(size_t)b * max_gt + g];
      int lvl, pix;
      ml_decode(L, a, lvl, pix);
      rc.lvl = lvl;
      rc.anchor = a;
      rc.off = ((long long)b * L.h[lvl] * L.w[lvl] + pix) * L.ld[lvl];
      rc.offd = ((long long)b * L.h[lvl] * L.w[lvl] + pix) * L.ldd[lvl];
      recs[(size_t)b * L.A + slot] = rc;
    }
    __syncthreads();
    if (tid == 255) base += cnt[255];
    __syncthreads();
  }
  if (tid == 0) nfg[b] = base;
}

// 1b. zero rows of the coefficient-gradient maps for the anchors that are not foreground (16 bytes per thread)
template <typename T>
__global__ void ml_zero_bg_kernel(const MaskLevels L, const int32_t* __restrict__ assign, int stride, const int* __restrict__ n_gt, int max_gt,
                                  int nm) {
  constexpr int E = ElemTraits<T>::E;
  const int groups = nm / E;
  const long total = (long)L.B * L.A * groups;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int gq = (int)(i % groups);
    const long ba = i / groups;
    const int b = (int)(ba / L.A), a = (int)(ba - (long)b * L.A);
    if (ml_gt_of(assign, stride, n_gt, max_gt, (int)ba, b) >= 0) continue;
    int lvl, pix;
    ml_decode(L, a, lvl, pix);
    T* row = (T*)L.dcoef[lvl] + ((size_t)b * L.h[lvl] * L.w[lvl] + pix) * L.ldd[lvl];
    *reinterpret_cast<u32x4*>(row + gq * E) = u32x4{0u, 0u, 0u, 0u};
  }
}

__device__ __forceinline__ int ml_total_fg(const int* nfg, int B) {  // block-uniform: every thread sums the same B values in order
  int t = 0;
  for (int i = 0; i < B; ++i) t += nfg[i];
  return t;
}

__device__ __forceinline__ float ml_quad_sum(float v) {  // over the ML_KQ adjacent lanes of one pixel, one order for all of them
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v;
}

// 2. workgroups (slot lane, image): each walks the image's foreground slots lane, lane + gridDim.x, ... (the grid is sized by the
// most foreground anchors an image can have, not by its anchors): loss term and coefficient gradient of one foreground anchor per turn
template <typename T>
__global__ __launch_bounds__(256) void ml_anchor_kernel(const MaskLevels L, const T* __restrict__ proto, int mh, int mw, int nm, int ldp,
                                                        const uint8_t* __restrict__ masks, const FgRec* __restrict__ recs,
                                                        const int* __restrict__ nfg, float gscale, const float* gs_dev,
                                                        float* __restrict__ terms) {
  const int b = blockIdx.y;
  __shared__ float red[64][ML_NM + 1];
  __shared__ float lred[64];
  const int tid = threadIdx.x, pl = tid >> 2, kq = tid & 3;
  const int n_img = nfg[b];
  const int ntot = ml_total_fg(nfg, L.B);
  for (int slot = blockIdx.x; slot < n_img; slot += gridDim.x) {  // block-uniform
  const FgRec rc = recs[(size_t)b * L.A + slot];
  const T* crow = (const T*)L.coef[rc.lvl] + rc.off;
  float cf[ML_KPT], dc[ML_KPT];
#pragma unroll
  for (int i = 0; i < ML_KPT; ++i) {
    const int k = kq + ML_KQ * i;
    cf[i] = k < nm ? ElemTraits<T>::load(crow + k) : 0.f;
    dc[i] = 0.f;
  }
  // the integer pixels that can pass x >= x1 & x < x2 & y >= y1 & y < y2 (the float comparisons decide below)
  const int xlo = (int)fminf(floorf(fmaxf(rc.x1, 0.f)), (float)mw), xhi = (int)fminf(ceilf(fmaxf(rc.x2, 0.f)), (float)mw);
  const int ylo = (int)fminf(floorf(fmaxf(rc.y1, 0.f)), (float)mh), yhi = (int)fminf(ceilf(fmaxf(rc.y2, 0.f)), (float)mh);
  const int bw = max(xhi - xlo, 0), bh = max(yhi - ylo, 0);
  const int npx = bw * bh;
  float lsum = 0.f;
  for (int i0 = 0; i0 < npx; i0 += 64) {  // block-uniform trip count: the quad shuffles run converged
    const int idx = i0 + pl;
    const bool in = idx < npx;
    const int yy = in ? ylo + idx / bw : 0, xx = in ? xlo + idx - (idx / bw) * bw : 0;
    const bool keep = in && (float)xx >= rc.x1 && (float)xx < rc.x2 && (float)yy >= rc.y1 && (float)yy < rc.y2;
    const size_t pix = ((size_t)b * mh + yy) * mw + xx;
    const T* prow = proto + pix * ldp;
    float pv[ML_KPT];
    float part = 0.f;
#pragma unroll
    for (int i = 0; i < ML_KPT; ++i) {
      const int k = kq + ML_KQ * i;
      pv[i] = (keep && k < nm) ? ElemTraits<T>::load(prow + k) : 0.f;
      part += cf[i] * pv[i];
    }
    const float pred = ml_quad_sum(part);
    if (keep) {
      const float t = (int)masks[pix] == rc.mid ? 1.f : 0.f;
      // F.binary_cross_entropy_with_logits: max(x, 0) - x t + log(1 + exp(-|x|))
      if (kq == 0) lsum += fmaxf(pred, 0.f) - pred * t + log1pf(expf(-fabsf(pred)));
      const float dp = 1.0f / (1.0f + expf(-pred)) - t;
#pragma unroll
      for (int i = 0; i < ML_KPT; ++i) dc[i] += dp * pv[i];
    }
  }
#pragma unroll
  for (int i = 0; i < ML_KPT; ++i) {
    const int k = kq + ML_KQ * i;
    if (k < nm) red[pl][k] = dc[i];
  }
  if (kq == 0) lred[pl] = lsum;
  __syncthreads();
  float gs = gscale / (float)ntot * rc.wgt;
  if (gs_dev) gs *= *gs_dev;
  if (tid < nm) {
    float s = 0.f;
    for (int j = 0; j < 64; ++j) s += red[j][tid];
    T* drow = (T*)L.dcoef[rc.lvl] + rc.offd;
    const float v = s * gs;
    if constexpr (sizeof(T) == 2) drow[tid] = f32_to_bf16(v);
    else drow[tid] = v;
  }
  if (tid == 0) {
    float s = 0.f;
    for (int j = 0; j < 64; ++j) s += lred[j];
    terms[(size_t)b * L.A + slot] = s * rc.wgt;  // crop_mask(loss).mean((1, 2)) / area
  }
  __syncthreads();  // red / lred are rewritten by the next slot
  }
}

// 3. one workgroup per (64-pixel tile of 8 x 8, image): dproto
template <typename T>
__global__ __launch_bounds__(256) void ml_proto_kernel(const MaskLevels L, const T* __restrict__ proto, int mh, int mw, int nm, int ldp,
                                                       const uint8_t* __restrict__ masks, const FgRec* __restrict__ recs,
                                                       const int* __restrict__ nfg, float gscale, const float* gs_dev, T* __restrict__ dproto,
                                                       int lddp) {
  const int b = blockIdx.y;
  const int tw = (mw + 7) / 8;
  const int ty0 = (blockIdx.x / tw) * 8, tx0 = (blockIdx.x % tw) * 8;
  const int tid = threadIdx.x, pl = tid >> 2, kq = tid & 3;
  const int yy = ty0 + (pl >> 3), xx = tx0 + (pl & 7);
  const bool in = yy < mh && xx < mw;
  const size_t pix = ((size_t)b * mh + (in ? yy : 0)) * mw + (in ? xx : 0);
  const T* prow = proto + pix * ldp;
  float pv[ML_KPT], dp[ML_KPT];
#pragma unroll
  for (int i = 0; i < ML_KPT; ++i) {
    const int k = kq + ML_KQ * i;
    pv[i] = (in && k < nm) ? ElemTraits<T>::load(prow + k) : 0.f;
    dp[i] = 0.f;
  }
  const int mval = in ? (int)masks[pix] : -1;
  const int n = nfg[b];
  const int ntot = ml_total_fg(nfg, L.B);
  float gs = ntot > 0 ? gscale / (float)ntot : 0.f;
  if (gs_dev) gs *= *gs_dev;
  const FgRec* rp = recs + (size_t)b * L.A;
  for (int j = 0; j < n; ++j) {  // block-uniform loop and skip: the quad shuffles run converged
    const FgRec rc = rp[j];
    if (!((float)(tx0 + 7) >= rc.x1 && (float)tx0 < rc.x2 && (float)(ty0 + 7) >= rc.y1 && (float)ty0 < rc.y2)) continue;
    const T* crow = (const T*)L.coef[rc.lvl] + rc.off;
    float cf[ML_KPT];
    float part = 0.f;
#pragma unroll
    for (int i = 0; i < ML_KPT; ++i) {
      const int k = kq + ML_KQ * i;
      cf[i] = k < nm ? ElemTraits<T>::load(crow + k) : 0.f;
      part += cf[i] * pv[i];
    }
    const float pred = ml_quad_sum(part);
    const bool keep = in && (float)xx >= rc.x1 && (float)xx < rc.x2 && (float)yy >= rc.y1 && (float)yy < rc.y2;
    if (keep) {
      const float t = mval == rc.mid ? 1.f : 0.f;
      const float d = (1.0f / (1.0f + expf(-pred)) - t) * rc.wgt;
#pragma unroll
      for (int i = 0; i < ML_KPT; ++i) dp[i] += d * cf[i];
    }
  }
  if (!in) return;
  T* drow = dproto + pix * lddp;
#pragma unroll
  for (int i = 0; i < ML_KPT; ++i) {
    const int k = kq + ML_KQ * i;
    if (k >= nm) continue;
    const float v = dp[i] * gs;
    if constexpr (sizeof(T) == 2) drow[k] = f32_to_bf16(v);
    else drow[k] = v;
  }
}

// 4. the item: one workgroup, the terms in one fixed order
__global__ __launch_bounds__(256) void ml_finish_kernel(const float* __restrict__ terms, const int* __restrict__ nfg, int B, int A, float gain,
                                                        float* __restrict__ item) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  int ntot = 0;
  for (int b = 0; b < B; ++b) {
    const int n = nfg[b];
    ntot += n;
    for (int j = tid; j < n; j += 256) s += (double)terms[(size_t)b * A + j];
  }
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) item[0] = ntot > 0 ? (float)(red[0] / (double)ntot) * gain : 0.f;
}

struct MlWs {
  int* nfg;
  float* terms;
  FgRec* recs;
};

size_t ml_ws_layout(int b, int a, char* base, MlWs* out) {
  size_t off = 0;
  const size_t n_nfg = ((size_t)b * 4 + 255) / 256 * 256;
  const size_t n_terms = ((size_t)b * a * 4 + 255) / 256 * 256;
  if (out) { out->nfg = (int*)(base + off); }
  off += n_nfg;
  if (out) { out->terms = (float*)(base + off); }
  off += n_terms;
  if (out) { out->recs = (FgRec*)(base + off); }
  off += (size_t)b * a * sizeof(FgRec);
  return off;
}

}  // namespace

// ---- entry points --------------------------------------------------------------------------------------------------------------------

extern "C" int upa_pack_conv_transpose2x2_weight_dev(const float* w, int cin, int cout, int dtype, void* out, void* stream) {
  UPA_CHECK_ARG(w && out && cin > 0 && cout > 0 && cout <= (1 << 20) && cin <= (1 << 20), "pack_conv_transpose2x2_weight_dev: bad args");
  UPA_CHECK_ARG(dtype == UPA_F32 || dtype == UPA_BF16, "pack_conv_transpose2x2_weight_dev: dtype %d", dtype);
  const int kb = dtype == UPA_BF16 ? 32 : 4;  // the forward kernel's MFMA depths
  const int kp = cdiv(cin, kb) * kb;
  const long total = (long)4 * cout * kp;
  const int grid = (int)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256);
  if (dtype == UPA_BF16) hipLaunchKernelGGL(convt2x2_pack_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, cin, cout, kp, out);
  else hipLaunchKernelGGL(convt2x2_pack_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, cin, cout, kp, out);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" size_t upa_conv_transpose2x2_bwd_workspace_bytes(int cin, int cout) {
  if (cin <= 0 || cout <= 0) return 0;
  const int tiles = cdiv(4 * cout, 64) * cdiv(cin, 64);
  int cap = 512 / tiles;
  cap = cap < 1 ? 1 : cap > CTB_MAX_SPLITS ? CTB_MAX_SPLITS : cap;
  return ctb_reduce_bytes(cout) + (size_t)cap * 4 * cout * cin * sizeof(float);
}

extern "C" int upa_conv_transpose2x2_bwd(const void* x, int n, int h, int w, int cin, int ldx, const void* dy, int cout, int lddy,
                                         const float* weight, void* dx, int lddx, int accumulate_dx, float* dweight, float* dbias,
                                         int accumulate_w, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
  UPA_CHECK_ARG(x && dy && weight && dweight && dbias && workspace, "conv_transpose2x2_bwd: null pointer");
  UPA_CHECK_ARG(n > 0 && h > 0 && w > 0 && cin > 0 && cout > 0 && ldx >= cin && lddy >= cout && (!dx || lddx >= cin),
                "conv_transpose2x2_bwd: bad shape n=%d h=%d w=%d cin=%d ldx=%d cout=%d lddy=%d lddx=%d", n, h, w, cin, ldx, cout, lddy, lddx);
  if (dtype != UPA_F32 && dtype != UPA_BF16) {
    upa_set_error("conv_transpose2x2_bwd: dtype %d outside f32 | bf16", dtype);
    return UPA_EUNSUPPORTED;
  }
  const int es = upa_elem_size(dtype), vec = 16 / es;
  if (cin % vec || cout % vec || ldx % vec || lddy % vec || (dx && lddx % vec) || ((uintptr_t)x % 16) || ((uintptr_t)dy % 16) ||
      (dx && ((uintptr_t)dx % 16))) {
    upa_set_error("conv_transpose2x2_bwd: channel counts / strides must be multiples of 16 bytes (cin=%d cout=%d ldx=%d lddy=%d lddx=%d)",
                  cin, cout, ldx, lddy, lddx);
    return UPA_EUNSUPPORTED;
  }
  const long long npix = (long long)n * h * w;
  if (npix > 0x3fffffffll || npix * 4 * lddy > (1ll << 40) || cout > 1024) {
    upa_set_error("conv_transpose2x2_bwd: %lld pixels / %d channels", npix, cout);
    return UPA_EUNSUPPORTED;
  }
  UPA_CHECK_ARG(workspace_bytes >= upa_conv_transpose2x2_bwd_workspace_bytes(cin, cout), "conv_transpose2x2_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const bool bf = dtype == UPA_BF16;
  int kc = 0;
  const int splits = ctb_splits(cin, cout, npix, bf ? 32 : 4, &kc);
  float* part = (float*)((char*)workspace + ctb_reduce_bytes(cout));
  // bias gradient: the channel sums of dy over its 4 n h w pixels
  if (int rc = upa_channel_sum(dy, 4 * (long)npix, cout, lddy, dbias, accumulate_w, (double*)workspace, dtype, stream); rc != UPA_OK)
    return rc;
  const dim3 gw((unsigned)cdiv(4 * cout, 64), (unsigned)cdiv(cin, 64), (unsigned)splits);
  if (bf)
    hipLaunchKernelGGL(convt2x2_wgrad_kernel<true>, gw, dim3(256), 0, s, x, (int)npix, h, w, cin, ldx, dy, cout, lddy, kc, part);
  else
    hipLaunchKernelGGL(convt2x2_wgrad_kernel<false>, gw, dim3(256), 0, s, x, (int)npix, h, w, cin, ldx, dy, cout, lddy, kc, part);
  hipLaunchKernelGGL(convt2x2_wgrad_combine_kernel, dim3((unsigned)cdiv(4 * cin * cout, 256)), dim3(256), 0, s, part, splits, cin, cout,
                     dweight, accumulate_w);
  if (dx) {
    const dim3 gd((unsigned)cdiv((int)npix, 64), (unsigned)cdiv(cin, 64));
    if (bf)
      hipLaunchKernelGGL(convt2x2_dgrad_kernel<true>, gd, dim3(256), 0, s, dy, (int)npix, h, w, cout, lddy, weight, cin, dx, lddx,
                         accumulate_dx);
    else
      hipLaunchKernelGGL(convt2x2_dgrad_kernel<false>, gd, dim3(256), 0, s, dy, (int)npix, h, w, cout, lddy, weight, cin, dx, lddx,
                         accumulate_dx);
  }
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" size_t upa_mask_loss_workspace_bytes(int b, int n_anchors) {
  if (b <= 0 || n_anchors <= 0) return 0;
  return ml_ws_layout(b, n_anchors, nullptr, nullptr);
}

extern "C" int upa_mask_loss(const void* proto, int b, int mh, int mw, int nm, int ldp, const void* const* coefs, void* const* dcoefs,
                             const int* hs, const int* ws, const int* lds, const int* ldds, int n_levels, const int32_t* assign_gt,
                             int assign_stride, const float* gt, const int* n_gt, int max_gt, const int32_t* mask_id, const uint8_t* masks,
                             int imgsz_h, int imgsz_w, float gain, float grad_scale, const float* grad_scale_dev, float* loss_item,
                             void* dproto, int lddp, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
  UPA_CHECK_ARG(proto && coefs && dcoefs && hs && ws && lds && ldds && assign_gt && gt && n_gt && mask_id && masks && loss_item && dproto &&
                workspace, "mask_loss: null pointer");
  UPA_CHECK_ARG(b > 0 && mh > 0 && mw > 0 && nm > 0 && ldp >= nm && lddp >= nm && n_levels >= 1 && n_levels <= ML_LEVELS && max_gt >= 1 &&
                assign_stride >= 1 && imgsz_h > 0 && imgsz_w > 0,
                "mask_loss: bad shape b=%d mh=%d mw=%d nm=%d ldp=%d lddp=%d levels=%d max_gt=%d stride=%d", b, mh, mw, nm, ldp, lddp,
                n_levels, max_gt, assign_stride);
  if (dtype != UPA_F32 && dtype != UPA_BF16) {
    upa_set_error("mask_loss: dtype %d outside f32 | bf16", dtype);
    return UPA_EUNSUPPORTED;
  }
  const int vec = 16 / upa_elem_size(dtype);
  if (nm > ML_NM || nm % vec) {
    upa_set_error("mask_loss: nm = %d: at most %d coefficients, a multiple of 16 bytes", nm, ML_NM);
    return UPA_EUNSUPPORTED;
  }
  MaskLevels L{};
  L.nl = n_levels; L.B = b;
  long long a = 0;
  for (int l = 0; l < n_levels; ++l) {
    UPA_CHECK_ARG(coefs[l] && dcoefs[l] && hs[l] > 0 && ws[l] > 0 && lds[l] >= nm && ldds[l] >= nm, "mask_loss: level %d: bad view", l);
    if (ldds[l] % vec || ((uintptr_t)dcoefs[l] % 16)) {
      upa_set_error("mask_loss: level %d: the gradient map's stride / address must be multiples of 16 bytes", l);
      return UPA_EUNSUPPORTED;
    }
    L.coef[l] = coefs[l]; L.dcoef[l] = dcoefs[l]; L.h[l] = hs[l]; L.w[l] = ws[l]; L.ld[l] = lds[l]; L.ldd[l] = ldds[l];
    L.a0[l] = (int)a;
    a += (long long)hs[l] * ws[l];
  }
  if (a > 65535 || (long long)b * a > 0x3fffffffll || b > 65535 || (long long)b * mh * mw > 0x7fffffffll) {
    upa_set_error("mask_loss: %lld anchors x %d images x %d x %d mask pixels is past the kernels' index range", a, b, mh, mw);
    return UPA_EUNSUPPORTED;
  }
  L.A = (int)a;
  UPA_CHECK_ARG(workspace_bytes >= upa_mask_loss_workspace_bytes(b, L.A), "mask_loss: workspace too small");
  MlWs W;
  ml_ws_layout(b, L.A, (char*)workspace, &W);
  hipStream_t s = (hipStream_t)stream;
  const float gscale = gain * (float)b * grad_scale;
  hipLaunchKernelGGL(ml_compact_kernel, dim3(b), dim3(256), 0, s, L, assign_gt, assign_stride, gt, n_gt, max_gt, mask_id, mh, mw,
                     (float)imgsz_h, (float)imgsz_w, W.recs, W.nfg);
  const long zt = (long)b * L.A * (nm / vec);
  const int zgrid = (int)((zt + 255) / 256 > 2048 ? 2048 : (zt + 255) / 256);
  // an image has at most min(A, 10 max_gt) foreground anchors (the assigner's top 10 per gt); more than 512 slot lanes buy nothing
  const long long fg_cap = (long long)max_gt * 10;
  const int lanes = (int)(fg_cap < L.A ? fg_cap : L.A) < 512 ? (int)(fg_cap < L.A ? fg_cap : L.A) : 512;
  const dim3 ga((unsigned)lanes, (unsigned)b), gp((unsigned)(cdiv(mw, 8) * cdiv(mh, 8)), (unsigned)b);
  if (dtype == UPA_BF16) {
    hipLaunchKernelGGL(ml_zero_bg_kernel<bf16_t>, dim3(zgrid), dim3(256), 0, s, L, assign_gt, assign_stride, n_gt, max_gt, nm);
    hipLaunchKernelGGL(ml_anchor_kernel<bf16_t>, ga, dim3(256), 0, s, L, (const bf16_t*)proto, mh, mw, nm, ldp, masks, W.recs, W.nfg, gscale,
                       grad_scale_dev, W.terms);
    hipLaunchKernelGGL(ml_proto_kernel<bf16_t>, gp, dim3(256), 0, s, L, (const bf16_t*)proto, mh, mw, nm, ldp, masks, W.recs, W.nfg, gscale,
                       grad_scale_dev, (bf16_t*)dproto, lddp);
  } else {
    hipLaunchKernelGGL(ml_zero_bg_kernel<float>, dim3(zgrid), dim3(256), 0, s, L, assign_gt, assign_stride, n_gt, max_gt, nm);
    hipLaunchKernelGGL(ml_anchor_kernel<float>, ga, dim3(256), 0, s, L, (const float*)proto, mh, mw, nm, ldp, masks, W.recs, W.nfg, gscale,
                       grad_scale_dev, W.terms);
    hipLaunchKernelGGL(ml_proto_kernel<float>, gp, dim3(256), 0, s, L, (const float*)proto, mh, mw, nm, ldp, masks, W.recs, W.nfg, gscale,
                       grad_scale_dev, (float*)dproto, lddp);
  }
  hipLaunchKernelGGL(ml_finish_kernel, dim3(1), dim3(256), 0, s, W.terms, W.nfg, b, L.A, gain, loss_item);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}
