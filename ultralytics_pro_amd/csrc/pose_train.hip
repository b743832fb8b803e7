// Pose training: the keypoint terms of v8PoseLoss with their gradients (utils/loss.py:396-412 KeypointLoss, :791-870 kpts_decode +
// calculate_keypoints_loss) and the batched pad gather / scatter of the trainer's padded convs.
//
//  - upa_kpt_loss.  Four passes, no floating-point atomics:
//      1. per image: the foreground anchors compacted in anchor order into records (gt row, level, cell, row offsets);
//      2. rows of the other anchors of the gradient maps zeroed, 16 bytes per thread, over the full c columns;
//      3. per foreground anchor one wave, lane k = keypoint k: the location term (1 - exp(-e_k)) m_k and the visibility term
//         BCE-with-logits(v_k, m_k), each summed over the wave's lanes by a butterfly (one order); the gradient row goes through LDS and
//         is stored 16 bytes at a time over the full c columns (columns nk..c: zero);
//      4. the two items: the per-anchor terms summed in one fixed order, / (foreground count * nkpt), * gain.
//  - upa_pad_copy_batched.  A conv whose channels are no 16-byte multiple trains on zero-padded f32 copies of its parameters: one
//    launch copies every master tensor of a descriptor table into its padded copy (zeros in the pad, or zeros everywhere for a
//    gradient), one launch brings the real rows back (gradients added, running statistics copied).
#include "common.h"

namespace {

constexpr int KL_NK = 128;      // values per anchor (upa_kpt_decode_rows' limit)
constexpr int KL_NKPT = 64;     // keypoints: nk / ndim with ndim >= 2, one lane each
constexpr int KL_LEVELS = 3;

struct KptLevels {
  const void* kpt[KL_LEVELS];
  void* dkpt[KL_LEVELS];
  int h[KL_LEVELS], w[KL_LEVELS], ld[KL_LEVELS], ldd[KL_LEVELS], a0[KL_LEVELS];
  float stride[KL_LEVELS];
  int nl, A, B;
};

struct KptSigma {
  float s2[KL_NKPT];  // (2 sigma_k)^2
};

struct KptRec {       // one foreground anchor
  int g;              // its gt row
  int lvl;
  int cx, cy;         // its cell: anchor_points - 0.5 (loss.py:796-797)
  long long off;      // element offset of its row within its level's map (off) and within the gradient map (offd)
  long long offd;
};

__device__ __forceinline__ void kl_decode(const KptLevels& L, int a, int& lvl, int& pix) {
  lvl = 0;
#pragma unroll
  for (int l = 1; l < KL_LEVELS; ++l)
    if (l < L.nl && a >= L.a0[l]) lvl = l;
  pix = a - L.a0[lvl];
}

__device__ __forceinline__ int kl_gt_of(const int32_t* assign, int stride, const int* n_gt, int max_gt, long ba, int b) {
  const int g = assign[(size_t)ba * stride];
  const int ng = min(n_gt[b], max_gt);
  return (g >= 0 && g < ng) ? g : -1;
}

// 1. one workgroup per image: compact the foreground anchors in anchor order
__global__ __launch_bounds__(256) void kl_compact_kernel(const KptLevels L, const int32_t* __restrict__ assign, int stride,
                                                         const int* __restrict__ n_gt, int max_gt, KptRec* __restrict__ recs,
                                                         int* __restrict__ nfg) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ int cnt[256];
  __shared__ int base;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int a0 = 0; a0 < L.A; a0 += 256) {
    const int a = a0 + tid;
    const int g = a < L.A ? kl_gt_of(assign, stride, n_gt, max_gt, (long)b * L.A + a, b) : -1;
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
      int lvl, pix;
      kl_decode(L, a, lvl, pix);
      KptRec rc;
      rc.g = g;
      rc.lvl = lvl;
      rc.cy = pix / L.w[lvl];
      rc.cx = pix - rc.cy * L.w[lvl];
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

// 2. zero the gradient rows of the anchors that are not foreground, over the full c columns (16 bytes per thread)
template <typename T>
__global__ void kl_zero_bg_kernel(const KptLevels L, const int32_t* __restrict__ assign, int stride, const int* __restrict__ n_gt, int max_gt,
                                  int c) {
  constexpr int E = ElemTraits<T>::E;
  const int groups = c / E;
  const long total = (long)L.B * L.A * groups;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int gq = (int)(i % groups);
    const long ba = i / groups;
    const int b = (int)(ba / L.A), a = (int)(ba - (long)b * L.A);
    if (kl_gt_of(assign, stride, n_gt, max_gt, ba, b) >= 0) continue;
    int lvl, pix;
    kl_decode(L, a, lvl, pix);
    T* row = (T*)L.dkpt[lvl] + ((size_t)b * L.h[lvl] * L.w[lvl] + pix) * L.ldd[lvl];
    *reinterpret_cast<u32x4*>(row + gq * E) = u32x4{0u, 0u, 0u, 0u};
  }
}

__device__ __forceinline__ float kl_wave_sum(float v) {  // over the 64 lanes, one order for all of them
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// 3. workgroups (slot group, image) of 4 waves: wave w takes the image's foreground slots s0 + w for s0 = 4 blockIdx.x, + 4 gridDim.x, ...
// (the grid is sized by the most foreground anchors an image can have, not by its anchors); lane k = keypoint k
template <typename T, int NDIM>
__global__ __launch_bounds__(256) void kl_anchor_kernel(const KptLevels L, const KptSigma S, int nkpt, int c, const float* __restrict__ gt,
                                                        int max_gt, const float* __restrict__ gt_kpt, const KptRec* __restrict__ recs,
                                                        const int* __restrict__ nfg, float gpose, float gkobj, const float* gs_dev,
                                                        float* __restrict__ tpose, float* __restrict__ tkobj) {
  constexpr int E = ElemTraits<T>::E;
  const int b = blockIdx.y;
  __shared__ float row[4][KL_NK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_img = nfg[b];
  int ntot = 0;
  for (int i = 0; i < L.B; ++i) ntot += nfg[i];
  float gs = 1.0f / ((float)ntot * (float)nkpt);
  if (gs_dev) gs *= *gs_dev;
  const int nk = nkpt * NDIM;
  for (int s0 = blockIdx.x * 4; s0 < n_img; s0 += gridDim.x * 4) {  // block-uniform
    const int slot = s0 + wave;
    const bool live = slot < n_img;  // wave-uniform
    KptRec rc{};
    if (live) rc = recs[(size_t)b * L.A + slot];
    const bool on = live && lane < nkpt;
    float gx_ = 0.f, gy_ = 0.f, dv = 0.f;
    float tp = 0.f, tk = 0.f, m = 0.f;
    float ex = 0.f, dxp = 0.f, dyp = 0.f, denom = 1.f;
    if (on) {
      const float st = L.stride[rc.lvl];
      const T* src = (const T*)L.kpt[rc.lvl] + rc.off + lane * NDIM;
      const float vx = ElemTraits<T>::load(src), vy = ElemTraits<T>::load(src + 1);
      const float* gk = gt_kpt + (((size_t)b * max_gt + rc.g) * nkpt + lane) * 3;
      const float* gb = gt + ((size_t)b * max_gt + rc.g) * 5;
      // loss.py:771 target_bboxes /= stride, :862 the product of its width and height
      const float area = (gb[3] / st - gb[1] / st) * (gb[4] / st - gb[2] / st);
      m = NDIM == 3 ? (gk[2] != 0.f ? 1.f : 0.f) : 1.f;
      dxp = (vx * 2.0f + (float)rc.cx) - gk[0] / st;
      dyp = (vy * 2.0f + (float)rc.cy) - gk[1] / st;
      const float d = dxp * dxp + dyp * dyp;
      denom = S.s2[lane] * (area + 1e-9f) * 2.0f;
      ex = expf(-(d / denom));
      tp = (1.0f - ex) * m;
      if constexpr (NDIM == 3) {
        const float v = ElemTraits<T>::load(src + 2);
        // F.binary_cross_entropy_with_logits: max(x, 0) - x t + log(1 + exp(-|x|))
        tk = fmaxf(v, 0.f) - v * m + log1pf(expf(-fabsf(v)));
        dv = 1.0f / (1.0f + expf(-v)) - m;
      }
    }
    const float msum = kl_wave_sum(m);
    const float factor = (float)nkpt / (msum + 1e-9f);
    const float psum = kl_wave_sum(tp);
    const float ksum = kl_wave_sum(tk);
    if (on) {
      // d/dv of factor (1 - exp(-e)) m with e = ((2 v + cell - g)^2 + ...) / denom: factor m exp(-e) 4 (2 v + cell - g) / denom.
      // exp(-e) may be a subnormal: it meets the coefficient once, as the last factor but the difference
      const float k = (gpose * gs * factor * 4.0f / denom) * (ex * m);
      gx_ = k * dxp;
      gy_ = k * dyp;
      row[wave][lane * NDIM] = gx_;
      row[wave][lane * NDIM + 1] = gy_;
      if constexpr (NDIM == 3) row[wave][lane * NDIM + 2] = gkobj * gs * dv;
    }
    if (live && lane == 0) {
      tpose[(size_t)b * L.A + slot] = factor * psum;
      tkobj[(size_t)b * L.A + slot] = ksum;
    }
    __syncthreads();
    if (live) {
      T* drow = (T*)L.dkpt[rc.lvl] + rc.offd;
      for (int gq = lane; gq < c / E; gq += 64) {
        float v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int col = gq * E + e;
          v[e] = col < nk ? row[wave][col] : 0.f;
        }
        u32x4 o;
        if constexpr (sizeof(T) == 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = __float_as_uint(v[e]);
        }
        *reinterpret_cast<u32x4*>(drow + gq * E) = o;
      }
    }
    __syncthreads();  // row is rewritten by the next turn
  }
}

// 4. the items: one workgroup, the terms in one fixed order
__global__ __launch_bounds__(256) void kl_finish_kernel(const float* __restrict__ tpose, const float* __restrict__ tkobj,
                                                        const int* __restrict__ nfg, int B, int A, int nkpt, int ndim, float gain_pose,
                                                        float gain_kobj, float* __restrict__ items) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  double sp = 0.0, sk = 0.0;
  int ntot = 0;
  for (int b = 0; b < B; ++b) {
    const int n = nfg[b];
    ntot += n;
    for (int j = tid; j < n; j += 256) {
      sp += (double)tpose[(size_t)b * A + j];
      sk += (double)tkobj[(size_t)b * A + j];
    }
  }
  red[0][tid] = sp;
  red[1][tid] = sk;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o];
      red[1][tid] += red[1][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double den = (double)ntot * (double)nkpt;
    items[0] = ntot > 0 ? (float)(red[0][0] / den) * gain_pose : 0.f;
    items[1] = (ntot > 0 && ndim == 3) ? (float)(red[1][0] / den) * gain_kobj : 0.f;
  }
}

struct KlWs {
  int* nfg;
  float* tpose;
  float* tkobj;
  KptRec* recs;
};

size_t kl_ws_layout(int b, int a, char* base, KlWs* out) {
  size_t off = 0;
  const size_t n_nfg = ((size_t)b * 4 + 255) / 256 * 256;
  const size_t n_terms = ((size_t)b * a * 4 + 255) / 256 * 256;
  if (out) out->nfg = (int*)(base + off);
  off += n_nfg;
  if (out) out->tpose = (float*)(base + off);
  off += n_terms;
  if (out) out->tkobj = (float*)(base + off);
  off += n_terms;
  if (out) out->recs = (KptRec*)(base + off);
  off += (size_t)b * a * sizeof(KptRec);
  return off;
}

// ---- pad gather / scatter -------------------------------------------------------------------------------------------------------------
// workgroups (part, descriptor): padded[r][c][i] = master[r][c][i] inside (rows, cols), 0 in the pad (or everywhere: a gradient)
__global__ __launch_bounds__(256) void pad_gather_kernel(const UpaPadDesc* __restrict__ descs) {
  const UpaPadDesc d = descs[blockIdx.y];
  const long total = (long)d.prows * d.pcols * d.inner;
  const bool copy = (d.flags & UPA_PAD_GATHER) != 0;
  for (long o = blockIdx.x * 256L + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
    const int i = (int)(o % d.inner);
    const long rc = o / d.inner;
    const int c = (int)(rc % d.pcols), r = (int)(rc / d.pcols);
    d.padded[o] = (copy && r < d.rows && c < d.cols) ? d.master[((size_t)r * d.cols + c) * d.inner + i] : 0.f;
  }
}

// master[r][c][i] (+)= padded[r][c][i]
__global__ __launch_bounds__(256) void pad_scatter_kernel(const UpaPadDesc* __restrict__ descs) {
  const UpaPadDesc d = descs[blockIdx.y];
  if (!(d.flags & (UPA_PAD_SCATTER_COPY | UPA_PAD_SCATTER_ADD))) return;
  const bool add = (d.flags & UPA_PAD_SCATTER_ADD) != 0;
  const long total = (long)d.rows * d.cols * d.inner;
  for (long o = blockIdx.x * 256L + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
    const int i = (int)(o % d.inner);
    const long rc = o / d.inner;
    const int c = (int)(rc % d.cols), r = (int)(rc / d.cols);
    const float v = d.padded[((size_t)r * d.pcols + c) * d.inner + i];
    d.master[o] = add ? d.master[o] + v : v;
  }
}

}  // namespace

// ---- entry points --------------------------------------------------------------------------------------------------------------------

extern "C" int upa_pad_copy_batched(const UpaPadDesc* descs_dev, int n, int scatter, void* stream) {
  UPA_CHECK_ARG(descs_dev && n > 0 && n <= 65535, "pad_copy_batched: bad args (n=%d)", n);
  const dim3 grid(16, (unsigned)n);
  if (scatter) hipLaunchKernelGGL(pad_scatter_kernel, grid, dim3(256), 0, (hipStream_t)stream, descs_dev);
  else hipLaunchKernelGGL(pad_gather_kernel, grid, dim3(256), 0, (hipStream_t)stream, descs_dev);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" size_t upa_kpt_loss_workspace_bytes(int b, int n_anchors) {
  if (b <= 0 || n_anchors <= 0) return 0;
  return kl_ws_layout(b, n_anchors, nullptr, nullptr);
}

extern "C" int upa_kpt_loss(const void* const* kpts, void* const* dkpts, const int* hs, const int* ws, const int* lds, const int* ldds,
                            int n_levels, int b, int c, int nkpt, int ndim, const int32_t* assign_gt, int assign_stride, const float* gt,
                            const int* n_gt, int max_gt, const float* gt_kpt, const float* strides, const float* sigma, float gain_pose,
                            float gain_kobj, float grad_scale, const float* grad_scale_dev, float* loss_items, void* workspace,
                            size_t workspace_bytes, int dtype, void* stream) {
  UPA_CHECK_ARG(kpts && dkpts && hs && ws && lds && ldds && assign_gt && gt && n_gt && gt_kpt && strides && sigma && loss_items && workspace,
                "kpt_loss: null pointer");
  UPA_CHECK_ARG(b > 0 && c > 0 && nkpt > 0 && n_levels >= 1 && n_levels <= KL_LEVELS && max_gt >= 1 && assign_stride >= 1,
                "kpt_loss: bad shape b=%d c=%d nkpt=%d levels=%d max_gt=%d stride=%d", b, c, nkpt, n_levels, max_gt, assign_stride);
  if (ndim != 2 && ndim != 3) {
    upa_set_error("kpt_loss: ndim = %d: a keypoint is (x, y) or (x, y, visibility)", ndim);
    return UPA_EUNSUPPORTED;
  }
  const long long nk = (long long)nkpt * ndim;
  if (nk > KL_NK) {
    upa_set_error("kpt_loss: %lld keypoint values per anchor, at most %d", nk, KL_NK);
    return UPA_EUNSUPPORTED;
  }
  if (dtype != UPA_F32 && dtype != UPA_BF16) {
    upa_set_error("kpt_loss: dtype %d outside f32 | bf16", dtype);
    return UPA_EUNSUPPORTED;
  }
  UPA_CHECK_ARG(c >= (int)nk, "kpt_loss: c = %d channels hold no %lld keypoint values", c, nk);
  const int vec = 16 / upa_elem_size(dtype);
  if (c % vec) {
    upa_set_error("kpt_loss: c = %d: the gradient rows are written 16 bytes at a time", c);
    return UPA_EUNSUPPORTED;
  }
  KptLevels L{};
  L.nl = n_levels; L.B = b;
  long long a = 0;
  for (int l = 0; l < n_levels; ++l) {
    UPA_CHECK_ARG(kpts[l] && dkpts[l] && hs[l] > 0 && ws[l] > 0 && lds[l] >= c && ldds[l] >= c && strides[l] > 0.f,
                  "kpt_loss: level %d: bad view", l);
    if (ldds[l] % vec || ((uintptr_t)dkpts[l] % 16)) {
      upa_set_error("kpt_loss: level %d: the gradient map's stride / address must be multiples of 16 bytes", l);
      return UPA_EUNSUPPORTED;
    }
    L.kpt[l] = kpts[l]; L.dkpt[l] = dkpts[l]; L.h[l] = hs[l]; L.w[l] = ws[l]; L.ld[l] = lds[l]; L.ldd[l] = ldds[l];
    L.stride[l] = strides[l];
    L.a0[l] = (int)a;
    a += (long long)hs[l] * ws[l];
  }
  if (a > 65535 || (long long)b * a > 0x3fffffffll || b > 65535) {
    upa_set_error("kpt_loss: %lld anchors x %d images is past the kernels' index range", a, b);
    return UPA_EUNSUPPORTED;
  }
  L.A = (int)a;
  UPA_CHECK_ARG(workspace_bytes >= upa_kpt_loss_workspace_bytes(b, L.A), "kpt_loss: workspace too small");
  KptSigma S{};
  for (int k = 0; k < nkpt; ++k) {
    const float s2 = 2.0f * sigma[k];
    S.s2[k] = s2 * s2;
  }
  KlWs W;
  kl_ws_layout(b, L.A, (char*)workspace, &W);
  hipStream_t s = (hipStream_t)stream;
  const float gpose = gain_pose * (float)b * grad_scale, gkobj = gain_kobj * (float)b * grad_scale;
  hipLaunchKernelGGL(kl_compact_kernel, dim3(b), dim3(256), 0, s, L, assign_gt, assign_stride, n_gt, max_gt, W.recs, W.nfg);
  const long zt = (long)b * L.A * (c / vec);
  const int zgrid = (int)((zt + 255) / 256 > 2048 ? 2048 : (zt + 255) / 256);
  // an image has at most min(A, 10 max_gt) foreground anchors (the assigner's top 10 per gt), four per workgroup; more than 128
  // workgroups per image buy nothing
  const long long fg_cap = (long long)max_gt * 10 < L.A ? (long long)max_gt * 10 : L.A;
  const int groups = (int)((fg_cap + 3) / 4 < 128 ? (fg_cap + 3) / 4 : 128);
  const dim3 ga((unsigned)groups, (unsigned)b);
#define UPA_KL_LAUNCH(T, ND)                                                                                                            \
  hipLaunchKernelGGL((kl_anchor_kernel<T, ND>), ga, dim3(256), 0, s, L, S, nkpt, c, gt, max_gt, gt_kpt, W.recs, W.nfg, gpose, gkobj, \
                     grad_scale_dev, W.tpose, W.tkobj)
  if (dtype == UPA_BF16) {
    hipLaunchKernelGGL(kl_zero_bg_kernel<bf16_t>, dim3(zgrid), dim3(256), 0, s, L, assign_gt, assign_stride, n_gt, max_gt, c);
    if (ndim == 3) UPA_KL_LAUNCH(bf16_t, 3);
    else UPA_KL_LAUNCH(bf16_t, 2);
  } else {
    hipLaunchKernelGGL(kl_zero_bg_kernel<float>, dim3(zgrid), dim3(256), 0, s, L, assign_gt, assign_stride, n_gt, max_gt, c);
    if (ndim == 3) UPA_KL_LAUNCH(float, 3);
    else UPA_KL_LAUNCH(float, 2);
  }
#undef UPA_KL_LAUNCH
  hipLaunchKernelGGL(kl_finish_kernel, dim3(1), dim3(256), 0, s, W.tpose, W.tkobj, W.nfg, b, L.A, nkpt, ndim, gain_pose, gain_kobj,
                     loss_items);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}
