// Pose estimation: keypoint decode, keypoint rescaling and OKS matching (ultralytics/nn/modules/head.py:1264-1273 Pose.kpts_decode;
// utils/ops.py scale_coords + clip_coords; models/yolo/pose/val.py:169-197 PoseValidator._process_batch; utils/metrics.py:164-184
// kpt_iou; engine/validator.py:267-308 match_predictions).  All three are bandwidth-bound, no matrix cores.
//
//  - upa_kpt_decode_rows: one workgroup per 64 pixels of one image.  A pixel's nk channels are contiguous (NHWC) and an output row's
//    anchors are contiguous ((n, nk, A) f32), so the tile passes through LDS: 16-byte loads along the channels, 16-byte stores along
//    the anchors (narrower ones where a pointer, a stride or the tile edge does not allow them).
//  - upa_scale_coords: one thread per (row, keypoint), rows past counts untouched.
//  - upa_pose_match: one workgroup per image, the shape of upa_match_predictions: the image's label keypoints, areas and visibility
//    counts are staged in LDS once, every detection walks the labels of its class (sums over the keypoints in ascending order: a
//    replay is bit-identical), then the claim step of match_claim.h.
#include "common.h"
#include "match_claim.h"

namespace {

constexpr int KD_TILE = 64;     // pixels per workgroup
constexpr int KD_PITCH = 65;    // LDS row pitch in floats: the channel-major tile is written down columns and read along rows
constexpr int KD_MAX_NK = 128;  // keypoint values per anchor: 128 x 65 floats = 33 KB of LDS
constexpr int PM_MAX_KPT = 64;  // keypoints per instance: sigma travels by value

struct KDArgs {
  const void* x;
  int hw, w, c, ldx, nk, ndim, vec_in, vec_out;
  float stride_px;
  float* out;
  float* raw;
  long a_total;
  int a0;
};

template <typename T>
__device__ __forceinline__ float kd_decode(float v, int d, int gx, int gy, float stride_px) {
  if (d == 0) return (v * 2.0f + (float)gx) * stride_px;  // (v * 2 + (anchor - 0.5)) * stride: anchor - 0.5 is the integer cell index
  if (d == 1) return (v * 2.0f + (float)gy) * stride_px;
  // the device sigmoid of upa_detect_decode (detect.hip): v_exp_f32 / v_rcp_f32 on bf16 logits, ocml expf + IEEE divide on f32
  return sizeof(T) == 2 ? __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.44269504088896340736f)) : 1.0f / (1.0f + expf(-v));
}

template <typename T>
__global__ __launch_bounds__(256) void kpt_decode_kernel(KDArgs A) {
  constexpr int E = ElemTraits<T>::E;
  __shared__ float s[KD_MAX_NK * KD_PITCH];
  const int tid = threadIdx.x, img = blockIdx.y;
  const int p0 = blockIdx.x * KD_TILE;
  const int np = min(KD_TILE, A.hw - p0);  // pixels of this tile
  const T* X = (const T*)A.x + ((size_t)img * A.hw + p0) * A.ldx;
  // ---- channels -> LDS [channel][pixel].  Whole 16-byte groups that lie inside the view's c channels move as vectors
  const int ngf = A.vec_in ? min(A.nk, A.c) / E : 0;
  for (int i = tid; i < np * ngf; i += 256) {
    const int p = i / ngf, g = i - p * ngf;
    const u32x4 v = *reinterpret_cast<const u32x4*>(X + (size_t)p * A.ldx + g * E);
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[(g * 8 + 2 * e) * KD_PITCH + p] = __uint_as_float(v[e] << 16);
        s[(g * 8 + 2 * e + 1) * KD_PITCH + p] = __uint_as_float(v[e] & 0xffff0000u);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) s[(g * 4 + e) * KD_PITCH + p] = __uint_as_float(v[e]);
    }
  }
  const int c_rest = ngf * E, n_rest = A.nk - c_rest;
  for (int i = tid; i < np * n_rest; i += 256) {
    const int p = i / n_rest, ch = c_rest + (i - p * n_rest);
    s[ch * KD_PITCH + p] = ElemTraits<T>::load(X + (size_t)p * A.ldx + ch);
  }
  __syncthreads();
  // ---- LDS -> rows of the (n, nk, a_total) outputs: 16 quads of anchors per channel row
  float* O = A.out + (size_t)img * A.nk * A.a_total + A.a0 + p0;
  float* Rw = A.raw ? A.raw + (size_t)img * A.nk * A.a_total + A.a0 + p0 : nullptr;
  for (int i = tid; i < A.nk * (KD_TILE / 4); i += 256) {
    const int j = i >> 4, q = (i & 15) * 4;
    if (q >= np) continue;
    const int d = j % A.ndim;
    float v[4], y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int pp = p0 + q + e;  // pixel index in the image (past the tile edge: LDS holds stale values, never stored)
      v[e] = s[j * KD_PITCH + q + e];
      const int gy = pp / A.w;
      y[e] = kd_decode<T>(v[e], d, pp - gy * A.w, gy, A.stride_px);
    }
    const size_t o = (size_t)j * A.a_total + q;
    if (A.vec_out && q + 4 <= np) {
      *reinterpret_cast<f32x4*>(O + o) = f32x4{y[0], y[1], y[2], y[3]};
      if (Rw) *reinterpret_cast<f32x4*>(Rw + o) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
      for (int e = 0; e < 4 && q + e < np; ++e) {
        O[o + e] = y[e];
        if (Rw) Rw[o + e] = v[e];
      }
    }
  }
}

// ---- scale_coords -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scale_coords_kernel(float* rows, long total, int max_det, int rs, int col0, int nkpt, int ndim,
                                                           const int32_t* __restrict__ counts, float gain, float px, float py, int padding,
                                                           float w0, float h0) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= total) return;
  const long row = i / nkpt;
  const int k = (int)(i - row * nkpt);
  if (counts) {
    const long img = row / max_det;
    if ((int)(row - img * max_det) >= counts[img]) return;
  }
  float* p = rows + row * rs + col0 + k * ndim;
  float x = p[0], y = p[1];
  if (padding) {
    x -= px;
    y -= py;
  }
  x /= gain;
  y /= gain;
  p[0] = fminf(fmaxf(x, 0.f), w0);  // clip_coords (utils/ops.py:180-201)
  p[1] = fminf(fmaxf(y, 0.f), h0);
}

// ---- OKS + match_predictions ----------------------------------------------------------------------------------------------------------
struct PoseSigma {
  float s2[PM_MAX_KPT];  // (2 sigma)^2
};

// LDS of one image: s_min [max_gt][MP_NT] ints | label keypoints [max_gt][nkpt][3] | per label: class, area + eps, visible count + eps
__global__ __launch_bounds__(256) void pose_match_kernel(const float* __restrict__ rows, int ld, int max_det, const int32_t* __restrict__ counts,
                                                         const float* __restrict__ gt, const int32_t* __restrict__ ngt, int max_gt,
                                                         const float* __restrict__ gt_kpt, int nkpt, int ndim, PoseSigma sg, MatchThr thr,
                                                         float eps, unsigned char* __restrict__ tp, float* __restrict__ oks_out) {
  extern __shared__ int s_min[];
  float* s_k = reinterpret_cast<float*>(s_min + max_gt * MP_NT);
  float* s_l = s_k + max_gt * nkpt * 3;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = max(min(counts[b], max_det), 0), M = max(min(ngt[b], max_gt), 0);
  for (int i = tid; i < M * MP_NT; i += 256) s_min[i] = 0x7fffffff;
  const float* GK = gt_kpt + (size_t)b * max_gt * nkpt * 3;
  for (int i = tid; i < M * nkpt * 3; i += 256) s_k[i] = GK[i];
  const float* G = gt + (size_t)b * max_gt * 5;
  for (int l = tid; l < M; l += 256) {
    // area = xyxy2xywh(bboxes)[:, 2:].prod(1) * 0.53 (pose/val.py:193)
    const float area = ((G[l * 5 + 3] - G[l * 5 + 1]) * (G[l * 5 + 4] - G[l * 5 + 2])) * 0.53f;
    int vis = 0;
    for (int k = 0; k < nkpt; ++k) vis += GK[(l * nkpt + k) * 3 + 2] != 0.f;  // kpt_mask = kpt1[..., 2] != 0
    s_l[l * 3] = G[l * 5];
    s_l[l * 3 + 1] = area + eps;
    s_l[l * 3 + 2] = (float)vis + eps;
  }
  __syncthreads();
  unsigned char* T = tp + (size_t)b * max_det * MP_NT;
  for (int base = 0; base < max_det; base += 256) {
    const int d = base + tid;
    int bl = -1;
    float bi = -1.f;
    float* orow = (oks_out && d < max_det) ? oks_out + ((size_t)b * max_det + d) * max_gt : nullptr;
    if (d < N) {
      const float* r = rows + ((size_t)b * max_det + d) * ld;
      const float cls = r[5];
      const float* pk = r + 6;
      for (int l = 0; l < M; ++l) {
        float oks = 0.f;
        if (s_l[l * 3] == cls) {
          const float ae = s_l[l * 3 + 1];
          const float* gk = s_k + l * nkpt * 3;
          float sum = 0.f;
          for (int k = 0; k < nkpt; ++k) {
            const float dx = gk[k * 3] - pk[k * ndim], dy = gk[k * 3 + 1] - pk[k * ndim + 1];
            const float dd = dx * dx + dy * dy;
            const float e = dd / ((sg.s2[k] * ae) * 2.0f);  // d / ((2 sigma)^2 (area + eps) 2), metrics.py:182
            const float t = expf(-e);
            sum += gk[k * 3 + 2] != 0.f ? t : 0.f * t;  // exp(-e) * mask: an invisible keypoint still spreads a NaN, as the product does
          }
          oks = sum / s_l[l * 3 + 2];
          if (oks >= bi) { bi = oks; bl = l; }  // ties: the larger label index, as upa_match_predictions
        }
        if (orow) orow[l] = oks;
      }
      if (orow)
        for (int l = M; l < max_gt; ++l) orow[l] = 0.f;
    } else if (orow) {
      for (int l = 0; l < max_gt; ++l) orow[l] = 0.f;
    }
    match_claim_round(s_min, d, N, max_det, bl, bi, thr, T);
  }
}

}  // namespace

// ---- entry points ------------------------------------------------------------------------------------------------------------------

extern "C" int upa_kpt_decode_rows(const void* x, int n, int h, int w, int c, int ldx, int dtype, int nkpt, int ndim, float stride_px,
                                   float* out, int a_total, int a0, float* raw, void* stream) {
  UPA_CHECK_ARG(x && out, "kpt_decode_rows: null pointer");
  UPA_CHECK_ARG(n > 0 && h > 0 && w > 0 && nkpt > 0 && ndim > 0 && c > 0 && ldx >= c && a0 >= 0 && (long long)h * w <= 0x7fffffc0ll &&
                    (long long)a0 + (long long)h * w <= a_total && n <= 65535,
                "kpt_decode_rows: bad shape n=%d h=%d w=%d c=%d ldx=%d nkpt=%d ndim=%d a0=%d a_total=%d", n, h, w, c, ldx, nkpt, ndim, a0,
                a_total);
  const long long nk = (long long)nkpt * ndim;
  if ((dtype != UPA_F32 && dtype != UPA_BF16) || (ndim != 2 && ndim != 3) || nk > KD_MAX_NK) {
    upa_set_error("kpt_decode_rows: dtype %d ndim %d nk %lld outside the supported form (f32 | bf16, ndim 2 | 3, nkpt * ndim <= %d)", dtype,
                  ndim, nk, KD_MAX_NK);
    return UPA_EUNSUPPORTED;
  }
  UPA_CHECK_ARG(nk <= c, "kpt_decode_rows: %lld keypoint values in a %d-channel view", nk, c);
  const int E = 16 / upa_elem_size(dtype);
  KDArgs A;
  A.x = x, A.hw = h * w, A.w = w, A.c = c, A.ldx = ldx, A.nk = (int)nk, A.ndim = ndim, A.stride_px = stride_px;
  A.out = out, A.raw = raw, A.a_total = a_total, A.a0 = a0;
  A.vec_in = ((uintptr_t)x % 16) == 0 && ldx % E == 0;
  A.vec_out = a_total % 4 == 0 && a0 % 4 == 0 && ((uintptr_t)out % 16) == 0 && (!raw || ((uintptr_t)raw % 16) == 0);
  const dim3 grid((unsigned)cdiv(A.hw, KD_TILE), (unsigned)n);
  if (dtype == UPA_BF16) hipLaunchKernelGGL(kpt_decode_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL(kpt_decode_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, A);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_scale_coords(float* rows, int b, int max_det, int row_stride, int col0, int nkpt, int ndim, const int32_t* counts,
                                float gain, float pad_x, float pad_y, int padding, float w0, float h0, void* stream) {
  UPA_CHECK_ARG(rows, "scale_coords: null pointer");
  UPA_CHECK_ARG(b >= 0 && max_det >= 0 && nkpt > 0 && ndim >= 2 && col0 >= 0 && (long long)col0 + (long long)nkpt * ndim <= row_stride &&
                    gain > 0.f,
                "scale_coords: bad shape b=%d max_det=%d row_stride=%d col0=%d nkpt=%d ndim=%d gain=%g", b, max_det, row_stride, col0, nkpt,
                ndim, (double)gain);
  const long total = (long)b * max_det * nkpt;
  if (total == 0) return UPA_OK;
  UPA_CHECK_ARG((total + 255) / 256 <= 0x7fffffffl, "scale_coords: %ld keypoints", total);
  hipLaunchKernelGGL(scale_coords_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, total, max_det,
                     row_stride, col0, nkpt, ndim, counts, gain, pad_x, pad_y, padding, w0, h0);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_pose_match(const float* rows, int ld, int b, int max_det, const int32_t* counts, const float* gt, const int32_t* ngt,
                              int max_gt, const float* gt_kpt, int nkpt, int ndim, const float* sigma, const float* iou_thresholds,
                              int n_thr, unsigned char* tp_p, float* oks_out, void* stream) {
  UPA_CHECK_ARG(rows && counts && gt && ngt && gt_kpt && sigma && iou_thresholds && tp_p, "pose_match: null pointer");
  UPA_CHECK_ARG(b > 0 && max_det > 0 && max_gt > 0 && nkpt > 0 && ndim > 0 && (long long)ld >= 6 + (long long)nkpt * ndim,
                "pose_match: bad shape b=%d max_det=%d max_gt=%d nkpt=%d ndim=%d ld=%d", b, max_det, max_gt, nkpt, ndim, ld);
  UPA_CHECK_ARG(n_thr == MP_NT, "pose_match: %d OKS thresholds (torch.linspace(0.5, 0.95, 10), detect/val.py:59)", MP_NT);
  if ((ndim != 2 && ndim != 3) || nkpt > PM_MAX_KPT) {
    upa_set_error("pose_match: ndim %d nkpt %d outside the supported form (ndim 2 | 3, nkpt <= %d)", ndim, nkpt, PM_MAX_KPT);
    return UPA_EUNSUPPORTED;
  }
  const size_t lds = (size_t)max_gt * (MP_NT + 3 * nkpt + 3) * 4;
  UPA_CHECK_ARG(lds <= 160 * 1024 - 1024, "pose_match: max_gt %d x nkpt %d too large for the LDS tables", max_gt, nkpt);
  PoseSigma sg;
  for (int k = 0; k < PM_MAX_KPT; ++k) {
    const float t = k < nkpt ? 2.0f * sigma[k] : 0.f;
    sg.s2[k] = t * t;
  }
  MatchThr thr;
  for (int k = 0; k < MP_NT; ++k) thr.v[k] = iou_thresholds[k];
  if (hipError_t e = upa_full_lds<pose_match_kernel>(); e != hipSuccess) return UPA_ELAUNCH;
  hipLaunchKernelGGL(pose_match_kernel, dim3((unsigned)b), dim3(256), lds, (hipStream_t)stream, rows, ld, max_det, counts, gt, ngt, max_gt,
                     gt_kpt, nkpt, ndim, sg, thr, 1e-7f, tp_p, oks_out);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}
