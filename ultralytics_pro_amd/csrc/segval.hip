// Segmentation validation on bit masks: the mask half of SegmentationValidator (ultralytics/models/yolo/segment/val.py:94-117
// postprocess with process_mask, :119-143 _prepare_batch, :145-172 _process_batch; utils/metrics.py:146-161 mask_iou;
// engine/validator.py:267-308 match_predictions).
//
// A mask of mh x mw pixels is ceil(mh mw / 32) uint32, bit k of word w = pixel 32 w + k.  The intersection of two masks is
// popcount(a & b) and every count is an integer below 2^24, so the f32 IoU equals the reference's float matmul form in any summation
// order - and a predicted mask (800 words at 160 x 160) fits in LDS, so it never has to exist in memory.
//
//  - upa_pack_mask_bits: one wave per (image, label) row: 64 pixels per step, __ballot gives two words.
//  - upa_mask_iou_bits: one wave per (i, j) pair.
//  - upa_segment_match / upa_segment_match_bits: TWO launches.  (1) segval_best_kernel, one wave per detection over the whole batch
//    (b x max_det waves: 9600 at batch 32, enough for every SIMD of the chip; one workgroup per image, the shape of the box matching,
//    would leave 224 of 256 CUs idle while each image's 300 dot-product masks are assembled): the wave assembles the detection's mask into
//    its own LDS rows - only the 64-pixel groups that intersect the crop box run the nm-deep dot product (mask_dot.h, shared with
//    upa_process_mask) -, ANDs and popcounts it against the label rows of its class (L2 resident) and leaves (best label, best IoU).
//    (2) segval_claim_kernel, one workgroup per image: the claim step of match_predictions (match_claim.h, shared with
//    upa_match_predictions), which is sequential over an image's detections.
#include "common.h"
#include "mask_dot.h"
#include "match_claim.h"

namespace {

constexpr int SV_NM = 128;          // coefficient depth limit (as upa_process_mask)
constexpr int SV_WAVES = 4;         // detections per workgroup of segval_best_kernel
constexpr int SV_MAX_WORDS = 3584;  // bit-row length limit: SV_WAVES rows of it are 56 KB of LDS (a 338 x 338 map)

// LDS traffic between the lanes of ONE wave: the wave's LDS operations complete in order; this keeps the compiler from moving
// accesses across and is the point where divergent lanes have reconverged
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// bits of the last word that are pixels (all of them when npix is a multiple of 32)
__device__ __forceinline__ unsigned tail_mask(int npix) { return (npix & 31) ? ((1u << (npix & 31)) - 1u) : 0xffffffffu; }

// popcount(a & b) over `words` words, lane-strided, the padding bits of the last word masked off; the same value in every lane
__device__ __forceinline__ int and_popcount(const uint32_t* a, const uint32_t* b, int words, int npix, int lane) {
  int s = 0;
  for (int w = lane; w < words; w += 64) {
    unsigned v = a[w] & b[w];
    if (w == words - 1) v &= tail_mask(npix);
    s += __popc(v);
  }
  return wave_sum(s);
}

__device__ __forceinline__ float iou_of(int inter, int area_a, int area_b, float eps) {
  const float fi = (float)inter;
  return fi / (((float)area_a + (float)area_b) - fi + eps);  // (area1 + area2) - intersection, + eps: utils/metrics.py:160-161
}

// ---- ground-truth masks -> bit rows -----------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ bool gt_pixel(const T* p, int form, int k) {
  if (form == UPA_MASKS_OVERLAP) return *p == (T)(k + 1) && (int)(T)(k + 1) == k + 1;  // a label index the type cannot hold matches nothing
  return (float)*p > 0.5f;
}

template <typename T>
__global__ __launch_bounds__(256) void pack_bits_kernel(const T* __restrict__ src, int form, long rows, int b, int max_gt, int npix,
                                                        int words, const int32_t* __restrict__ ngt, uint32_t* __restrict__ bits,
                                                        int32_t* __restrict__ areas) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);  // (image, label) row of the output
  if (row >= (long)b * max_gt) return;
  const int img = (int)(row / max_gt), k = (int)(row % max_gt);
  const int n = ngt ? ngt[img] : max_gt;
  uint32_t* out = bits + row * words;
  const T* plane = nullptr;
  if (k < n) {
    if (form == UPA_MASKS_OVERLAP) {
      plane = src + (size_t)img * npix;
    } else {
      long base = 0;  // exclusive prefix sum of the label counts: the ragged per-instance form
      for (int i = 0; i < img; ++i) base += ngt ? (ngt[i] > 0 ? ngt[i] : 0) : max_gt;
      if (base + k < rows) plane = src + (size_t)(base + k) * npix;
    }
  }
  if (!plane) {  // wave-uniform
    for (int w = lane; w < words; w += 64) out[w] = 0u;
    if (lane == 0) areas[row] = 0;
    return;
  }
  int area = 0;
  for (int p0 = 0; p0 < npix; p0 += 64) {
    const int p = p0 + lane;
    const bool bit = p < npix && gt_pixel(plane + p, form, k);
    const unsigned long long m = __ballot(bit);
    area += __popcll(m);
    const int w = (p0 >> 5) + lane;
    if (lane < 2 && w < words) out[w] = lane ? (unsigned)(m >> 32) : (unsigned)m;
  }
  if (lane == 0) areas[row] = area;
}

// ---- mask_iou on bit rows ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_iou_bits_kernel(const uint32_t* __restrict__ a, const int32_t* __restrict__ area_a, int n,
                                                            const uint32_t* __restrict__ b, const int32_t* __restrict__ area_b, int m,
                                                            int words, int npix, float eps, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= (long)n * m) return;
  const int i = (int)(pair / m), j = (int)(pair % m);
  const int inter = and_popcount(a + (size_t)i * words, b + (size_t)j * words, words, npix, lane);
  if (lane == 0) out[pair] = iou_of(inter, area_a[i], area_b[j], eps);
}

// ---- per detection: mask, IoU with the labels of its class, best label ---------------------------------------------------------------
struct SVArgs {
  const void* protos;  // SRC 0 (f32) | 1 (bf16)
  int ldp, mh, mw, nm;
  const uint32_t* det_bits;  // SRC 2
  const int32_t* det_area;
  const float* rows;
  int ld, max_det, b;
  const int32_t* counts;
  float cx, cy;
  const float* gt_cls;  // class of label l of image i: gt_cls[(i * max_gt + l) * gt_cls_ld]
  int gt_cls_ld;
  const uint32_t* gt_bits;
  const int32_t* gt_area;
  const int32_t* ngt;
  int max_gt, words, npix;
  float eps;
  uint32_t* pred_bits;
  int32_t* pred_area;
  float* iou_out;
  int2* best;  // (b, max_det): (best label or -1, best IoU as bits)
};

template <int SRC>
__global__ __launch_bounds__(64 * SV_WAVES) void segval_best_kernel(SVArgs A) {
  extern __shared__ uint32_t s_bits[];  // [SV_WAVES][words]
  __shared__ float s_coef[SV_WAVES][SV_NM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * SV_WAVES + wave;
  if (row >= (long)A.b * A.max_det) return;  // whole waves leave: nothing below synchronises across waves
  const int img = (int)(row / A.max_det), d = (int)(row % A.max_det);
  const int N = min(A.counts[img], A.max_det), M = max(min(A.ngt[img], A.max_gt), 0);
  float* iou_row = A.iou_out ? A.iou_out + row * A.max_gt : nullptr;
  if (d >= N) {
    if (A.pred_bits) {
      for (int w = lane; w < A.words; w += 64) A.pred_bits[row * A.words + w] = 0u;
      if (lane == 0) A.pred_area[row] = 0;
    }
    if (iou_row)
      for (int l = lane; l < A.max_gt; l += 64) iou_row[l] = 0.f;
    if (lane == 0) A.best[row] = make_int2(-1, __float_as_int(-1.f));
    return;
  }
  uint32_t* mybits = s_bits + wave * A.words;
  const float* r = A.rows + row * A.ld;
  int area;
  if constexpr (SRC == 2) {
    const uint32_t* src = A.det_bits + row * A.words;
    for (int w = lane; w < A.words; w += 64) mybits[w] = src[w];
    area = A.det_area[row];
  } else {
    float* coef = s_coef[wave];
    for (int k = lane; k < A.nm; k += 64) coef[k] = r[6 + k];
    for (int w = lane; w < A.words; w += 64) mybits[w] = 0u;
    wave_sync();
    // crop_mask's comparison form on `boxes * ratios` (f32 products), as upa_process_mask mode 0
    const float cx1 = r[0] * A.cx, cy1 = r[1] * A.cy, cx2 = r[2] * A.cx, cy2 = r[3] * A.cy;
    // rows a pixel of the box can lie in: fy >= cy1 <=> fy >= ceil(cy1), fy < cy2 <=> fy < ceil(cy2) for integer fy.  Only a bound
    // for the loop (NaN / inf corners fall to 0 or mh); the comparisons below decide every bit
    const int ylo = (int)fminf(fmaxf(ceilf(cy1), 0.f), (float)A.mh), yhi = (int)fminf(fmaxf(ceilf(cy2), 0.f), (float)A.mh);
    area = 0;
    const int p_end = yhi * A.mw;  // <= npix
    for (int p0 = (ylo * A.mw) & ~63; p0 < p_end; p0 += 64) {
      const int p = p0 + lane;
      const int py = p / A.mw, px = p - py * A.mw;
      const bool in = p < A.npix && mask_in_crop((float)px, (float)py, cx1, cy1, cx2, cy2);
      if (__ballot(in) == 0ull) continue;  // the whole group is outside the box: its two words stay zero, no proto is loaded
      bool bit = false;
      if (in) {
        const size_t pix = (size_t)img * A.npix + p;
        float v;
        if constexpr (SRC == 1) v = mask_dot_bf16(coef, (const bf16_t*)A.protos + pix * A.ldp, A.nm);
        else v = mask_dot_f32(coef, (const float*)A.protos + pix * A.ldp, A.nm);
        bit = v > 0.f;
      }
      const unsigned long long m = __ballot(bit);
      area += __popcll(m);
      const int w = (p0 >> 5) + lane;
      if (lane < 2 && w < A.words) mybits[w] = lane ? (unsigned)(m >> 32) : (unsigned)m;
    }
  }
  wave_sync();
  if (A.pred_bits) {
    for (int w = lane; w < A.words; w += 64) A.pred_bits[row * A.words + w] = mybits[w];
    if (lane == 0) A.pred_area[row] = area;
  }
  const float cls = r[5];
  const float* gc = A.gt_cls + (size_t)img * A.max_gt * A.gt_cls_ld;
  int bl = -1;
  float bi = -1.f;
  for (int l = 0; l < M; ++l) {  // wave-uniform control flow
    float iou = 0.f;
    const bool same = gc[(size_t)l * A.gt_cls_ld] == cls;
    if (same) {
      const size_t g = (size_t)img * A.max_gt + l;
      iou = iou_of(and_popcount(mybits, A.gt_bits + g * A.words, A.words, A.npix, lane), area, A.gt_area[g], A.eps);
      if (iou >= bi) { bi = iou; bl = l; }  // ties: the larger label index, as upa_match_predictions
    }
    if (iou_row && lane == 0) iou_row[l] = iou;
  }
  if (iou_row)
    for (int l = M + lane; l < A.max_gt; l += 64) iou_row[l] = 0.f;
  if (lane == 0) A.best[row] = make_int2(bl, __float_as_int(bi));
}

// ---- per image: the claim step ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void segval_claim_kernel(const int2* __restrict__ best, const int32_t* __restrict__ counts, int max_det,
                                                           const int32_t* __restrict__ ngt, int max_gt, MatchThr thr,
                                                           unsigned char* __restrict__ tp) {
  extern __shared__ int s_min[];  // [max_gt][MP_NT]
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = min(counts[b], max_det), M = min(ngt[b], max_gt);
  for (int i = tid; i < M * MP_NT; i += 256) s_min[i] = 0x7fffffff;
  __syncthreads();
  unsigned char* T = tp + (size_t)b * max_det * MP_NT;
  for (int base = 0; base < max_det; base += 256) {
    const int d = base + tid;
    int bl = -1;
    float bi = -1.f;
    if (d < N) {
      const int2 v = best[(size_t)b * max_det + d];
      bl = v.x < M ? v.x : -1;
      bi = __int_as_float(v.y);
    }
    match_claim_round(s_min, d, N, max_det, bl, bi, thr, T);
  }
}

int sv_launch(SVArgs& A, int src, const float* iou_thresholds, int n_thr, unsigned char* tp_m, void* workspace, size_t workspace_bytes,
              const char* what, hipStream_t s) {
  UPA_CHECK_ARG(A.rows && A.counts && A.gt_cls && A.gt_bits && A.gt_area && A.ngt && iou_thresholds && tp_m && workspace,
                "%s: null pointer", what);
  UPA_CHECK_ARG(A.b > 0 && A.mh > 0 && A.mw > 0 && A.max_det > 0 && A.max_gt > 0 && A.gt_cls_ld > 0 && (long long)A.mh * A.mw <= 0x7fffffc0ll,
                "%s: bad shape b=%d map=%dx%d max_det=%d max_gt=%d", what, A.b, A.mh, A.mw, A.max_det, A.max_gt);
  UPA_CHECK_ARG((A.pred_bits == nullptr) == (A.pred_area == nullptr), "%s: pred_bits and pred_area come together", what);
  UPA_CHECK_ARG(n_thr == MP_NT, "%s: %d IoU thresholds (torch.linspace(0.5, 0.95, 10), detect/val.py:59)", what, MP_NT);
  UPA_CHECK_ARG((size_t)A.max_gt * MP_NT * 4 <= 160 * 1024 - 1024, "%s: max_gt too large for the LDS table", what);
  UPA_CHECK_ARG(workspace_bytes >= upa_segment_match_workspace_bytes(A.b, A.max_det) && ((uintptr_t)workspace % 8) == 0,
                "%s: workspace of %zu bytes", what, workspace_bytes);
  A.npix = A.mh * A.mw;
  A.words = cdiv(A.npix, 32);
  if (A.words > SV_MAX_WORDS) {
    upa_set_error("%s: a %dx%d map is %d words per mask, more than the %d a workgroup keeps in LDS", what, A.mh, A.mw, A.words, SV_MAX_WORDS);
    return UPA_EUNSUPPORTED;
  }
  A.eps = 1e-7f;
  A.best = (int2*)workspace;
  MatchThr thr;
  for (int k = 0; k < MP_NT; ++k) thr.v[k] = iou_thresholds[k];
  if (hipError_t e = upa_full_lds<segval_claim_kernel>(); e != hipSuccess) return UPA_ELAUNCH;
  const dim3 grid((unsigned)(((long)A.b * A.max_det + SV_WAVES - 1) / SV_WAVES)), block(64 * SV_WAVES);
  const size_t lds = (size_t)SV_WAVES * A.words * 4;
  if (src == 0) hipLaunchKernelGGL(segval_best_kernel<0>, grid, block, lds, s, A);
  else if (src == 1) hipLaunchKernelGGL(segval_best_kernel<1>, grid, block, lds, s, A);
  else hipLaunchKernelGGL(segval_best_kernel<2>, grid, block, lds, s, A);
  UPA_LAUNCH_CHECK();
  hipLaunchKernelGGL(segval_claim_kernel, dim3((unsigned)A.b), dim3(256), (size_t)A.max_gt * MP_NT * 4, s, A.best, A.counts, A.max_det,
                     A.ngt, A.max_gt, thr, tp_m);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

}  // namespace

// ---- entry points ------------------------------------------------------------------------------------------------------------------

extern "C" int upa_pack_mask_bits(const void* src, int src_type, int form, long rows, int b, int max_gt, int mh, int mw, const int32_t* ngt,
                                  uint32_t* bits, int32_t* areas, void* stream) {
  UPA_CHECK_ARG(src && bits && areas, "pack_mask_bits: null pointer");
  UPA_CHECK_ARG(b > 0 && max_gt > 0 && mh > 0 && mw > 0 && rows >= 0 && (long long)mh * mw <= 0x7fffffc0ll,
                "pack_mask_bits: bad shape b=%d max_gt=%d map=%dx%d rows=%ld", b, max_gt, mh, mw, rows);
  UPA_CHECK_ARG(form == UPA_MASKS_PLANES || form == UPA_MASKS_OVERLAP, "pack_mask_bits: form %d", form);
  if ((src_type != UPA_MASK_U8 && src_type != UPA_MASK_F32 && src_type != UPA_MASK_I32) ||
      (form == UPA_MASKS_PLANES && src_type == UPA_MASK_I32)) {
    upa_set_error("pack_mask_bits: source type %d outside u8 | f32 (planes) and u8 | i32 | f32 (index maps)", src_type);
    return UPA_EUNSUPPORTED;
  }
  const int npix = mh * mw, words = cdiv(npix, 32);
  const dim3 grid((unsigned)(((long)b * max_gt + 3) / 4));
  hipStream_t s = (hipStream_t)stream;
  if (src_type == UPA_MASK_U8)
    hipLaunchKernelGGL(pack_bits_kernel<uint8_t>, grid, dim3(256), 0, s, (const uint8_t*)src, form, rows, b, max_gt, npix, words, ngt, bits, areas);
  else if (src_type == UPA_MASK_F32)
    hipLaunchKernelGGL(pack_bits_kernel<float>, grid, dim3(256), 0, s, (const float*)src, form, rows, b, max_gt, npix, words, ngt, bits, areas);
  else
    hipLaunchKernelGGL(pack_bits_kernel<int32_t>, grid, dim3(256), 0, s, (const int32_t*)src, form, rows, b, max_gt, npix, words, ngt, bits, areas);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_mask_iou_bits(const uint32_t* a, const int32_t* area_a, int n, const uint32_t* b, const int32_t* area_b, int m, int npix,
                                 float eps, float* out, void* stream) {
  UPA_CHECK_ARG(n >= 0 && m >= 0 && npix > 0 && npix <= 0x7fffffc0, "mask_iou_bits: bad shape n=%d m=%d npix=%d", n, m, npix);
  if (n == 0 || m == 0) return UPA_OK;
  UPA_CHECK_ARG(a && area_a && b && area_b && out, "mask_iou_bits: null pointer");
  const long pairs = (long)n * m;
  hipLaunchKernelGGL(mask_iou_bits_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, area_a, n, b, area_b, m,
                     cdiv(npix, 32), npix, eps, out);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" size_t upa_segment_match_workspace_bytes(int b, int max_det) {
  return b > 0 && max_det > 0 ? (size_t)b * max_det * sizeof(int2) : 0;
}

extern "C" int upa_segment_match(const void* protos, int b, int mh, int mw, int nm, int ldp, int dtype, const float* rows, int ld, int max_det,
                                 const int32_t* counts, float crop_sx, float crop_sy, const float* gt_cls, int gt_cls_ld, const uint32_t* gt_bits,
                                 const int32_t* gt_area, const int32_t* ngt, int max_gt, const float* iou_thresholds, int n_thr,
                                 unsigned char* tp_m, uint32_t* pred_bits, int32_t* pred_area, float* iou_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  UPA_CHECK_ARG(protos, "segment_match: null pointer");
  UPA_CHECK_ARG(nm > 0 && ldp >= nm && ld >= 6 + nm, "segment_match: bad shape nm=%d ldp=%d ld=%d", nm, ldp, ld);
  if ((dtype != UPA_F32 && dtype != UPA_BF16) || nm > SV_NM) {
    upa_set_error("segment_match: dtype %d nm %d outside the supported form (f32 | bf16, nm <= %d)", dtype, nm, SV_NM);
    return UPA_EUNSUPPORTED;
  }
  const int vec = 16 / upa_elem_size(dtype);
  UPA_CHECK_ARG(nm % vec == 0 && ldp % vec == 0 && ((uintptr_t)protos % 16) == 0, "segment_match: proto channels must be 16-byte groups");
  SVArgs A{};
  A.protos = protos, A.ldp = ldp, A.mh = mh, A.mw = mw, A.nm = nm;
  A.rows = rows, A.ld = ld, A.max_det = max_det, A.b = b, A.counts = counts, A.cx = crop_sx, A.cy = crop_sy;
  A.gt_cls = gt_cls, A.gt_cls_ld = gt_cls_ld, A.gt_bits = gt_bits, A.gt_area = gt_area, A.ngt = ngt, A.max_gt = max_gt;
  A.pred_bits = pred_bits, A.pred_area = pred_area, A.iou_out = iou_out;
  return sv_launch(A, dtype == UPA_BF16 ? 1 : 0, iou_thresholds, n_thr, tp_m, workspace, workspace_bytes, "segment_match", (hipStream_t)stream);
}

extern "C" int upa_segment_match_bits(const uint32_t* det_bits, const int32_t* det_area, int b, int mh, int mw, const float* rows, int ld,
                                      int max_det, const int32_t* counts, const float* gt_cls, int gt_cls_ld, const uint32_t* gt_bits,
                                      const int32_t* gt_area, const int32_t* ngt, int max_gt, const float* iou_thresholds, int n_thr,
                                      unsigned char* tp_m, float* iou_out, void* workspace, size_t workspace_bytes, void* stream) {
  UPA_CHECK_ARG(det_bits && det_area, "segment_match_bits: null pointer");
  UPA_CHECK_ARG(ld >= 6, "segment_match_bits: bad row stride %d", ld);
  SVArgs A{};
  A.det_bits = det_bits, A.det_area = det_area, A.mh = mh, A.mw = mw;
  A.rows = rows, A.ld = ld, A.max_det = max_det, A.b = b, A.counts = counts;
  A.gt_cls = gt_cls, A.gt_cls_ld = gt_cls_ld, A.gt_bits = gt_bits, A.gt_area = gt_area, A.ngt = ngt, A.max_gt = max_gt;
  A.iou_out = iou_out;
  return sv_launch(A, 2, iou_thresholds, n_thr, tp_m, workspace, workspace_bytes, "segment_match_bits", (hipStream_t)stream);
}
