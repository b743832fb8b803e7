// Classification head for gfx950 (CDNA4): the Classify module's hot path (ultralytics/nn/modules/head.py:1481-1531).
//
//   upa_classify_pool   pooled[i, c] = (1 / HW) * sum_p act( sum_k x[i, p, k] * W[c, k] + bias[c] )
//                       = AdaptiveAvgPool2d(1)(Conv(c1, 1280, 1)(x)).flatten(1) with BN folded, as ONE launch: the (n, h, w, 1280)
//                       activation stays in MFMA accumulators and is never written.
//   upa_softmax_topk    probs = softmax(logits, 1) and the indices of the k largest logits per row.
// The nn.Linear between the two is upa_linear (csrc/transformer.hip).
//
// upa_classify_pool mapping: a workgroup of 4 waves owns ONE image and 64 output channels (4 n-tiles).  It walks the image's HW
// pixels in chunks of 64 rows, 16 per wave.  GEMM orientation as in conv.hip: A = packed weights (rows = channels), B = pixels
// (columns), D[row = channel][col = pixel] - lane (g, r) holds channels 4 g .. 4 g + 3 of every n-tile for pixel r.  Both operands
// are read straight from global memory in fragment order (a lane's 16 bytes of a pixel row; a wave's coalesced 1 KiB of packed
// weights): a 64-channel weight slab at cin = 1280 is 327 KB in f32 and fits no LDS, so the weights stream per k-tile - once when
// HW <= 64 (every cls model at 224 x 224 has a 7 x 7 map), from L2 again for each further pixel chunk.
//   * rows past HW: their B fragment is zero and, because act(bias) != 0, their activation is dropped AFTER the activation;
//   * channels past cin inside the last k-tile: zero fragments (the packed weights are zero there too, the input need not be);
//   * summation order is fixed: per lane over the chunks, then over the 16 pixel lanes (xor 8, 4, 2, 1), then over the four waves
//     through LDS in wave order, then one divide by HW.  No atomics, nothing depends on the grid: two runs are bit-identical.
#include "common.h"

namespace {

struct ClsPoolParams {
  const char* x;
  const char* w;
  const float* bias;
  float* pooled;
  int HW, Cin, ldx, Cout, ldp;
  int KTT;  // k-tiles (64 bytes of channels each) of the packed weights
  int NTn;  // n-tiles of the packed weights (Cout padded to 16 / 16)
};

template <bool PRECISE, int ACT>
__device__ __forceinline__ float cls_act(float v) {
  if constexpr (ACT == UPA_ACT_SILU) {
    if constexpr (PRECISE) return v / (1.0f + expf(-v));  // f32 parity mode: ocml expf + IEEE divide, as conv.hip's f32 epilogue
    return silu_rcp(v);
  } else {
    return v;
  }
}

template <typename T, int ACT>
__global__ __launch_bounds__(256) void classify_pool_kernel(const ClsPoolParams p) {
  constexpr int ES = sizeof(T);
  constexpr int E = 16 / ES;
  constexpr int KT_CH = 64 / ES;
  __shared__ float red[4][64];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int img = blockIdx.y;
  const int nt0 = blockIdx.x * 4;

  f32x4 bv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int co = (nt0 + j) * 16 + g * 4 + e;
      bv[j][e] = (p.bias && co < p.Cout) ? p.bias[co] : 0.0f;
    }
  }

  f32x4 sum[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) sum[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const size_t wTile = (size_t)p.NTn * 1024;  // bytes per k-tile of packed weights
  const char* wlane = p.w + (size_t)nt0 * 1024 + lane * 16;

  for (int p0 = wave * 16; p0 < p.HW; p0 += 64) {  // this wave's 16 rows of each 64-row chunk (wave-uniform trip count)
    const int pix = p0 + r;
    const bool valid = pix < p.HW;
    const char* xrow = p.x + ((size_t)img * p.HW + (valid ? pix : 0)) * (size_t)p.ldx * ES;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int kt = 0; kt < p.KTT; ++kt) {
      const int ch = kt * KT_CH + g * E;
      u32x4 b = u32x4{0u, 0u, 0u, 0u};
      if (valid && ch < p.Cin) b = *reinterpret_cast<const u32x4*>(xrow + (size_t)ch * ES);
      u32x4 a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        a[j] = (nt0 + j < p.NTn) ? *reinterpret_cast<const u32x4*>(wlane + (size_t)kt * wTile + j * 1024) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (ES == 2) {
          acc[j] = mfma32(a[j], b, acc[j]);
        } else {
          const float* af = reinterpret_cast<const float*>(&a[j]);
          const float* bf = reinterpret_cast<const float*>(&b);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[0], bf[0], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[1], bf[1], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[2], bf[2], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[3], bf[3], acc[j], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float s = cls_act<ES == 4, ACT>(acc[j][e] + bv[j][e]);
        sum[j][e] += valid ? s : 0.0f;  // a padded row would add act(bias): masked after the activation
      }
    }
  }

  // over the 16 pixel lanes of each channel group (lanes g * 16 + r: xor < 16 stays inside the group)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = sum[j][e];
      v += __shfl_xor(v, 8, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 1, 64);
      if (r == 0) red[wave][j * 16 + g * 4 + e] = v;
    }
  }
  __syncthreads();
  if (tid < 64) {
    const int co = blockIdx.x * 64 + tid;
    if (co < p.Cout) {
      const float total = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
      p.pooled[(size_t)img * p.ldp + co] = total / (float)p.HW;
    }
  }
}

// ---- softmax + top-k -------------------------------------------------------------------------------------------------------------
// One workgroup per row (64 threads up to 512 classes, else 256).  Every reduction runs in a fixed order (strided per thread, xor
// butterfly per wave, wave order through LDS).  The top-k ranks LOGITS: key = the float's bits mapped to an unsigned integer with the
// float order (-0 counts as +0), packed above ~index, so the 64-bit maximum is the largest logit at the lowest index; pass t takes
// the largest packed key below pass t - 1's winner.
__device__ __forceinline__ unsigned long long topk_key(float v, int idx) {
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)idx);
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
  const unsigned lo = __shfl_xor((unsigned)(v & 0xFFFFFFFFull), m, 64);
  const unsigned hi = __shfl_xor((unsigned)(v >> 32), m, 64);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ void softmax_topk_kernel(const float* __restrict__ logits, int nc, int ldl, float* __restrict__ probs, int ldpr, int k,
                                    int32_t* __restrict__ topk) {
  __shared__ float redf[4];
  __shared__ unsigned long long redk[4];
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  const size_t row = blockIdx.x;
  const float* z = logits + row * (size_t)ldl;
  float* pr = probs + row * (size_t)ldpr;

  float m = -INFINITY;
  for (int i = tid; i < nc; i += nthr) m = fmaxf(m, z[i]);
  for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
  if (lane == 0) redf[wave] = m;
  __syncthreads();
  m = redf[0];
  for (int w = 1; w < nw; ++w) m = fmaxf(m, redf[w]);
  __syncthreads();

  float s = 0.0f;
  for (int i = tid; i < nc; i += nthr) s += expf(z[i] - m);
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) redf[wave] = s;
  __syncthreads();
  s = redf[0];
  for (int w = 1; w < nw; ++w) s += redf[w];
  for (int i = tid; i < nc; i += nthr) pr[i] = expf(z[i] - m) / s;

  if (topk == nullptr) return;
  unsigned long long prev = ~0ull;
  for (int t = 0; t < k; ++t) {
    unsigned long long best = 0ull;  // below every key (the high word of a finite or infinite logit's key is never 0)
    for (int i = tid; i < nc; i += nthr) {
      const unsigned long long key = topk_key(z[i], i);
      if (key < prev && key > best) best = key;
    }
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = shfl_xor_u64(best, d);
      best = o > best ? o : best;
    }
    __syncthreads();  // the previous pass's readers of redk are done
    if (lane == 0) redk[wave] = best;
    __syncthreads();
    best = redk[0];
    for (int w = 1; w < nw; ++w) best = redk[w] > best ? redk[w] : best;
    if (tid == 0) topk[row * (size_t)k + t] = (int32_t)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
    prev = best;
  }
}

template <typename T>
void launch_pool(const ClsPoolParams& p, int n, int act, hipStream_t stream) {
  const dim3 grid((unsigned)cdiv(p.Cout, 64), (unsigned)n);
  if (act == UPA_ACT_SILU) hipLaunchKernelGGL((classify_pool_kernel<T, UPA_ACT_SILU>), grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((classify_pool_kernel<T, UPA_ACT_NONE>), grid, dim3(256), 0, stream, p);
}

}  // namespace

extern "C" int upa_classify_pool(const void* x, int n, int h, int w, int cin, int ldx, const void* w_packed, const float* bias,
                                 float* pooled, int cout, int ldp, int act, int dtype, const upa_opts* opts, void* stream) {
  (void)opts;  // no dispatch choice to override
  UPA_CHECK_ARG(x && w_packed && bias && pooled, "classify_pool: null pointer");
  UPA_CHECK_ARG(n > 0 && h > 0 && w > 0 && cin > 0 && cout > 0, "classify_pool: bad shape");
  UPA_CHECK_ARG(n <= 65535 && (long long)h * w <= (1 << 24), "classify_pool: n > 65535 or h * w > 2^24");
  UPA_CHECK_ARG(ldx >= cin && ldp >= cout, "classify_pool: ldx < cin or ldp < cout");
  if ((act != UPA_ACT_NONE && act != UPA_ACT_SILU) || (dtype != UPA_F32 && dtype != UPA_BF16)) {
    upa_set_error("classify_pool: act must be NONE | SILU and dtype F32 | BF16");
    return UPA_EUNSUPPORTED;
  }
  const int E = 16 / upa_elem_size(dtype);
  UPA_CHECK_ARG(cin % E == 0 && ldx % E == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)w_packed % 16 == 0,
                "classify_pool: x, cin and ldx must be multiples of 16 bytes (%d elements)", E);
  UPA_CHECK_ARG((uintptr_t)pooled % 4 == 0 && (uintptr_t)bias % 4 == 0, "classify_pool: misaligned float pointer");
  ClsPoolParams p;
  p.x = (const char*)x; p.w = (const char*)w_packed; p.bias = bias; p.pooled = pooled;
  p.HW = h * w; p.Cin = cin; p.ldx = ldx; p.Cout = cout; p.ldp = ldp;
  p.KTT = cdiv(cin, 4 * E); p.NTn = cdiv(cout, 16);
  if (dtype == UPA_BF16) launch_pool<bf16_t>(p, n, act, (hipStream_t)stream);
  else launch_pool<float>(p, n, act, (hipStream_t)stream);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_softmax_topk(const float* logits, int rows, int nc, int ldl, float* probs, int ldpr, int k, int32_t* topk_idx,
                                void* stream) {
  UPA_CHECK_ARG(logits && probs, "softmax_topk: null pointer");
  UPA_CHECK_ARG(rows > 0 && nc > 0, "softmax_topk: bad shape");
  UPA_CHECK_ARG(ldl >= nc && ldpr >= nc, "softmax_topk: ldl < nc or ldpr < nc");
  if (nc > 65536 || k < 1 || k > 16 || k > nc) {
    upa_set_error("softmax_topk: needs 1 <= k <= min(nc, 16) and nc <= 65536 (k = %d, nc = %d)", k, nc);
    return UPA_EUNSUPPORTED;
  }
  hipLaunchKernelGGL(softmax_topk_kernel, dim3((unsigned)rows), dim3(nc <= 512 ? 64 : 256), 0, (hipStream_t)stream, logits, nc, ldl,
                     probs, ldpr, k, topk_idx);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}
