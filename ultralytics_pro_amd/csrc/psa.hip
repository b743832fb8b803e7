// YOLO11 PSA attention core (v10_Attention.forward, ultralytics/nn/modules/block.py:1701-1722) after its qkv conv:
//   per (image, head):  attn = softmax_keys(scale * q^T k),  out[j][p] = sum_q v[j][q] attn[p][q]  +  pe(v)[j][p]
// where q / k / v are the channel slices [q (key_dim) | k (key_dim) | v (head_dim)] of the head's 2 key_dim + head_dim channels of the
// qkv conv's NHWC output (`qkv.view(B, heads, 2 kd + hd, N).split(...)`, :1713-1716) and pe is the depthwise 3x3 conv of v laid out as
// an image with channel head * hd + j (BN folded, no activation, :1719).  The result is `proj`'s input.
//
// Work split: a workgroup = 64 queries (one per lane) x 4 key partitions (one wave each) of one (image, head).  The keys are streamed
// through LDS in blocks of 64 (K and V as f32), wave `part` takes keys [16 part, 16 part + 16) of every block, so any number of tokens
// works (1600 at 1280 x 1280: K + V of one head is 300 KB in bf16, more than LDS).  Every lane keeps an online softmax (max, sum,
// out[hd]) in registers; the four partial states are merged in partition order through LDS (exact, deterministic).  The normalised
// outputs go through LDS once more so that all 256 threads add pe and write channel-contiguous 64-channel rows.
// This is the f32 (exact) path, and the bf16 path for views the matrix-core kernel below cannot read (unaligned strides).
//
// bf16, key_dim 32 / head_dim 64 (every YOLO11 scale): psa_attn_mfma_kernel, the layout of attention.hip's mhsa_mfma_bf16_d32_kernel
// with streamed key blocks.  A wave owns 16 queries; a workgroup of PSA_MW waves shares each block of 64 keys, staged in LDS as K
// ([key][64 B], 16-byte groups XOR-swizzled by key >> 1) and V^T ([dim][key], pitch 4 mod 8 dwords).  Per block and wave:
//   S^T (64 keys x 16 queries) = K . Q^T: four 16x16x32 MFMAs, lane (g, r) holds keys 4g .. 4g + 3 of each 16-key tile for query r;
//   online softmax in f32 on log2(e)-scaled scores (v_exp_f32), the block max reduced over the query's four lanes;
//   O^T (64 dims x 16 queries) += V^T . P^T: the exponentials of two S^T tiles packed to bf16 are the B operand (k order: keys 4g + e of
//   the first tile, then of the second), four dim tiles x two key halves = eight MFMAs.
// The normalised outputs go through LDS to the same channel-contiguous pe epilogue as the f32 path.
#include "common.h"

constexpr int PSA_KB = 64;  // keys per LDS block
constexpr int PSA_KP = 4;   // key partitions (waves) of the f32 kernel
constexpr int PSA_MW = 2;   // waves (x 16 queries) per workgroup of the matrix-core kernel


template <int KD, int HD>
constexpr size_t psa_lds_bytes() {
  return ((size_t)PSA_KB * (KD + HD) + (size_t)(PSA_KP - 1) * (HD + 2) * 64) * sizeof(float);
}

// y[query, hh * HD + j] = os[query - q0][j] + pe(v)[query, j] for the NQ queries from q0: channel-contiguous over the workgroup
template <typename T, int KD, int HD, bool PE = true>
__device__ __forceinline__ void psa_pe_epilogue(const T* __restrict__ qkv, int ld, size_t pix0, int N, int W, int heads, int hh, int q0, int NQ,
                                                const float* os, const float* __restrict__ pw, const float* __restrict__ pb, T* __restrict__ y,
                                                int ldy) {
  const int C = heads * HD, cv = hh * (2 * KD + HD) + 2 * KD, Hh = N / W;
  for (int i = threadIdx.x; i < NQ * HD; i += blockDim.x) {
    const int ql = i / HD, j = i % HD;
    const int pq = q0 + ql;
    if (pq >= N) continue;
    const int py = pq / W, px = pq % W;
    const int c = hh * HD + j;
    float acc = 0.f;  // PE = false (training forward): the same `os + 0` as a zero pe gives, so the two entries agree bit for bit
    if constexpr (PE) {
      acc = pb[c];
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const int iy = py + dy;
        if (iy < 0 || iy >= Hh) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int ix = px + dx;
          if (ix < 0 || ix >= W) continue;
          acc = fmaf(pw[(size_t)((dy + 1) * 3 + dx + 1) * C + c], ElemTraits<T>::load(qkv + (pix0 + (size_t)iy * W + ix) * (size_t)ld + cv + j), acc);
        }
      }
    }
    const float val = os[ql * (HD + 1) + j] + acc;
    T* yp = y + (pix0 + pq) * (size_t)ldy + c;
    if constexpr (sizeof(T) == 4) *yp = val;
    else *yp = f32_to_bf16(val);
  }
}

// TRAIN: no pe (upa_psa_attention_train_fwd) and lse[(image * heads + head) * N + query] = log sum_keys exp(scale q.k) is written.
template <typename T, int KD, int HD, bool TRAIN = false>
__global__ __launch_bounds__(256) void psa_attn_kernel(const T* __restrict__ qkv, int ld, int N, int W, int heads, int tiles_q, float scale,
                                                       const float* __restrict__ pw, const float* __restrict__ pb, T* __restrict__ y, int ldy,
                                                       float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  float* ks = reinterpret_cast<float*>(sm);                 // [KB][KD]
  float* vs = ks + PSA_KB * KD;                             // [KB][HD]
  float* part_sm = vs + PSA_KB * HD;                        // [KP - 1][HD + 2][64] partial states (lane-major)
  float* os = ks;                                           // [64][HD + 1] normalised outputs (after the key walk)
  constexpr int CH = 2 * KD + HD;
  const int tid = threadIdx.x, lane = tid & 63, part = tid >> 6;
  const int qt = blockIdx.x % tiles_q, bh = blockIdx.x / tiles_q;
  const int hh = bh % heads, b = bh / heads;
  const size_t pix0 = (size_t)b * N;
  const int cq = hh * CH, ck = cq + KD, cv = cq + 2 * KD;
  const int p = qt * 64 + lane;
  const bool valid = p < N;
  float qr[KD], o[HD];
  {
    const T* qp = qkv + (pix0 + (valid ? p : 0)) * (size_t)ld + cq;
#pragma unroll
    for (int i = 0; i < KD; ++i) qr[i] = valid ? ElemTraits<T>::load(qp + i) * scale : 0.f;
#pragma unroll
    for (int i = 0; i < HD; ++i) o[i] = 0.f;
  }
  float m = -INFINITY, l = 0.f;
  constexpr int PER = PSA_KB / PSA_KP;
  for (int k0 = 0; k0 < N; k0 += PSA_KB) {
    __syncthreads();  // the previous block has been consumed by every wave
    for (int i = tid; i < PSA_KB * KD; i += 256) {
      const int key = k0 + i / KD;
      ks[i] = key < N ? ElemTraits<T>::load(qkv + (pix0 + key) * (size_t)ld + ck + i % KD) : 0.f;
    }
    for (int i = tid; i < PSA_KB * HD; i += 256) {
      const int key = k0 + i / HD;
      vs[i] = key < N ? ElemTraits<T>::load(qkv + (pix0 + key) * (size_t)ld + cv + i % HD) : 0.f;
    }
    __syncthreads();
    const int j0 = part * PER;
    const int jn = min(PER, N - k0 - j0);
    for (int jj = 0; jj < jn; ++jj) {
      const float* kr = ks + (j0 + jj) * KD;
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < KD; ++i) s = fmaf(qr[i], kr[i], s);
      const float mn = fmaxf(m, s);
      const float alpha = expf(m - mn);  // exp(-inf) = 0 on the partition's first key
      const float pj = expf(s - mn);
      l = l * alpha + pj;
      const float* vr = vs + (j0 + jj) * HD;
#pragma unroll
      for (int i = 0; i < HD; ++i) o[i] = fmaf(pj, vr[i], o[i] * alpha);
      m = mn;
    }
  }
  // merge the partitions into wave 0 (partition 0 always holds key 0, so the merged max is finite)
  if (part > 0) {
    float* mine = part_sm + (size_t)(part - 1) * (HD + 2) * 64;
    mine[lane] = m;
    mine[64 + lane] = l;
#pragma unroll
    for (int i = 0; i < HD; ++i) mine[(2 + i) * 64 + lane] = o[i];
  }
  __syncthreads();  // also: every wave is done with ks / vs, which `os` reuses
  if (part == 0) {
    float mm = m;
#pragma unroll
    for (int q_ = 1; q_ < PSA_KP; ++q_) mm = fmaxf(mm, part_sm[(size_t)(q_ - 1) * (HD + 2) * 64 + lane]);
    const float a0 = expf(m - mm);
    l *= a0;
#pragma unroll
    for (int i = 0; i < HD; ++i) o[i] *= a0;
#pragma unroll
    for (int q_ = 1; q_ < PSA_KP; ++q_) {
      const float* ot = part_sm + (size_t)(q_ - 1) * (HD + 2) * 64;
      const float aq = expf(ot[lane] - mm);
      l += ot[64 + lane] * aq;
#pragma unroll
      for (int i = 0; i < HD; ++i) o[i] = fmaf(ot[(2 + i) * 64 + lane], aq, o[i]);
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int i = 0; i < HD; ++i) os[lane * (HD + 1) + i] = o[i] * inv;
    if constexpr (TRAIN) {
      if (valid) lse[(size_t)bh * N + p] = mm + logf(l);
    }
  }
  __syncthreads();
  psa_pe_epilogue<T, KD, HD, !TRAIN>(qkv, ld, pix0, N, W, heads, hh, qt * 64, 64, os, pw, pb, y, ldy);
}

// bf16, KD = 32, HD = 64 on the matrix cores (see the top of the file).  Requires ld % 8 == 0 and a 16-byte aligned qkv.
template <bool TRAIN = false>
__global__ __launch_bounds__(64 * PSA_MW) void psa_attn_mfma_kernel(const bf16_t* __restrict__ qkv, int ld, int N, int W, int heads, int tiles_q,
                                                                   float c_log2, const float* __restrict__ pw, const float* __restrict__ pb,
                                                                   bf16_t* __restrict__ y, int ldy, float* __restrict__ lse) {
  constexpr int KD = 32, HD = 64, CH = 2 * KD + HD, NQ = 16 * PSA_MW;
  constexpr int VP = PSA_KB / 2 + 4;  // dwords per V^T row (= 4 mod 8)
  __shared__ __attribute__((aligned(16))) char ks[PSA_KB * 64];
  __shared__ __attribute__((aligned(16))) char vt[HD * VP * 4];
  __shared__ float os[NQ * (HD + 1)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = 64 * PSA_MW;
  const int g = lane >> 4, r = lane & 15;
  const int qt = blockIdx.x % tiles_q, bh = blockIdx.x / tiles_q;
  const int hh = bh % heads, b = bh / heads;
  const size_t pix0 = (size_t)b * N;
  const int cq = hh * CH, ck = cq + KD, cv = cq + 2 * KD;
  const int qi = qt * NQ + wave * 16 + r;
  u32x4 qB = u32x4{0u, 0u, 0u, 0u};
  if (qi < N) qB = *reinterpret_cast<const u32x4*>(qkv + (pix0 + qi) * (size_t)ld + cq + g * 8);
  float m = -INFINITY, l = 0.f;
  f32x4 o[4][1];
  const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j][0] = z;
  for (int k0 = 0; k0 < N; k0 += PSA_KB) {
    __syncthreads();  // every wave is done with the previous block
    for (int i = tid; i < PSA_KB * 4; i += NT) {  // K: (key, 16-byte group), swizzled
      const int key = i >> 2, cg = i & 3;
      u32x4 x = u32x4{0u, 0u, 0u, 0u};
      if (k0 + key < N) x = *reinterpret_cast<const u32x4*>(qkv + (pix0 + k0 + key) * (size_t)ld + ck + cg * 8);
      *reinterpret_cast<u32x4*>(ks + key * 64 + ((cg ^ ((key >> 1) & 3)) << 4)) = x;
    }
    for (int i = tid; i < PSA_KB * 8; i += NT) {  // V^T: (key, 8 dims) -> eight 2-byte stores
      const int key = i >> 3, dg = i & 7;
      u32x4 x = u32x4{0u, 0u, 0u, 0u};
      if (k0 + key < N) x = *reinterpret_cast<const u32x4*>(qkv + (pix0 + k0 + key) * (size_t)ld + cv + dg * 8);
      unsigned short* col = reinterpret_cast<unsigned short*>(vt) + key;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        col[(size_t)(dg * 8 + 2 * e) * VP * 2] = (unsigned short)(x[e] & 0xFFFFu);
        col[(size_t)(dg * 8 + 2 * e + 1) * VP * 2] = (unsigned short)(x[e] >> 16);
      }
    }
    __syncthreads();
    float t[16];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int kk = tt * 16 + r;
      const u32x4 a = *reinterpret_cast<const u32x4*>(ks + kk * 64 + ((g ^ ((kk >> 1) & 3)) << 4));
      const f32x4 sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&a), *reinterpret_cast<const bf16x8*>(&qB), z, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) t[tt * 4 + e] = (k0 + tt * 16 + 4 * g + e < N) ? sc[e] * c_log2 : -INFINITY;
    }
    float bm = t[0];
#pragma unroll
    for (int e = 1; e < 16; ++e) bm = fmaxf(bm, t[e]);
    bm = fmaxf(bm, __shfl_xor(bm, 16));
    bm = fmaxf(bm, __shfl_xor(bm, 32));
    const float mn = fmaxf(m, bm);  // finite: every block holds at least one key
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    float pe[16], ps = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      pe[e] = __builtin_amdgcn_exp2f(t[e] - mn);
      ps += pe[e];
    }
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int half = 0; half < 2; ++half) {  // keys [32 half, 32 half + 32): tiles 2 half and 2 half + 1
      const float* p0 = pe + half * 8;
      const u32x4 pB = u32x4{pack_bf16x2(p0[0], p0[1]), pack_bf16x2(p0[2], p0[3]), pack_bf16x2(p0[4], p0[5]), pack_bf16x2(p0[6], p0[7])};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const char* vrow = vt + ((size_t)(16 * j + r) * VP) * 4 + (half * 32 + 4 * g) * 2;
        const u32x2 va = *reinterpret_cast<const u32x2*>(vrow), vb = *reinterpret_cast<const u32x2*>(vrow + 32);
        const u32x4 av = u32x4{va[0], va[1], vb[0], vb[1]};
        if (half == 0) o[j][0] *= alpha;
        o[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&av), *reinterpret_cast<const bf16x8*>(&pB), o[j][0], 0, 0, 0);
      }
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  const float inv = 1.0f / l;
  const int ql = wave * 16 + r;
  if constexpr (TRAIN) {  // m and l are in log2 units of the scaled scores
    if (g == 0 && qi < N) lse[(size_t)bh * N + qi] = (m + log2f(l)) * 0.6931471805599453f;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) os[ql * (HD + 1) + 16 * j + 4 * g + e] = o[j][0][e] * inv;
  __syncthreads();
  psa_pe_epilogue<bf16_t, KD, HD, !TRAIN>(qkv, ld, pix0, N, W, heads, hh, qt * NQ, NQ, os, pw, pb, y, ldy);
}

template <typename T, int KD, int HD, bool TRAIN = false>
int launch_psa(const void* qkv, int ld, int n, int h, int w, int heads, float scale, const float* pw, const float* pb, void* y, int ldy,
               hipStream_t s, float* lse = nullptr) {
  auto kern = psa_attn_kernel<T, KD, HD, TRAIN>;
  if (upa_full_lds<psa_attn_kernel<T, KD, HD, TRAIN>>() != hipSuccess) {
    upa_set_error("psa_attention: could not raise the LDS limit");
    return UPA_ELAUNCH;
  }
  const int N = h * w, tiles_q = cdiv(N, 64);
  const long long grid = (long long)n * heads * tiles_q;
  if (grid > 0x7fffffffll) {
    upa_set_error("psa_attention: %lld workgroups", grid);
    return UPA_EUNSUPPORTED;
  }
  const size_t lds = psa_lds_bytes<KD, HD>();
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, s, (const T*)qkv, ld, N, w, heads, tiles_q, scale, pw,
                     pb, (T*)y, ldy, lse);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

extern "C" int upa_psa_attention(const void* qkv, int ldqkv, int n, int h, int w, int heads, int key_dim, int head_dim, float scale,
                                 const float* pe_weight, const float* pe_bias, void* y, int ldy, int dtype, void* stream) {
  UPA_CHECK_ARG(qkv && pe_weight && pe_bias && y, "psa_attention: null pointer");
  UPA_CHECK_ARG(n > 0 && h > 0 && w > 0 && heads > 0 && key_dim > 0 && head_dim > 0, "psa_attention: bad shape");
  UPA_CHECK_ARG(ldqkv >= heads * (2 * key_dim + head_dim) && ldy >= heads * head_dim, "psa_attention: strides %d / %d too small", ldqkv, ldy);
  if (dtype != UPA_F32 && dtype != UPA_BF16) {
    upa_set_error("psa_attention: dtype %d", dtype);
    return UPA_EUNSUPPORTED;
  }
  {  // y is written while v (pe's input) is still read by other workgroups
    const int es = upa_elem_size(dtype);
    const size_t np = (size_t)n * h * w;
    const char *xa = (const char*)qkv, *ya = (const char*)y;
    const size_t xb = ((np - 1) * ldqkv + heads * (2 * key_dim + head_dim)) * es, yb = ((np - 1) * ldy + heads * head_dim) * es;
    UPA_CHECK_ARG(xa + xb <= ya || ya + yb <= xa, "psa_attention: output view overlaps qkv");
  }
  hipStream_t s = (hipStream_t)stream;
  if (key_dim == 32 && head_dim == 64 && dtype == UPA_BF16 && ldqkv % 8 == 0 && ((uintptr_t)qkv % 16) == 0) {
    const int N = h * w, tiles_q = cdiv(N, 16 * PSA_MW);
    const long long grid = (long long)n * heads * tiles_q;
    if (grid <= 0x7fffffffll) {
      hipLaunchKernelGGL(psa_attn_mfma_kernel<false>, dim3((unsigned)grid), dim3(64 * PSA_MW), 0, s, (const bf16_t*)qkv, ldqkv, N, w, heads,
                         tiles_q, scale * 1.4426950408889634f, pe_weight, pe_bias, (bf16_t*)y, ldy, (float*)nullptr);
      UPA_LAUNCH_CHECK();
      return UPA_OK;
    }
  }
  if (key_dim == 32 && head_dim == 64)  // every YOLO11 scale (C2PSA: heads = c // 64, attn_ratio 0.5)
    return dtype == UPA_BF16 ? launch_psa<bf16_t, 32, 64>(qkv, ldqkv, n, h, w, heads, scale, pe_weight, pe_bias, y, ldy, s)
                             : launch_psa<float, 32, 64>(qkv, ldqkv, n, h, w, heads, scale, pe_weight, pe_bias, y, ldy, s);
  upa_set_error("psa_attention: key_dim %d / head_dim %d not supported (32 / 64)", key_dim, head_dim);
  return UPA_EUNSUPPORTED;
}

// ---- training -------------------------------------------------------------------------------------------------------------------------
// Forward for training: the same core without pe (its BatchNorm runs on batch statistics in train mode, so pe is a depthwise conv + BN
// of its own, csrc/dwconv.hip) + the row statistic lse (f32, natural log of the scaled scores' exponential sum) the backward rebuilds
// the softmax from.  The kernels are the ones above with TRAIN = true.
static int psa_check(const char* what, int n, int h, int w, int heads, int key_dim, int head_dim, int dtype) {
  if (!(n > 0 && h > 0 && w > 0 && heads > 0 && key_dim > 0 && head_dim > 0)) {
    upa_set_error("%s: bad shape", what);
    return UPA_EINVAL;
  }
  if (dtype != UPA_F32 && dtype != UPA_BF16) {
    upa_set_error("%s: dtype %d", what, dtype);
    return UPA_EUNSUPPORTED;
  }
  if (key_dim != 32 || head_dim != 64) {
    upa_set_error("%s: key_dim %d / head_dim %d not supported (32 / 64)", what, key_dim, head_dim);
    return UPA_EUNSUPPORTED;
  }
  if ((long long)n * heads * cdiv(h * w, 16) > 0x7fffffffll || (long long)h * w > 0x7fffffffll) {
    upa_set_error("%s: too many workgroups", what);
    return UPA_EUNSUPPORTED;
  }
  return UPA_OK;
}

static bool views_overlap(const void* a, size_t ab, const void* b, size_t bb) {
  const char *x = (const char*)a, *y = (const char*)b;
  return !(x + ab <= y || y + bb <= x);
}

extern "C" int upa_psa_attention_train_fwd(const void* qkv, int ldqkv, int n, int h, int w, int heads, int key_dim, int head_dim, float scale,
                                           void* o, int ldo, float* lse, int dtype, void* stream) {
  UPA_CHECK_ARG(qkv && o && lse, "psa_attention_train_fwd: null pointer");
  const int rc = psa_check("psa_attention_train_fwd", n, h, w, heads, key_dim, head_dim, dtype);
  if (rc != UPA_OK) return rc;
  UPA_CHECK_ARG(ldqkv >= heads * (2 * key_dim + head_dim) && ldo >= heads * head_dim, "psa_attention_train_fwd: strides %d / %d too small",
                ldqkv, ldo);
  const int es = upa_elem_size(dtype);
  const size_t np = (size_t)n * h * w;
  UPA_CHECK_ARG(!views_overlap(qkv, ((np - 1) * ldqkv + heads * 128) * es, o, ((np - 1) * ldo + heads * 64) * es),
                "psa_attention_train_fwd: output view overlaps qkv");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UPA_BF16 && ldqkv % 8 == 0 && ((uintptr_t)qkv % 16) == 0) {
    const int N = h * w, tiles_q = cdiv(N, 16 * PSA_MW);
    hipLaunchKernelGGL(psa_attn_mfma_kernel<true>, dim3((unsigned)(n * heads * tiles_q)), dim3(64 * PSA_MW), 0, s, (const bf16_t*)qkv, ldqkv, N, w,
                       heads, tiles_q, scale * 1.4426950408889634f, (const float*)nullptr, (const float*)nullptr, (bf16_t*)o, ldo, lse);
    UPA_LAUNCH_CHECK();
    return UPA_OK;
  }
  return dtype == UPA_BF16 ? launch_psa<bf16_t, 32, 64, true>(qkv, ldqkv, n, h, w, heads, scale, nullptr, nullptr, o, ldo, s, lse)
                           : launch_psa<float, 32, 64, true>(qkv, ldqkv, n, h, w, heads, scale, nullptr, nullptr, o, ldo, s, lse);
}

// Backward.  With P_ij = exp(scale q_i.k_j - lse_i) (the softmax rebuilt from q, k and the forward's lse), D_i = d_o_i . o_i and
// dS_ij = P_ij (d_o_i . v_j - D_i):   dv_j = sum_i P_ij d_o_i,   dq_i = scale sum_j dS_ij k_j,   dk_j = scale sum_i dS_ij q_i.
// Two launches, no atomics, every sum in an order fixed by the shapes:
//   psa_bwd_dq_kernel   a workgroup owns 64 queries (one per lane) of one (image, head) and streams the keys through LDS in blocks of 64
//                       (K, V as f32); wave `part` takes keys [16 part, 16 part + 16) of every block, the four partial dq are added in
//                       partition order through LDS.
//   psa_bwd_dkv_kernel  the transpose: a workgroup owns 64 keys, streams the queries (scale q, d_o, lse, D) in blocks of 64, wave `part`
//                       takes queries [16 part, 16 part + 16) of every block; partial (dk, dv) are added in partition order.
// Rounding points: q, k, v, o, d_o are read in their storage type (bf16 operands are exact in f32) and every product and sum is an f32
// fmaf chain in both modes - scale q is rounded once to f32, as in the forward; P, dS and D stay f32 and are never rounded to bf16; dq,
// dk, dv are rounded once, at the store (bf16 mode).  The bf16 mode does not use the matrix cores: at the 49 tokens of a 224 x 224
// classification step the pass is bound by launch latency, not by its 128 fmaf per (query, key) pair.
constexpr int PSA_BQ = 64;

template <int KD, int HD>
constexpr size_t psa_bwd_dq_lds() {
  return ((size_t)PSA_BQ * (KD + HD) + (size_t)(PSA_KP - 1) * KD * 64) * sizeof(float);
}
template <int KD, int HD>
constexpr size_t psa_bwd_dkv_lds() {
  return ((size_t)PSA_BQ * (KD + HD + 2) + (size_t)(PSA_KP - 1) * (KD + HD) * 64) * sizeof(float);
}

template <typename T>
__device__ __forceinline__ void psa_store(T* p, float v) {
  if constexpr (sizeof(T) == 4) *p = v;
  else *p = f32_to_bf16(v);
}

template <typename T, int KD, int HD>
__global__ __launch_bounds__(256) void psa_bwd_dq_kernel(const T* __restrict__ qkv, int ld, const T* __restrict__ o, int ldo,
                                                         const float* __restrict__ lse, const T* __restrict__ d_o, int lddo,
                                                         T* __restrict__ dqkv, int lddq, int N, int heads, int tiles, float scale) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  float* ks = reinterpret_cast<float*>(sm);  // [64][KD]
  float* vs = ks + PSA_BQ * KD;              // [64][HD]
  float* part_sm = vs + PSA_BQ * HD;         // [KP - 1][KD][64]
  constexpr int CH = 2 * KD + HD;
  const int tid = threadIdx.x, lane = tid & 63, part = tid >> 6;
  const int qt = blockIdx.x % tiles, bh = blockIdx.x / tiles;
  const int hh = bh % heads, b = bh / heads;
  const size_t pix0 = (size_t)b * N;
  const int cq = hh * CH, ck = cq + KD, cv = cq + 2 * KD;
  const int p = qt * 64 + lane;
  const bool valid = p < N;
  const size_t row = pix0 + (valid ? p : 0);
  float qr[KD], dq[KD], dor[HD];
  float D = 0.f;
  {
    const T* qp = qkv + row * (size_t)ld + cq;
#pragma unroll
    for (int i = 0; i < KD; ++i) {
      qr[i] = ElemTraits<T>::load(qp + i) * scale;
      dq[i] = 0.f;
    }
    const T* dp = d_o + row * (size_t)lddo + hh * HD;
    const T* op = o + row * (size_t)ldo + hh * HD;
#pragma unroll
    for (int i = 0; i < HD; ++i) {
      dor[i] = ElemTraits<T>::load(dp + i);
      D = fmaf(dor[i], ElemTraits<T>::load(op + i), D);
    }
  }
  const float L = lse[(size_t)bh * N + (valid ? p : 0)];
  constexpr int PER = PSA_BQ / PSA_KP;
  for (int k0 = 0; k0 < N; k0 += PSA_BQ) {
    __syncthreads();
    for (int i = tid; i < PSA_BQ * KD; i += 256) {
      const int key = k0 + i / KD;
      ks[i] = key < N ? ElemTraits<T>::load(qkv + (pix0 + key) * (size_t)ld + ck + i % KD) : 0.f;
    }
    for (int i = tid; i < PSA_BQ * HD; i += 256) {
      const int key = k0 + i / HD;
      vs[i] = key < N ? ElemTraits<T>::load(qkv + (pix0 + key) * (size_t)ld + cv + i % HD) : 0.f;
    }
    __syncthreads();
    const int j0 = part * PER;
    const int jn = min(PER, N - k0 - j0);
    for (int jj = 0; jj < jn; ++jj) {
      const float* kr = ks + (j0 + jj) * KD;
      const float* vr = vs + (j0 + jj) * HD;
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int i = 0; i < KD; ++i) s = fmaf(qr[i], kr[i], s);
#pragma unroll
      for (int i = 0; i < HD; ++i) dp = fmaf(dor[i], vr[i], dp);
      const float ds = expf(s - L) * (dp - D);
#pragma unroll
      for (int i = 0; i < KD; ++i) dq[i] = fmaf(ds, kr[i], dq[i]);
    }
  }
  if (part > 0) {
    float* mine = part_sm + (size_t)(part - 1) * KD * 64;
#pragma unroll
    for (int i = 0; i < KD; ++i) mine[i * 64 + lane] = dq[i];
  }
  __syncthreads();
  if (part == 0 && valid) {
    T* out = dqkv + row * (size_t)lddq + cq;
#pragma unroll
    for (int i = 0; i < KD; ++i) {
      float a = dq[i];
#pragma unroll
      for (int q_ = 1; q_ < PSA_KP; ++q_) a += part_sm[(size_t)(q_ - 1) * KD * 64 + i * 64 + lane];
      psa_store<T>(out + i, a * scale);
    }
  }
}

template <typename T, int KD, int HD>
__global__ __launch_bounds__(256) void psa_bwd_dkv_kernel(const T* __restrict__ qkv, int ld, const T* __restrict__ o, int ldo,
                                                          const float* __restrict__ lse, const T* __restrict__ d_o, int lddo,
                                                          T* __restrict__ dqkv, int lddq, int N, int heads, int tiles, float scale) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  float* qs = reinterpret_cast<float*>(sm);  // [64][KD]  scale * q
  float* ds_ = qs + PSA_BQ * KD;             // [64][HD]  d_o
  float* ls = ds_ + PSA_BQ * HD;             // [64] lse
  float* Ds = ls + PSA_BQ;                   // [64] D
  float* part_sm = Ds + PSA_BQ;              // [KP - 1][KD + HD][64]
  constexpr int CH = 2 * KD + HD;
  const int tid = threadIdx.x, lane = tid & 63, part = tid >> 6;
  const int kt = blockIdx.x % tiles, bh = blockIdx.x / tiles;
  const int hh = bh % heads, b = bh / heads;
  const size_t pix0 = (size_t)b * N;
  const int cq = hh * CH, ck = cq + KD, cv = cq + 2 * KD;
  const int p = kt * 64 + lane;
  const bool valid = p < N;
  const size_t row = pix0 + (valid ? p : 0);
  float kr[KD], vr[HD], dk[KD], dv[HD];
  {
    const T* kp = qkv + row * (size_t)ld + ck;
    const T* vp = qkv + row * (size_t)ld + cv;
#pragma unroll
    for (int i = 0; i < KD; ++i) {
      kr[i] = ElemTraits<T>::load(kp + i);
      dk[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < HD; ++i) {
      vr[i] = ElemTraits<T>::load(vp + i);
      dv[i] = 0.f;
    }
  }
  constexpr int PER = PSA_BQ / PSA_KP;
  for (int q0 = 0; q0 < N; q0 += PSA_BQ) {
    __syncthreads();
    for (int i = tid; i < PSA_BQ * KD; i += 256) {
      const int qi = q0 + i / KD;
      qs[i] = qi < N ? ElemTraits<T>::load(qkv + (pix0 + qi) * (size_t)ld + cq + i % KD) * scale : 0.f;
    }
    for (int i = tid; i < PSA_BQ * HD; i += 256) {
      const int qi = q0 + i / HD;
      ds_[i] = qi < N ? ElemTraits<T>::load(d_o + (pix0 + qi) * (size_t)lddo + hh * HD + i % HD) : 0.f;
    }
    __syncthreads();
    if (tid < PSA_BQ) {  // D of the block's queries, the same chain as psa_bwd_dq_kernel's
      const int qi = q0 + tid;
      float D = 0.f, Lq = 0.f;
      if (qi < N) {
        const T* op = o + (pix0 + qi) * (size_t)ldo + hh * HD;
        for (int i = 0; i < HD; ++i) D = fmaf(ds_[tid * HD + i], ElemTraits<T>::load(op + i), D);
        Lq = lse[(size_t)bh * N + qi];
      }
      ls[tid] = Lq;
      Ds[tid] = D;
    }
    __syncthreads();
    const int j0 = part * PER;
    const int jn = min(PER, N - q0 - j0);
    for (int jj = 0; jj < jn; ++jj) {
      const float* qr = qs + (j0 + jj) * KD;
      const float* dor = ds_ + (j0 + jj) * HD;
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int i = 0; i < KD; ++i) s = fmaf(qr[i], kr[i], s);
#pragma unroll
      for (int i = 0; i < HD; ++i) dp = fmaf(dor[i], vr[i], dp);
      const float P = expf(s - ls[j0 + jj]);
      const float dS = P * (dp - Ds[j0 + jj]);
#pragma unroll
      for (int i = 0; i < HD; ++i) dv[i] = fmaf(P, dor[i], dv[i]);
#pragma unroll
      for (int i = 0; i < KD; ++i) dk[i] = fmaf(dS, qr[i], dk[i]);  // qr carries `scale`
    }
  }
  if (part > 0) {
    float* mine = part_sm + (size_t)(part - 1) * (KD + HD) * 64;
#pragma unroll
    for (int i = 0; i < KD; ++i) mine[i * 64 + lane] = dk[i];
#pragma unroll
    for (int i = 0; i < HD; ++i) mine[(KD + i) * 64 + lane] = dv[i];
  }
  __syncthreads();
  if (part == 0 && valid) {
    T* outk = dqkv + row * (size_t)lddq + ck;
    T* outv = dqkv + row * (size_t)lddq + cv;
#pragma unroll
    for (int i = 0; i < KD; ++i) {
      float a = dk[i];
#pragma unroll
      for (int q_ = 1; q_ < PSA_KP; ++q_) a += part_sm[(size_t)(q_ - 1) * (KD + HD) * 64 + i * 64 + lane];
      psa_store<T>(outk + i, a);
    }
#pragma unroll
    for (int i = 0; i < HD; ++i) {
      float a = dv[i];
#pragma unroll
      for (int q_ = 1; q_ < PSA_KP; ++q_) a += part_sm[(size_t)(q_ - 1) * (KD + HD) * 64 + (KD + i) * 64 + lane];
      psa_store<T>(outv + i, a);
    }
  }
}

template <typename T>
static int launch_psa_bwd(const void* qkv, int ld, const void* o, int ldo, const float* lse, const void* d_o, int lddo, void* dqkv, int lddq,
                          int n, int N, int heads, float scale, hipStream_t s) {
  if (upa_full_lds<psa_bwd_dq_kernel<T, 32, 64>>() != hipSuccess || upa_full_lds<psa_bwd_dkv_kernel<T, 32, 64>>() != hipSuccess) {
    upa_set_error("psa_attention_bwd: could not raise the LDS limit");
    return UPA_ELAUNCH;
  }
  const int tiles = cdiv(N, 64);
  const dim3 grid((unsigned)(n * heads * tiles));
  hipLaunchKernelGGL((psa_bwd_dq_kernel<T, 32, 64>), grid, dim3(256), (psa_bwd_dq_lds<32, 64>()), s, (const T*)qkv, ld, (const T*)o, ldo, lse,
                     (const T*)d_o, lddo, (T*)dqkv, lddq, N, heads, tiles, scale);
  UPA_LAUNCH_CHECK();
  hipLaunchKernelGGL((psa_bwd_dkv_kernel<T, 32, 64>), grid, dim3(256), (psa_bwd_dkv_lds<32, 64>()), s, (const T*)qkv, ld, (const T*)o, ldo, lse,
                     (const T*)d_o, lddo, (T*)dqkv, lddq, N, heads, tiles, scale);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

// Nothing is staged in global memory today (D is recomputed by both passes): the query keeps the ABI of the other backward entries.
extern "C" size_t upa_psa_attention_bwd_workspace_bytes(int n, int h, int w, int heads) {
  (void)n, (void)h, (void)w, (void)heads;
  return 0;
}

extern "C" int upa_psa_attention_bwd(const void* qkv, int ldqkv, const void* o, int ldo, const float* lse, const void* d_o, int ldd_o, void* dqkv,
                                     int lddqkv, int n, int h, int w, int heads, int key_dim, int head_dim, float scale, void* ws,
                                     size_t ws_bytes, int dtype, void* stream) {
  (void)ws, (void)ws_bytes;
  UPA_CHECK_ARG(qkv && o && lse && d_o && dqkv, "psa_attention_bwd: null pointer");
  const int rc = psa_check("psa_attention_bwd", n, h, w, heads, key_dim, head_dim, dtype);
  if (rc != UPA_OK) return rc;
  UPA_CHECK_ARG(ldqkv >= heads * 128 && lddqkv >= heads * 128 && ldo >= heads * 64 && ldd_o >= heads * 64,
                "psa_attention_bwd: strides %d / %d / %d / %d too small", ldqkv, lddqkv, ldo, ldd_o);
  const int es = upa_elem_size(dtype);
  const size_t np = (size_t)n * h * w;
  const size_t qb = ((np - 1) * ldqkv + heads * 128) * es, gb = ((np - 1) * lddqkv + heads * 128) * es;
  UPA_CHECK_ARG(!views_overlap(dqkv, gb, qkv, qb) && !views_overlap(dqkv, gb, o, ((np - 1) * ldo + heads * 64) * es) &&
                    !views_overlap(dqkv, gb, d_o, ((np - 1) * ldd_o + heads * 64) * es),
                "psa_attention_bwd: dqkv overlaps an input view");
  hipStream_t s = (hipStream_t)stream;
  return dtype == UPA_BF16 ? launch_psa_bwd<bf16_t>(qkv, ldqkv, o, ldo, lse, d_o, ldd_o, dqkv, lddqkv, n, h * w, heads, scale, s)
                           : launch_psa_bwd<float>(qkv, ldqkv, o, ldo, lse, d_o, ldd_o, dqkv, lddqkv, n, h * w, heads, scale, s);
}
