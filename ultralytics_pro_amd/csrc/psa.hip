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
template <typename T, int KD, int HD>
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
    float acc = pb[c];
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
    const float val = os[ql * (HD + 1) + j] + acc;
    T* yp = y + (pix0 + pq) * (size_t)ldy + c;
    if constexpr (sizeof(T) == 4) *yp = val;
    else *yp = f32_to_bf16(val);
  }
}

template <typename T, int KD, int HD>
__global__ __launch_bounds__(256) void psa_attn_kernel(const T* __restrict__ qkv, int ld, int N, int W, int heads, int tiles_q, float scale,
                                                       const float* __restrict__ pw, const float* __restrict__ pb, T* __restrict__ y, int ldy) {
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
  }
  __syncthreads();
  psa_pe_epilogue<T, KD, HD>(qkv, ld, pix0, N, W, heads, hh, qt * 64, 64, os, pw, pb, y, ldy);
}

// bf16, KD = 32, HD = 64 on the matrix cores (see the top of the file).  Requires ld % 8 == 0 and a 16-byte aligned qkv.
__global__ __launch_bounds__(64 * PSA_MW) void psa_attn_mfma_kernel(const bf16_t* __restrict__ qkv, int ld, int N, int W, int heads, int tiles_q,
                                                                   float c_log2, const float* __restrict__ pw, const float* __restrict__ pb,
                                                                   bf16_t* __restrict__ y, int ldy) {
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
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) os[ql * (HD + 1) + 16 * j + 4 * g + e] = o[j][0][e] * inv;
  __syncthreads();
  psa_pe_epilogue<bf16_t, KD, HD>(qkv, ld, pix0, N, W, heads, hh, qt * NQ, NQ, os, pw, pb, y, ldy);
}

template <typename T, int KD, int HD>
int launch_psa(const void* qkv, int ld, int n, int h, int w, int heads, float scale, const float* pw, const float* pb, void* y, int ldy,
               hipStream_t s) {
  auto kern = psa_attn_kernel<T, KD, HD>;
  if (upa_full_lds<psa_attn_kernel<T, KD, HD>>() != hipSuccess) {
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
                     pb, (T*)y, ldy);
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
      hipLaunchKernelGGL(psa_attn_mfma_kernel, dim3((unsigned)grid), dim3(64 * PSA_MW), 0, s, (const bf16_t*)qkv, ldqkv, N, w, heads, tiles_q,
                         scale * 1.4426950408889634f, pe_weight, pe_bias, (bf16_t*)y, ldy);
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
