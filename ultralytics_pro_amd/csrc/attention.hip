// MHSA core of the BoT3 block: per (image, head) dense self-attention over the L = H*W pixels of a feature map,
//   energy[p][q] = sum_i Q[i][p] K[i][q]   (NOT scaled by 1/sqrt(d)),  attn = softmax_q(energy),
//   out[i][p]    = sum_q V[i][q] attn[p][q]                                  (+ residual, BottleneckTransformer)
// The same kernel is the core of nn.MultiheadAttention in the RT-DETR decoder (scale = 1/sqrt(d), 300 queries,
// transformer.py:670-673): there "pixels" are query tokens.
// Replaces torch.matmul / Softmax / matmul of MHSA.forward (ultralytics/nn/modules/block.py:6036-6062) and the
// `x + ...` of BottleneckTransformer.forward (:6090-6091).  q/k/v come from three 1x1 convs written into one NHWC
// buffer (channels [q | k | v]), so a (pixel, head) row is d contiguous elements.
//
// L = 400, d = 32 on the hot path (yolov5n-BoT3 @640): K and V of one (image, head) fit LDS (f32: 100 KiB, bf16: 50 KiB),
// are staged once per workgroup and broadcast-read by all lanes; one lane owns one query row and keeps a running
// (max, sum, out[d]) online softmax in registers, so the L x L energy matrix never exists in memory.
#include "common.h"

// Work split: a workgroup = 64 queries x KP key partitions (KP waves): wave `part` walks keys [part*L/KP, (part+1)*L/KP) for
// the 64 queries (one per lane) with the online softmax above; the KP partial states (max, sum, out[D]) are merged through
// LDS by wave 0 (exact: out = sum_p out_p * exp(m_p - m) / sum_p l_p * exp(m_p - m)).  With one lane walking all L keys
// (the first form) the RT-DETR self-attention (300 queries, 128 (image, head) pairs) ran 202 us on 384 two-wave workgroups.
// TRAIN (upa_mhsa_train_fwd): lse[(image * heads + head) * L + query] = log sum_keys exp(scale q.k) is written as well, from the merged
// running max and sum; the output is the same arithmetic, bit for bit.
// K / V are staged with 16-byte loads when their views are 16-byte aligned, element by element otherwise (a channel slice that starts at
// an odd element).
template <typename T, int D, int KP, bool TRAIN = false>
__global__ __launch_bounds__(64 * KP) void mhsa_kernel(const char* q, const char* k, const char* v, int ld, int L, int heads,
                                                      const char* res, int ldr, char* y, int ldy, float scale, float* lse) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  T* ks = reinterpret_cast<T*>(sm);  // [L][D]
  T* vs = ks + (size_t)L * D;        // [L][D]
  float* part_sm = reinterpret_cast<float*>(vs + (size_t)L * D);  // [KP][D + 2][64] partial states (lane-major: conflict free)
  constexpr int NT = 64 * KP;
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const size_t pix0 = (size_t)b * L;
  constexpr int E = 16 / sizeof(T);
  const bool vec = D % E == 0 && ((reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;  // (ld: 16-byte multiple)
  if (vec) {
    constexpr int G = D % E == 0 ? D / E : 1;  // 16-byte groups per row
    for (int i = threadIdx.x; i < L * G; i += NT) {
      const int p = i / G, gq = i % G;
      const size_t off = ((pix0 + p) * ld + h * D + gq * E) * sizeof(T);
      reinterpret_cast<u32x4*>(ks)[i] = *reinterpret_cast<const u32x4*>(k + off);
      reinterpret_cast<u32x4*>(vs)[i] = *reinterpret_cast<const u32x4*>(v + off);
    }
  } else {  // tiny heads (unit-test sized) and unaligned views: element-wise staging
    for (int i = threadIdx.x; i < L * D; i += NT) {
      const int p = i / D, e = i % D;
      const size_t off = ((pix0 + p) * ld + h * D + e) * sizeof(T);
      ks[i] = *reinterpret_cast<const T*>(k + off);
      vs[i] = *reinterpret_cast<const T*>(v + off);
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int p = blockIdx.y * 64 + lane;
  const bool valid = p < L;
  float qr[D], o[D];
  {
    const T* qp = reinterpret_cast<const T*>(q + ((pix0 + (valid ? p : 0)) * ld + h * D) * sizeof(T));
#pragma unroll
    for (int i = 0; i < D; ++i) {
      qr[i] = ElemTraits<T>::load(qp + i) * scale;  // nn.MultiheadAttention scales q; BoT3's MHSA passes 1.0
      o[i] = 0.f;
    }
  }
  float m = -INFINITY, l = 0.f;
  float mfin = 0.f;  // the merged maximum (TRAIN)
  const int per = (L + KP - 1) / KP;
  const int j0 = part * per, j1 = min(L, j0 + per);
  for (int j = j0; j < j1; ++j) {
    const T* kr = ks + (size_t)j * D;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i) s = fmaf(qr[i], ElemTraits<T>::load(kr + i), s);
    const float mn = fmaxf(m, s);
    const float alpha = expf(m - mn);  // exp(-inf) = 0 on the first key
    const float pj = expf(s - mn);
    l = l * alpha + pj;
    const T* vr = vs + (size_t)j * D;
#pragma unroll
    for (int i = 0; i < D; ++i) o[i] = fmaf(pj, ElemTraits<T>::load(vr + i), o[i] * alpha);
    m = mn;
  }
  if constexpr (KP > 1) {
    float* mine = part_sm + (size_t)part * (D + 2) * 64;
    mine[lane] = m;
    mine[64 + lane] = l;
#pragma unroll
    for (int i = 0; i < D; ++i) mine[(2 + i) * 64 + lane] = o[i];
    __syncthreads();
    if (part != 0) return;
    // merge in partition order (deterministic); a partition without keys carries m = -inf, l = 0
    float mm = m;
#pragma unroll
    for (int q_ = 1; q_ < KP; ++q_) mm = fmaxf(mm, part_sm[(size_t)q_ * (D + 2) * 64 + lane]);
    const float a0 = expf(m - mm);
    l *= a0;
#pragma unroll
    for (int i = 0; i < D; ++i) o[i] *= a0;
#pragma unroll
    for (int q_ = 1; q_ < KP; ++q_) {
      const float* ot = part_sm + (size_t)q_ * (D + 2) * 64;
      const float aq = expf(ot[lane] - mm);
      l += ot[64 + lane] * aq;
#pragma unroll
      for (int i = 0; i < D; ++i) o[i] = fmaf(ot[(2 + i) * 64 + lane], aq, o[i]);
    }
    mfin = mm;
  } else {
    mfin = m;
  }
  if (!valid) return;
  if constexpr (TRAIN) lse[(size_t)blockIdx.x * L + p] = mfin + logf(l);
  const float inv = 1.0f / l;
  T* yp = reinterpret_cast<T*>(y + ((pix0 + p) * ldy + h * D) * sizeof(T));
  const T* rp = res ? reinterpret_cast<const T*>(res + ((pix0 + p) * ldr + h * D) * sizeof(T)) : nullptr;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    float val = o[i] * inv;
    if (rp) val += ElemTraits<T>::load(rp + i);
    if constexpr (sizeof(T) == 4) yp[i] = val;
    else yp[i] = f32_to_bf16(val);
  }
}

// =====================================================================================================================
// bf16, d = 32 (BoT3's MHSA on the hot path: 4 heads x 32 dims, 400 keys): the same attention on the matrix cores.
// One wave owns 16 queries and walks the keys in blocks of 32 with an online softmax; both GEMMs are transposed so that a lane
// keeps ONE query for the whole walk:
//   S^T (keys x queries)  = K . Q^T   A = 16 keys x 32 dims from the K image in LDS ([key][64 B], 16-byte groups XOR-swizzled by
//                                     key >> 1: conflict-free ds_read_b128), B = the wave's 16 queries (registers, loaded once);
//                                     D: lane (g, r) holds keys 4g .. 4g + 3 of the tile for query r: the softmax statistics of a
//                                     query live in its four lanes (two butterfly steps), none cross queries;
//   O^T (dims x queries) += V^T . P^T  B = P^T: the exponentials of two S^T tiles packed to bf16 ARE a B operand (k order: keys
//                                     4g + e of the first tile, then of the second - the conv_big tail trick), A = 16 dims x those 32
//                                     keys from a TRANSPOSED V image in LDS ([dim][key], pitch = 4 mod 8 dwords: conflict-free
//                                     ds_read_b64); D: lane (g, r): dims 4g .. 4g + 3 of query r, so the running rescale
//                                     exp2(m_old - m_new) of query r multiplies registers of the lane that computed it.
// 4 MFMAs per 32 keys x 16 queries instead of ~2 k FMAs + 2 accurate expf per (query, key) on the vector ALU: 176 us -> see DESIGN.md.
// exp via v_exp_f32 on log2(e)-scaled scores (the scale of nn.MultiheadAttention folds into the same multiply), P rounded to bf16
// (the values being averaged are bf16 already); f32 accumulation, f32 residual add, one rounding of the output as before.
// =====================================================================================================================

// TRAIN: lse as in mhsa_kernel; m and l are in log2 units of the scaled scores here.
template <bool TRAIN = false>
__global__ __launch_bounds__(512) void mhsa_mfma_bf16_d32_kernel(const char* q, const char* k, const char* v, int ld, int L, int Lp, int VP,
                                                                 int heads, const char* res, int ldr, char* y, int ldy, float c_log2,
                                                                 float* lse) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  char* ks = sm;                       // [Lp][64 B]
  char* vt = sm + (size_t)Lp * 64;     // [32][VP dwords]
  const int tid = threadIdx.x, lane = tid & 63, NT = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r = lane & 15;
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const size_t pix0 = (size_t)b * L;
  // ---- K by LDS-DMA (slot i of the image = 16-byte group (i & 3) ^ swz of key i >> 2; zero page past L)
  for (int base = wave * 64; base < Lp * 4; base += NT) {
    const int i = base + lane, key = i >> 2, cg = (i & 3) ^ ((key >> 1) & 3);
    const char* src = key < L ? k + ((pix0 + key) * (size_t)ld + h * 32 + cg * 8) * 2 : reinterpret_cast<const char*>(g_zero16);
    lds_dma16(src, ks + base * 16);
  }
  // ---- V transposed: item = (key, 8 dims) -> eight 2-byte stores
  for (int i = tid; i < Lp * 4; i += NT) {
    const int key = i >> 2, dg = i & 3;
    u32x4 x = u32x4{0u, 0u, 0u, 0u};
    if (key < L) x = *reinterpret_cast<const u32x4*>(v + ((pix0 + key) * (size_t)ld + h * 32 + dg * 8) * 2);
    unsigned short* col = reinterpret_cast<unsigned short*>(vt) + key;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      col[(size_t)(dg * 8 + 2 * e) * VP * 2] = (unsigned short)(x[e] & 0xFFFFu);
      col[(size_t)(dg * 8 + 2 * e + 1) * VP * 2] = (unsigned short)(x[e] >> 16);
    }
  }
  // this wave's queries
  const int q0 = (blockIdx.y * (NT >> 6) + wave) * 16;
  const int qi = q0 + r;
  u32x4 qB = u32x4{0u, 0u, 0u, 0u};
  if (qi < L) qB = *reinterpret_cast<const u32x4*>(q + ((pix0 + qi) * (size_t)ld + h * 32 + g * 8) * 2);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (q0 >= L) return;  // (after the barrier: every wave takes part in the staging)

  float m = -INFINITY, l = 0.f;
  f32x4 o0 = f32x4{0.f, 0.f, 0.f, 0.f}, o1 = o0;
  const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
  const char* vrow0 = vt + ((size_t)r * VP + 2 * g) * 4;          // dims r / 16 + r, keys 4g .. of a block
  const char* vrow1 = vt + ((size_t)(16 + r) * VP + 2 * g) * 4;
  for (int kb = 0; kb < Lp; kb += 32) {
    const int k0 = kb + r, k1 = kb + 16 + r;
    const u32x4 a0 = *reinterpret_cast<const u32x4*>(ks + k0 * 64 + ((g ^ ((k0 >> 1) & 3)) << 4));
    const u32x4 a1 = *reinterpret_cast<const u32x4*>(ks + k1 * 64 + ((g ^ ((k1 >> 1) & 3)) << 4));
    f32x4 s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&a0), *reinterpret_cast<const bf16x8*>(&qB), z, 0, 0, 0);
    f32x4 s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&a1), *reinterpret_cast<const bf16x8*>(&qB), z, 0, 0, 0);
    // the V^T fragments of this block (independent of the softmax: issued early)
    const u32x2 v00 = *reinterpret_cast<const u32x2*>(vrow0 + kb * 2), v01 = *reinterpret_cast<const u32x2*>(vrow0 + kb * 2 + 32);
    const u32x2 v10 = *reinterpret_cast<const u32x2*>(vrow1 + kb * 2), v11 = *reinterpret_cast<const u32x2*>(vrow1 + kb * 2 + 32);
    float t[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      t[e] = s0[e] * c_log2;
      t[4 + e] = s1[e] * c_log2;
    }
    if (kb + 32 > L) {  // the last block: keys past L do not exist
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (kb + 4 * g + e >= L) t[e] = -INFINITY;
        if (kb + 16 + 4 * g + e >= L) t[4 + e] = -INFINITY;
      }
    }
    float bm = fmaxf(fmaxf(fmaxf(t[0], t[1]), fmaxf(t[2], t[3])), fmaxf(fmaxf(t[4], t[5]), fmaxf(t[6], t[7])));
    bm = fmaxf(bm, __shfl_xor(bm, 16));
    bm = fmaxf(bm, __shfl_xor(bm, 32));
    const float mn = fmaxf(m, bm);  // finite: the first block always holds a key
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    float pe[8], ps = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      pe[e] = __builtin_amdgcn_exp2f(t[e] - mn);
      ps += pe[e];
    }
    l = l * alpha + ps;
    m = mn;
    o0 *= alpha;
    o1 *= alpha;
    const u32x4 pB = u32x4{pack_bf16x2(pe[0], pe[1]), pack_bf16x2(pe[2], pe[3]), pack_bf16x2(pe[4], pe[5]), pack_bf16x2(pe[6], pe[7])};
    const u32x4 av0 = u32x4{v00[0], v00[1], v01[0], v01[1]}, av1 = u32x4{v10[0], v10[1], v11[0], v11[1]};
    o0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&av0), *reinterpret_cast<const bf16x8*>(&pB), o0, 0, 0, 0);
    o1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&av1), *reinterpret_cast<const bf16x8*>(&pB), o1, 0, 0, 0);
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (qi >= L) return;
  if constexpr (TRAIN) {
    if (g == 0) lse[(size_t)blockIdx.x * L + qi] = (m + log2f(l)) * 0.6931471805599453f;
  }
  const float inv = 1.0f / l;
  const size_t row = pix0 + qi;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const f32x4 o = j ? o1 : o0;
    float val[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) val[e] = o[e] * inv;
    const int d0 = h * 32 + 16 * j + 4 * g;
    if (res) {
      const u32x2 rv = *reinterpret_cast<const u32x2*>(res + (row * (size_t)ldr + d0) * 2);
      val[0] += __uint_as_float(rv[0] << 16); val[1] += __uint_as_float(rv[0] & 0xFFFF0000u);
      val[2] += __uint_as_float(rv[1] << 16); val[3] += __uint_as_float(rv[1] & 0xFFFF0000u);
    }
    *reinterpret_cast<u32x2*>(y + (row * (size_t)ldy + d0) * 2) = u32x2{pack_bf16x2(val[0], val[1]), pack_bf16x2(val[2], val[3])};
  }
}

template <bool TRAIN>
static int launch_mhsa_mfma(const void* q, const void* k, const void* v, int ld, int n, int hw, int heads, const void* residual, int ldr,
                            void* y, int ldy, float scale, float* lse, hipStream_t s) {
  const int Lp = (hw + 31) & ~31;
  const int VP = Lp / 2 + 4;  // dwords per V^T row: = 4 mod 8 -> the 16 rows of a ds_read_b64 half hit 16 distinct bank quads
  const size_t lds = (size_t)Lp * 64 + (size_t)32 * VP * 4;
  if (lds > 158 * 1024) return UPA_EUNSUPPORTED;
  const int tiles = cdiv(hw, 16);
  const int chunks = cdiv(tiles, 8);              // query chunks per (image, head)
  const int waves = cdiv(tiles, chunks);          // 25 tiles -> 4 chunks x 7 waves
  (void)upa_full_lds<mhsa_mfma_bf16_d32_kernel<TRAIN>>();
  hipLaunchKernelGGL(mhsa_mfma_bf16_d32_kernel<TRAIN>, dim3((unsigned)(n * heads), (unsigned)chunks), dim3(64 * waves), lds, s, (const char*)q,
                     (const char*)k, (const char*)v, ld, hw, Lp, VP, heads, (const char*)residual, ldr, (char*)y, ldy,
                     scale * 1.4426950408889634f, lse);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

template <typename T, int D, bool TRAIN>
static int launch_mhsa(const void* q, const void* k, const void* v, int ld, int n, int hw, int heads, const void* residual,
                       int ldr, void* y, int ldy, float scale, float* lse, hipStream_t s) {
  constexpr int KP = 4;
  const size_t lds = (size_t)2 * hw * D * sizeof(T) + (size_t)KP * (D + 2) * 64 * sizeof(float);
  if (lds > 158 * 1024) {
    upa_set_error("mhsa: %d keys x %d dims do not fit LDS", hw, D);
    return UPA_EUNSUPPORTED;
  }
  dim3 grid((unsigned)(n * heads), (unsigned)cdiv(hw, 64));
  auto kern = mhsa_kernel<T, D, KP, TRAIN>;
  (void)upa_full_lds<mhsa_kernel<T, D, KP, TRAIN>>();
  hipLaunchKernelGGL(kern, grid, dim3(64 * KP), lds, s, (const char*)q, (const char*)k, (const char*)v, ld, hw, heads,
                     (const char*)residual, ldr, (char*)y, ldy, scale, lse);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

static bool mhsa_aligned(const void* p, unsigned a) { return !p || (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// One dispatcher for upa_mhsa (TRAIN = false) and upa_mhsa_train_fwd: the two entries pick the same kernel for the same arguments.
template <bool TRAIN>
static int mhsa_dispatch(const void* q, const void* k, const void* v, int ldqkv, int n, int hw, int heads, int d, float scale,
                         const void* residual, int ldr, void* y, int ldy, float* lse, int dtype, hipStream_t s) {
  // the matrix-core form: LDS-DMA of K, 16-byte q / V loads, 8-byte residual / output groups
  if (dtype == UPA_BF16 && d == 32 && hw >= 16 && ldr % 4 == 0 && mhsa_aligned(q, 16) && mhsa_aligned(k, 16) && mhsa_aligned(v, 16) &&
      mhsa_aligned(y, 8) && mhsa_aligned(residual, 8)) {
    const int rc = launch_mhsa_mfma<TRAIN>(q, k, v, ldqkv, n, hw, heads, residual, ldr, y, ldy, scale, lse, s);
    if (rc != UPA_EUNSUPPORTED) return rc;
  }
#define UPA_MHSA_CASE(DD)                                                                                                        \
  if (d == DD)                                                                                                                   \
    return dtype == UPA_BF16 ? launch_mhsa<bf16_t, DD, TRAIN>(q, k, v, ldqkv, n, hw, heads, residual, ldr, y, ldy, scale, lse, s) \
                             : launch_mhsa<float, DD, TRAIN>(q, k, v, ldqkv, n, hw, heads, residual, ldr, y, ldy, scale, lse, s);
  UPA_MHSA_CASE(4)
  UPA_MHSA_CASE(8)
  UPA_MHSA_CASE(16)
  UPA_MHSA_CASE(32)
  UPA_MHSA_CASE(64)
#undef UPA_MHSA_CASE
  upa_set_error("mhsa: head dim %d not supported (4, 8, 16, 32, 64)", d);
  return UPA_EUNSUPPORTED;
}

extern "C" int upa_mhsa(const void* q, const void* k, const void* v, int ldqkv, int n, int hw, int heads, int d,
                        float scale, const void* residual, int ldr, void* y, int ldy, int dtype, void* stream) {
  UPA_CHECK_ARG(q && k && v && y, "mhsa: null pointer");
  const int es = upa_elem_size(dtype);
  UPA_CHECK_ARG(ldqkv % (16 / es) == 0 && ldy % (16 / es) == 0, "mhsa: strides must be multiples of 16 bytes");
  return mhsa_dispatch<false>(q, k, v, ldqkv, n, hw, heads, d, scale, residual, ldr, y, ldy, nullptr, dtype, (hipStream_t)stream);
}

// ---- training -------------------------------------------------------------------------------------------------------------------------
static bool mhsa_overlap(const void* a, size_t ab, const void* b, size_t bb) {
  const char *x = (const char*)a, *y = (const char*)b;
  return !(x + ab <= y || y + bb <= x);
}

static bool mhsa_dim_built(int d) { return d == 4 || d == 8 || d == 16 || d == 32 || d == 64; }

static int mhsa_train_check(const char* what, int n, int hw, int heads, int d, int dtype) {
  if (!(n > 0 && hw > 0 && heads > 0 && d > 0)) {
    upa_set_error("%s: bad shape", what);
    return UPA_EINVAL;
  }
  if (dtype != UPA_F32 && dtype != UPA_BF16) {
    upa_set_error("%s: dtype %d", what, dtype);
    return UPA_EUNSUPPORTED;
  }
  if (!mhsa_dim_built(d)) {
    upa_set_error("%s: head dim %d not supported (4, 8, 16, 32, 64)", what, d);
    return UPA_EUNSUPPORTED;
  }
  if ((long long)n * heads * cdiv(hw, 64) > 0x7fffffffll || (long long)n * heads > 0x7fffffffll) {
    upa_set_error("%s: too many workgroups", what);
    return UPA_EUNSUPPORTED;
  }
  return UPA_OK;
}

// Forward for training: upa_mhsa's kernels with TRAIN = true (the same output bits) + the row statistic lse the backward rebuilds the
// softmax from.  The whole-K/V-in-LDS forward bounds hw as upa_mhsa does (UPA_EUNSUPPORTED past it); the backward streams and has no bound.
extern "C" int upa_mhsa_train_fwd(const void* q, const void* k, const void* v, int ldqkv, int n, int hw, int heads, int d, float scale,
                                  const void* residual, int ldr, void* y, int ldy, float* lse, int dtype, void* stream) {
  UPA_CHECK_ARG(q && k && v && y && lse, "mhsa_train_fwd: null pointer");
  if (const int rc = mhsa_train_check("mhsa_train_fwd", n, hw, heads, d, dtype); rc != UPA_OK) return rc;
  const int es = upa_elem_size(dtype);
  UPA_CHECK_ARG(ldqkv % (16 / es) == 0 && ldy % (16 / es) == 0, "mhsa_train_fwd: strides must be multiples of 16 bytes");
  UPA_CHECK_ARG(ldqkv >= heads * d && ldy >= heads * d && (!residual || ldr >= heads * d), "mhsa_train_fwd: strides too small");
  const size_t np = (size_t)n * hw, ib = ((np - 1) * ldqkv + (size_t)heads * d) * es, yb = ((np - 1) * ldy + (size_t)heads * d) * es;
  // (y is written by one workgroup while others still stage K and V)
  UPA_CHECK_ARG(!mhsa_overlap(y, yb, q, ib) && !mhsa_overlap(y, yb, k, ib) && !mhsa_overlap(y, yb, v, ib) &&
                    !mhsa_overlap(y, yb, lse, np * heads * sizeof(float)),
                "mhsa_train_fwd: the output view overlaps q, k, v or lse");
  return mhsa_dispatch<true>(q, k, v, ldqkv, n, hw, heads, d, scale, residual, ldr, y, ldy, lse, dtype, (hipStream_t)stream);
}

// Backward.  With P_ij = exp(scale q_i.k_j - lse_i) (the softmax rebuilt from q, k and the forward's lse), dP_ij = d_o_i . v_j,
// D_i = sum_j P_ij dP_ij and dS_ij = P_ij (dP_ij - D_i):   dv_j = sum_i P_ij d_o_i,   dq_i = scale sum_j dS_ij k_j,   dk_j = scale sum_i dS_ij q_i.
// D is RECOMPUTED from P and d_o . v, not read as d_o . o: the forward's y carries BottleneckTransformer's residual and, in bf16, one
// rounding of the sum - subtracting the residual again would put a bf16 ulp of y into every D.  So the backward needs neither y nor the
// residual; the gradient of the residual branch is d_o itself and belongs to the caller.
// Two launches, no atomics, every sum in an order fixed by the shapes (the layout of psa.hip's backward):
//   mhsa_bwd_dq_kernel   a workgroup owns 64 queries (one per lane) of one (image, head) and streams the keys through LDS in blocks of 64
//                        (K, V as f32) TWICE: the first walk sums D (wave `part` takes keys [16 part, 16 part + 16) of every block, the
//                        four partial sums are added in partition order through LDS; D goes to the workspace for the second launch),
//                        the second walk sums dq the same way.
//   mhsa_bwd_dkv_kernel  the transpose: a workgroup owns 64 keys, streams the queries (scale q, d_o, lse, D) in blocks of 64, wave `part`
//                        takes queries [16 part, 16 part + 16) of every block; partial (dk, dv) are added in partition order.
// LDS per workgroup at d = 32 / 64: dq 40.0 / 80.0 KiB (two [64][d] f32 blocks + 3 x [d][64] partials + [4][64] D partials), dkv 64.5 /
// 128.5 KiB (two [64][d] blocks + lse / D rows + 3 x [2 d][64] partials).  Bank layout: in the walks every lane of a wave reads the SAME
// word of the staged block (a broadcast, conflict free); the partial states are lane-major ([value][lane]: 64 consecutive words per
// access); the staging writes are consecutive words (or consecutive 16-byte groups) over the workgroup.
// Staging reads 16-byte groups when the view is 16-byte aligned with a 16-byte pitch and d is a multiple of the group, single elements
// otherwise (an odd channel offset, a pitch off the group, d = 4 in bf16).
// Rounding points: q, k, v, d_o are read in their storage type (bf16 operands are exact in f32) and every product and sum is an f32 fmaf
// chain in both modes - scale q is rounded once to f32, as in the forward; P, dS and D stay f32; dq, dk, dv are rounded once, at the store.
// The bf16 mode does not use the matrix cores (DESIGN.md section 8 has the measured share of the step this pass takes).
constexpr int MHSA_BQ = 64;  // queries / keys per LDS block
constexpr int MHSA_BP = 4;   // partitions (waves) of a block

template <int D>
constexpr size_t mhsa_bwd_dq_lds() {
  return ((size_t)MHSA_BQ * 2 * D + (size_t)(MHSA_BP - 1) * D * 64 + (size_t)MHSA_BP * 64) * sizeof(float);
}
template <int D>
constexpr size_t mhsa_bwd_dkv_lds() {
  return ((size_t)MHSA_BQ * (2 * D + 2) + (size_t)(MHSA_BP - 1) * 2 * D * 64) * sizeof(float);
}

template <typename T>
__device__ __forceinline__ void mhsa_store(T* p, float v) {
  if constexpr (sizeof(T) == 4) *p = v;
  else *p = f32_to_bf16(v);
}

// dst[r][0 .. D) (f32) = mul * src[(row0 + r) * ld + 0 .. D) for r < 64, zero for rows >= rows_end
template <typename T, int D>
__device__ __forceinline__ void mhsa_stage(float* dst, const T* src, int ld, size_t row_base, int row0, int rows_end, float mul, bool vec) {
  constexpr int E = 16 / sizeof(T);
  if constexpr (D % E == 0) {
    if (vec) {
      constexpr int G = D / E;
      for (int i = threadIdx.x; i < MHSA_BQ * G; i += 256) {
        const int r = i / G, g = i % G;
        float x[E];
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = 0.f;
        if (row0 + r < rows_end) {
          const u32x4 t = *reinterpret_cast<const u32x4*>(src + (row_base + row0 + r) * (size_t)ld + g * E);
          if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = __uint_as_float(t[e]) * mul;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              x[2 * e] = __uint_as_float(t[e] << 16) * mul;
              x[2 * e + 1] = __uint_as_float(t[e] & 0xFFFF0000u) * mul;
            }
          }
        }
#pragma unroll
        for (int e = 0; e < E; e += 4) *reinterpret_cast<f32x4*>(dst + r * D + g * E + e) = f32x4{x[e], x[e + 1], x[e + 2], x[e + 3]};
      }
      return;
    }
  }
  for (int i = threadIdx.x; i < MHSA_BQ * D; i += 256) {
    const int r = i / D;
    dst[i] = row0 + r < rows_end ? ElemTraits<T>::load(src + (row_base + row0 + r) * (size_t)ld + i % D) * mul : 0.f;
  }
}

template <typename T>
__device__ __forceinline__ bool mhsa_vec_ok(const T* p, int ld) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % (16 / (int)sizeof(T)) == 0;
}

template <typename T, int D>
__global__ __launch_bounds__(256) void mhsa_bwd_dq_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, int ld,
                                                          const float* __restrict__ lse, const T* __restrict__ d_o, int lddo,
                                                          T* __restrict__ dq_out, int lddq, float* __restrict__ Dws, int L, int heads,
                                                          int tiles, float scale) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  float* ks = reinterpret_cast<float*>(sm);          // [64][D]
  float* vs = ks + MHSA_BQ * D;                      // [64][D]
  float* part_sm = vs + MHSA_BQ * D;                 // [BP - 1][D][64]
  float* dpart = part_sm + (MHSA_BP - 1) * D * 64;   // [BP][64] partial D
  const int tid = threadIdx.x, lane = tid & 63, part = tid >> 6;
  const int qt = blockIdx.x % tiles, bh = blockIdx.x / tiles;
  const int hh = bh % heads, b = bh / heads;
  const size_t pix0 = (size_t)b * L;
  const int ch = hh * D;
  const int p = qt * 64 + lane;
  const bool valid = p < L;
  const size_t row = pix0 + (valid ? p : 0);
  const bool kvec = mhsa_vec_ok(k + ch, ld), vvec = mhsa_vec_ok(v + ch, ld);
  float qr[D], dq[D], dor[D];
  {
    const T* qp = q + row * (size_t)ld + ch;
    const T* dp = d_o + row * (size_t)lddo + ch;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      qr[i] = ElemTraits<T>::load(qp + i) * scale;
      dor[i] = ElemTraits<T>::load(dp + i);
      dq[i] = 0.f;
    }
  }
  const float Lq = lse[(size_t)bh * L + (valid ? p : 0)];
  constexpr int PER = MHSA_BQ / MHSA_BP;
  float Dq = 0.f;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    for (int k0 = 0; k0 < L; k0 += MHSA_BQ) {
      __syncthreads();  // the previous block has been consumed by every wave
      mhsa_stage<T, D>(ks, k + ch, ld, pix0, k0, L, 1.f, kvec);
      mhsa_stage<T, D>(vs, v + ch, ld, pix0, k0, L, 1.f, vvec);
      __syncthreads();
      const int j0 = part * PER;
      const int jn = min(PER, L - k0 - j0);
      for (int jj = 0; jj < jn; ++jj) {
        const float* kr = ks + (j0 + jj) * D;
        const float* vr = vs + (j0 + jj) * D;
        float s = 0.f, dp = 0.f;
#pragma unroll
        for (int i = 0; i < D; ++i) s = fmaf(qr[i], kr[i], s);
#pragma unroll
        for (int i = 0; i < D; ++i) dp = fmaf(dor[i], vr[i], dp);
        const float P = expf(s - Lq);
        if (pass == 0) {
          Dq = fmaf(P, dp, Dq);
        } else {
          const float ds = P * (dp - Dq);
#pragma unroll
          for (int i = 0; i < D; ++i) dq[i] = fmaf(ds, kr[i], dq[i]);
        }
      }
    }
    if (pass == 0) {  // D of the lane's query: the four partial sums in partition order, the same value in every wave
      dpart[part * 64 + lane] = Dq;
      __syncthreads();
      Dq = dpart[lane];
#pragma unroll
      for (int q_ = 1; q_ < MHSA_BP; ++q_) Dq += dpart[q_ * 64 + lane];
      if (part == 0 && valid) Dws[(size_t)bh * L + p] = Dq;
    }
  }
  if (part > 0) {
    float* mine = part_sm + (size_t)(part - 1) * D * 64;
#pragma unroll
    for (int i = 0; i < D; ++i) mine[i * 64 + lane] = dq[i];
  }
  __syncthreads();
  if (part == 0 && valid) {
    T* out = dq_out + row * (size_t)lddq + ch;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      float a = dq[i];
#pragma unroll
      for (int q_ = 1; q_ < MHSA_BP; ++q_) a += part_sm[(size_t)(q_ - 1) * D * 64 + i * 64 + lane];
      mhsa_store<T>(out + i, a * scale);
    }
  }
}

template <typename T, int D>
__global__ __launch_bounds__(256) void mhsa_bwd_dkv_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, int ld,
                                                           const float* __restrict__ lse, const T* __restrict__ d_o, int lddo,
                                                           T* __restrict__ dk_out, T* __restrict__ dv_out, int lddq,
                                                           const float* __restrict__ Dws, int L, int heads, int tiles, float scale) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  float* qs = reinterpret_cast<float*>(sm);  // [64][D]  scale * q
  float* ds_ = qs + MHSA_BQ * D;             // [64][D]  d_o
  float* ls = ds_ + MHSA_BQ * D;             // [64] lse
  float* Ds = ls + MHSA_BQ;                  // [64] D
  float* part_sm = Ds + MHSA_BQ;             // [BP - 1][2 D][64]
  const int tid = threadIdx.x, lane = tid & 63, part = tid >> 6;
  const int kt = blockIdx.x % tiles, bh = blockIdx.x / tiles;
  const int hh = bh % heads, b = bh / heads;
  const size_t pix0 = (size_t)b * L;
  const int ch = hh * D;
  const int p = kt * 64 + lane;
  const bool valid = p < L;
  const size_t row = pix0 + (valid ? p : 0);
  const bool qvec = mhsa_vec_ok(q + ch, ld), dvec = mhsa_vec_ok(d_o + ch, lddo);
  float kr[D], vr[D], dk[D], dv[D];
  {
    const T* kp = k + row * (size_t)ld + ch;
    const T* vp = v + row * (size_t)ld + ch;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      kr[i] = ElemTraits<T>::load(kp + i);
      vr[i] = ElemTraits<T>::load(vp + i);
      dk[i] = 0.f;
      dv[i] = 0.f;
    }
  }
  constexpr int PER = MHSA_BQ / MHSA_BP;
  for (int q0 = 0; q0 < L; q0 += MHSA_BQ) {
    __syncthreads();
    mhsa_stage<T, D>(qs, q + ch, ld, pix0, q0, L, scale, qvec);
    mhsa_stage<T, D>(ds_, d_o + ch, lddo, pix0, q0, L, 1.f, dvec);
    if (tid < MHSA_BQ) {
      const int qi = q0 + tid;
      ls[tid] = qi < L ? lse[(size_t)bh * L + qi] : 0.f;
      Ds[tid] = qi < L ? Dws[(size_t)bh * L + qi] : 0.f;
    }
    __syncthreads();
    const int j0 = part * PER;
    const int jn = min(PER, L - q0 - j0);
    for (int jj = 0; jj < jn; ++jj) {
      const float* qr = qs + (j0 + jj) * D;
      const float* dor = ds_ + (j0 + jj) * D;
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int i = 0; i < D; ++i) s = fmaf(qr[i], kr[i], s);
#pragma unroll
      for (int i = 0; i < D; ++i) dp = fmaf(dor[i], vr[i], dp);
      const float P = expf(s - ls[j0 + jj]);
      const float dS = P * (dp - Ds[j0 + jj]);
#pragma unroll
      for (int i = 0; i < D; ++i) dv[i] = fmaf(P, dor[i], dv[i]);
#pragma unroll
      for (int i = 0; i < D; ++i) dk[i] = fmaf(dS, qr[i], dk[i]);  // qr carries `scale`
    }
  }
  if (part > 0) {
    float* mine = part_sm + (size_t)(part - 1) * 2 * D * 64;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      mine[i * 64 + lane] = dk[i];
      mine[(D + i) * 64 + lane] = dv[i];
    }
  }
  __syncthreads();
  if (part == 0 && valid) {
    T* outk = dk_out + row * (size_t)lddq + ch;
    T* outv = dv_out + row * (size_t)lddq + ch;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      float a = dk[i], c = dv[i];
#pragma unroll
      for (int q_ = 1; q_ < MHSA_BP; ++q_) {
        a += part_sm[(size_t)(q_ - 1) * 2 * D * 64 + i * 64 + lane];
        c += part_sm[(size_t)(q_ - 1) * 2 * D * 64 + (D + i) * 64 + lane];
      }
      mhsa_store<T>(outk + i, a);
      mhsa_store<T>(outv + i, c);
    }
  }
}

template <typename T, int D>
static int launch_mhsa_bwd(const void* q, const void* k, const void* v, int ld, const float* lse, const void* d_o, int lddo, void* dq, void* dk,
                           void* dv, int lddq, float* Dws, int n, int L, int heads, float scale, hipStream_t s) {
  if (upa_full_lds<mhsa_bwd_dq_kernel<T, D>>() != hipSuccess || upa_full_lds<mhsa_bwd_dkv_kernel<T, D>>() != hipSuccess) {
    upa_set_error("mhsa_bwd: could not raise the LDS limit");
    return UPA_ELAUNCH;
  }
  const int tiles = cdiv(L, 64);
  const dim3 grid((unsigned)(n * heads * tiles));
  hipLaunchKernelGGL((mhsa_bwd_dq_kernel<T, D>), grid, dim3(256), (mhsa_bwd_dq_lds<D>()), s, (const T*)q, (const T*)k, (const T*)v, ld, lse,
                     (const T*)d_o, lddo, (T*)dq, lddq, Dws, L, heads, tiles, scale);
  UPA_LAUNCH_CHECK();
  hipLaunchKernelGGL((mhsa_bwd_dkv_kernel<T, D>), grid, dim3(256), (mhsa_bwd_dkv_lds<D>()), s, (const T*)q, (const T*)k, (const T*)v, ld, lse,
                     (const T*)d_o, lddo, (T*)dk, (T*)dv, lddq, (const float*)Dws, L, heads, tiles, scale);
  UPA_LAUNCH_CHECK();
  return UPA_OK;
}

// D (one f32 per (image, head, query)) travels from the dq launch to the dk / dv launch through the workspace.
extern "C" size_t upa_mhsa_bwd_workspace_bytes(int n, int hw, int heads) {
  if (n <= 0 || hw <= 0 || heads <= 0) return 0;
  return (size_t)n * hw * heads * sizeof(float);
}

extern "C" int upa_mhsa_bwd(const void* q, const void* k, const void* v, int ldqkv, const float* lse, const void* d_o, int ldd_o, void* dq,
                            void* dk, void* dv, int lddqkv, int n, int hw, int heads, int d, float scale, void* ws, size_t ws_bytes,
                            int dtype, void* stream) {
  UPA_CHECK_ARG(q && k && v && lse && d_o && dq && dk && dv, "mhsa_bwd: null pointer");
  if (const int rc = mhsa_train_check("mhsa_bwd", n, hw, heads, d, dtype); rc != UPA_OK) return rc;
  const int C = heads * d;
  UPA_CHECK_ARG(ldqkv >= C && lddqkv >= C && ldd_o >= C, "mhsa_bwd: strides %d / %d / %d too small", ldqkv, lddqkv, ldd_o);
  const size_t need = upa_mhsa_bwd_workspace_bytes(n, hw, heads);
  UPA_CHECK_ARG(ws && ws_bytes >= need && ((uintptr_t)ws & 3) == 0, "mhsa_bwd: workspace too small (%zu < %zu bytes) or unaligned", ws_bytes, need);
  const size_t es = (size_t)upa_elem_size(dtype);
  UPA_CHECK_ARG(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)d_o | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) % es == 0,
                "mhsa_bwd: a view is not aligned to its element");
  const size_t np = (size_t)n * hw;
  const size_t ib = ((np - 1) * ldqkv + C) * es, ob = ((np - 1) * lddqkv + C) * es, db = ((np - 1) * ldd_o + C) * es;
  const void* outs[3] = {dq, dk, dv};
  for (int i = 0; i < 3; ++i) {
    UPA_CHECK_ARG(!mhsa_overlap(outs[i], ob, q, ib) && !mhsa_overlap(outs[i], ob, k, ib) && !mhsa_overlap(outs[i], ob, v, ib) &&
                      !mhsa_overlap(outs[i], ob, d_o, db) && !mhsa_overlap(outs[i], ob, lse, np * heads * sizeof(float)) &&
                      !mhsa_overlap(outs[i], ob, ws, need),
                  "mhsa_bwd: a gradient view overlaps an input view or the workspace");
  }
  hipStream_t s = (hipStream_t)stream;
#define UPA_MHSA_BWD_CASE(DD)                                                                                                              \
  if (d == DD)                                                                                                                             \
    return dtype == UPA_BF16                                                                                                               \
               ? launch_mhsa_bwd<bf16_t, DD>(q, k, v, ldqkv, lse, d_o, ldd_o, dq, dk, dv, lddqkv, (float*)ws, n, hw, heads, scale, s)       \
               : launch_mhsa_bwd<float, DD>(q, k, v, ldqkv, lse, d_o, ldd_o, dq, dk, dv, lddqkv, (float*)ws, n, hw, heads, scale, s);
  UPA_MHSA_BWD_CASE(4)
  UPA_MHSA_BWD_CASE(8)
  UPA_MHSA_BWD_CASE(16)
  UPA_MHSA_BWD_CASE(32)
  UPA_MHSA_BWD_CASE(64)
#undef UPA_MHSA_BWD_CASE
  return UPA_EUNSUPPORTED;  // (unreachable: mhsa_train_check)
}
