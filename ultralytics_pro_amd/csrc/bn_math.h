// The activation derivative of the BatchNorm + activation backward, shared by the element-wise passes of train.hip and the fused
// depthwise backward of dwconv.hip: both must form du = dy * act'(gamma * xhat + beta) with the same instructions.
#pragma once
#include "common.h"

// FAST (bf16 perf mode): v_exp_f32 / v_rcp_f32, 1 ulp - the operands carry 8 bits; the f32 parity mode keeps ocml expf
// and the IEEE divide.  (These element-wise passes are VALU-bound, not HBM-bound, with the accurate forms.)
template <bool FAST>
__device__ __forceinline__ float sigmoid_t(float u) {
  if constexpr (FAST) return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u * -1.44269504088896340736f));
  else return 1.0f / (1.0f + expf(-u));
}
template <bool FAST>
__device__ __forceinline__ float silu_grad(float u) {
  const float s = sigmoid_t<FAST>(u);
  return s * (1.0f + u * (1.0f - s));
}

// (train.hip) The two channel sums of the BatchNorm + activation backward: s0 = sum(du), s1 = sum(du * xhat) over the view, as
// per-block partials in ws added in block order; dbeta (+)= s0, dgamma (+)= s1; the f64 sums stay at the returned address inside ws
// ([c] s0, then [c] s1) for the pass that forms dz.  Arguments as upa_bn_act_bwd, which starts with exactly these two launches.
const double* upa_bn_bwd_sums(const void* z, const void* dy, long npix, int c, int ldz, int lddy, const float* mean, const float* var,
                              const float* gamma, const float* beta, float eps, int act, float* dgamma, float* dbeta, int accumulate,
                              double* ws, int dtype, hipStream_t s);
// (train.hip) Batch statistics from [nrows][2][ld] f32 rows of per-workgroup sums and sums of squares, added in row order.
int upa_bn_finalize_rows(const float* rows, int nrows, int ld, long npix, int c, float momentum, float* mean, float* var,
                         float* running_mean, float* running_var, void* stream);
