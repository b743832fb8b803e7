// Relative error of the two exponentials csrc/psa.hip calls, against float64, over the arguments its online softmax can form
// (always <= 0: a score minus a running maximum): `expf` (the scalar kernels) and `__builtin_amdgcn_exp2f` = v_exp_f32 (the
// matrix-core kernel, on log2(e)-scaled scores).  tests/yolo11_kernel_ref.py records the result next to EXPF_REL / EXP2_REL.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off tools/experiments/exp_error.hip -o tools/experiments/exp_error && tools/experiments/exp_error
//
// Samples: 2^28 evenly spaced arguments in [-LO, 0] and, to cover the neighbourhood of 0 as densely in relative terms, 2^22 mantissas
// for each of the 40 binades of magnitude 2^-40 .. 1.  Results below 2^-126 (where f32 has no relative precision, and v_exp_f32 may flush)
// are reported as an absolute error instead.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#define CK(x)                                                                      \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                 \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

template <int FN>
__device__ __forceinline__ float f32_exp(float x) {
  if constexpr (FN == 0) return expf(x);
  else return __builtin_amdgcn_exp2f(x);
}
template <int FN>
__device__ __forceinline__ double f64_exp(double x) {
  if constexpr (FN == 0) return exp(x);
  else return exp2(x);
}

// out[0]: max relative error (float bits) over normal results, out[1]: max absolute error over results below 2^-126
template <int FN>
__global__ void sweep(float lo, unsigned n_lin, unsigned n_man, unsigned* out) {
  float rel = 0.f, ab = 0.f;
  const unsigned total = n_lin + 40u * n_man;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    float x;
    if (i < n_lin) {
      x = -lo * (((float)i + 0.5f) / (float)n_lin);
    } else {
      const unsigned j = i - n_lin, bin = j / n_man, m = j - bin * n_man;
      x = -ldexpf(1.0f + (float)m / (float)n_man, -(int)bin - 1);
    }
    const float y = f32_exp<FN>(x);
    const double r = f64_exp<FN>((double)x);
    const double d = fabs((double)y - r);
    if (r >= 0x1p-126) rel = fmaxf(rel, (float)(d / r));
    else ab = fmaxf(ab, (float)d);
  }
  atomicMax(out, __float_as_uint(rel));  // non-negative floats order as their bit patterns
  atomicMax(out + 1, __float_as_uint(ab));
}

template <int FN>
__global__ void specials(float* out) {
  out[0] = f32_exp<FN>(0.0f);
  out[1] = f32_exp<FN>(-INFINITY);
  out[2] = f32_exp<FN>(-0.0f);
}

template <int FN>
static int run(const char* name, float lo) {
  unsigned* d;
  float* s;
  CK(hipMalloc(&d, 8));
  CK(hipMalloc(&s, 12));
  CK(hipMemset(d, 0, 8));
  hipLaunchKernelGGL(sweep<FN>, dim3(4096), dim3(256), 0, 0, lo, 1u << 28, 1u << 22, d);
  hipLaunchKernelGGL(specials<FN>, dim3(1), dim3(1), 0, 0, s);
  CK(hipDeviceSynchronize());
  unsigned h[2];
  float sp[3];
  CK(hipMemcpy(h, d, 8, hipMemcpyDeviceToHost));
  CK(hipMemcpy(sp, s, 12, hipMemcpyDeviceToHost));
  float rel, ab;
  std::memcpy(&rel, &h[0], 4);
  std::memcpy(&ab, &h[1], 4);
  std::printf("%s on [-%g, 0]: max relative error %.6g = %.4f * 2^-24 (results >= 2^-126); max absolute error below that %.3g = 2^%.1f; "
              "f(0) = %.9g, f(-inf) = %.9g, f(-0) = %.9g\n",
              name, lo, rel, rel * 0x1p24, ab, ab > 0 ? std::log2(ab) : -999.0, sp[0], sp[1], sp[2]);
  CK(hipFree(d));
  CK(hipFree(s));
  return 0;
}

int main() {
  if (run<0>("expf", 130.0f)) return 1;
  if (run<1>("v_exp_f32 (exp2)", 190.0f)) return 1;
  return 0;
}
