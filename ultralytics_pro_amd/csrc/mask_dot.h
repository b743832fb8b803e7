// The two pieces of process_mask (ultralytics/utils/ops.py:489-545) that fix a mask pixel's value, shared by every kernel that
// assembles masks (segment.hip: upa_process_mask; segval.hip: upa_segment_match) so that their bits cannot drift apart:
//  - `masks_in @ protos` of one pixel: an nm-deep dot product, k ascending, one fma per term;
//  - crop_mask's float-comparison form on the `boxes * ratios` products (the branch the reference takes on a GPU, ops.py:510-513).
#pragma once
#include "common.h"

// coef: nm floats (LDS or global); pr: the pixel's nm proto channels, 16-byte aligned, nm a multiple of 16 bytes
__device__ __forceinline__ float mask_dot_bf16(const float* coef, const bf16_t* pr, int nm) {
  float acc = 0.f;
  for (int k = 0; k < nm; k += 8) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(pr + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc = fmaf(coef[k + 2 * e], __uint_as_float(v[e] << 16), acc);
      acc = fmaf(coef[k + 2 * e + 1], __uint_as_float(v[e] & 0xffff0000u), acc);
    }
  }
  return acc;
}

__device__ __forceinline__ float mask_dot_f32(const float* coef, const float* pr, int nm) {
  float acc = 0.f;
  for (int k = 0; k < nm; k += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(pr + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = fmaf(coef[k + e], v[e], acc);
  }
  return acc;
}

// (cx1, cy1, cx2, cy2) = box * (ratio_x, ratio_y, ratio_x, ratio_y) as f32 products; pixel (fx, fy) as floats
__device__ __forceinline__ bool mask_in_crop(float fx, float fy, float cx1, float cy1, float cx2, float cy2) {
  return fx >= cx1 && fx < cx2 && fy >= cy1 && fy < cy2;
}
