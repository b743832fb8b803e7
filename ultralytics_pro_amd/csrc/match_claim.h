// The claim step of match_predictions (engine/validator.py:267-308, the non-scipy branch), shared by the box matching
// (metrics.hip: upa_match_predictions) and the mask matching (segval.hip: upa_segment_match*).  A detection's best same-class label
// and best IoU do not depend on the threshold; per (label, threshold) the smallest detection index whose best label it is wins - an
// LDS atomicMin - and a detection is a true positive at threshold k iff it holds that minimum and its IoU reaches the threshold.
#pragma once
#include "common.h"

namespace {  // per translation unit, like the kernels that use it

constexpr int MP_NT = 10;  // torch.linspace(0.5, 0.95, 10), models/yolo/detect/val.py:59

struct MatchThr {
  float v[MP_NT];
};

// s_min: [M][MP_NT] ints, set to 0x7fffffff before the first round.  One round of a 256-thread workgroup: detection d (= round base +
// threadIdx.x) with best label bl (-1: none) and best IoU bi claims, the workgroup synchronises, then row d of T is written.  Rounds
// must be visited in increasing d: a later round can only lower no minimum below an index of this round.
__device__ __forceinline__ void match_claim_round(int* s_min, int d, int N, int max_det, int bl, float bi, const MatchThr& thr,
                                                  unsigned char* T) {
  if (d < N && bl >= 0)
    for (int k = 0; k < MP_NT; ++k)
      if (bi >= thr.v[k]) atomicMin(&s_min[bl * MP_NT + k], d);
  __syncthreads();
  if (d < max_det)
    for (int k = 0; k < MP_NT; ++k) T[d * MP_NT + k] = (d < N && bl >= 0 && bi >= thr.v[k] && s_min[bl * MP_NT + k] == d) ? 1 : 0;
  __syncthreads();
}

}  // namespace
