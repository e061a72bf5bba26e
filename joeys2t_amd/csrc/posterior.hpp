// The posterior of an n-best list (EXTENSION; the reference has no n-best list): which slots carry mass and what share of it, stated
// once for the two entry points that need it - js2t_mbr_rescore (mbr.hip) weighs distances with it, js2t_nbest_confidence
// (confidence.hip) weighs votes.  The semantics are stated in the header above js2t_mbr_rescore.
#pragma once
#include "common.hpp"
#include "nbest.hpp"
#include "editdist.hpp"

// what the two entry points ask beyond the list's shape, in front of it (a row too long for the table would also fail the stride rule, and this says
// why): rows an edit table takes - `what` names the table in the error - and a scale that is finite and above 0
inline int posterior_args(const char* who, int64_t Lp, float scale, const char* what) {
  JS2T_CHECK(Lp - 1 <= JS2T_EDIT_MAX_LEN, "%s: Lp - 1 = %lld above the longest row %s takes (%d)", who, (long long)(Lp - 1), what, JS2T_EDIT_MAX_LEN);
  JS2T_CHECK(scale > 0.f && scale <= 3.402823466e38f, "%s: scale %g not finite and above 0", who, (double)scale);  // (a NaN fails too)
  return JS2T_OK;
}

// a slot without posterior mass: dead by the rule of the list, or a score that is no log mass (NaN, +inf)
__device__ __forceinline__ bool mbr_dead(float score, int n, int64_t Lp) { return nbest_dead(score, n, Lp) || score != score || score == INFINITY; }

// Lane k = slot k of ONE utterance; every lane of the wave calls it (N wave-uniform; a lane >= N, or a dead slot, passes live =
// false).  z = scale * score rounded, the maximum by the wave, e = exp(z - max) and exactly 1 at the maximum, S summed in ascending
// slot order (a dead slot adds an exact 0), p = e / S; 0 for a lane that is not live.
__device__ __forceinline__ float nbest_posterior(float score, bool live, int N, float scale) {
#pragma clang fp contract(off)
  const float z = live ? scale * score : -INFINITY;
  const float m = wave_max(z);
  const float e = live ? (z == m ? 1.f : expf(z - m)) : 0.f;
  float S = 0.f;
  for (int j = 0; j < N; ++j) S += __shfl(e, j, 64);  // ascending slot order (a dead slot adds an exact 0)
  return live ? e / S : 0.f;
}
