// Edit distances on the device and minimum-Bayes-risk ranking of an n-best list (EXTENSION; the reference has neither): the
// decision that minimises the expected label error over the list instead of the one with the highest score.  The semantics are
// stated in the header; the distance itself is editdist.hpp's wave_edit_distance.
//
//   js2t_edit_distance: one launch, edit_rows_kernel - one wave per pair of rows and four per block.
//   js2t_mbr_rescore: two launches.
//     1. mbr_pairs_kernel: one wave per (utterance, i < j) pair of slots and four per block; the wave computes the pair once and
//        stores (i, j) and (j, i), so the matrix is symmetric by construction.  A pair with a dead member stores its -1s and reads
//        no ids.
//     2. mbr_risk_kernel: one wave per utterance, lane k = slot k: the diagonal, the posterior (maximum by the wave, the sum in
//        ascending slot order), the risk (ascending j, no contraction) and the rank by nbest.hpp's rule on the key -risk.
//
// The dead-slot rule of the list, the ranking and the limit on N are nbest.hpp's, shared with rescore.hip, ngram.hip and
// ctc_beam.hip; a score that is no log mass (NaN, +inf) makes a slot dead here as well (posterior.hpp, shared with confidence.hip).
//
// No atomics, no allocation, no workspace beyond `dist`, no host synchronisation: bit-reproducible, capturable.
#include "common.hpp"
#include "nbest.hpp"
#include "posterior.hpp"
#include "editdist.hpp"

namespace {

__global__ __launch_bounds__(256) void edit_rows_kernel(const int64_t* __restrict__ a, int64_t a_stride, const int32_t* __restrict__ a_len,
                                                        const int64_t* __restrict__ b, int64_t b_stride, const int32_t* __restrict__ b_len,
                                                        int32_t* __restrict__ dist, int64_t R, int64_t group, int a_max, int b_max) {
  __shared__ uint16_t bnd[4][EDIT_CELLS];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t r = (int64_t)blockIdx.x * 4 + w;
  if (r >= R) return;  // (wave-uniform; no barriers below)
  const int64_t rb = r / group;
  const int na = __builtin_amdgcn_readfirstlane(a_len[r]), nb = __builtin_amdgcn_readfirstlane(b_len[rb]);
  int d = -1;
  if (na >= 0 && nb >= 0 && na <= a_max && nb <= b_max) d = wave_edit_distance(a + r * a_stride, na, b + rb * b_stride, nb, bnd[w]);
  if ((threadIdx.x & 63) == 0) dist[r] = d;
}

__global__ __launch_bounds__(256) void mbr_pairs_kernel(const int64_t* __restrict__ ids, int64_t ids_stride, const int32_t* __restrict__ n,
                                                        const float* __restrict__ score, int32_t* __restrict__ dist, int64_t pairs, int N,
                                                        int64_t Lp) {
  __shared__ uint16_t bnd[4][EDIT_CELLS];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t q = (int64_t)blockIdx.x * 4 + w;
  if (q >= pairs) return;  // (wave-uniform; no barriers below)
  const int P = N * (N - 1) / 2;
  const int64_t u = q / P;
  int p = (int)(q - u * P), i = 0;
  while (p >= N - 1 - i) p -= N - 1 - i, ++i;  // pair p of the utterance, rows of the upper triangle in order
  const int j = i + 1 + p;
  const int64_t ri = u * N + i, rj = u * N + j;
  const int ni = __builtin_amdgcn_readfirstlane(n[ri]), nj = __builtin_amdgcn_readfirstlane(n[rj]);
  int d = -1;
  if (!mbr_dead(score[ri], ni, Lp) && !mbr_dead(score[rj], nj, Lp))
    d = wave_edit_distance(ids + ri * ids_stride, ni, ids + rj * ids_stride, nj, bnd[w]);
  if ((threadIdx.x & 63) == 0) {
    dist[ri * N + j] = d;
    dist[rj * N + i] = d;
  }
}

__global__ __launch_bounds__(64) void mbr_risk_kernel(const int32_t* __restrict__ n, const float* __restrict__ score, int32_t* __restrict__ dist,
                                                      float* __restrict__ posterior, float* __restrict__ risk, int32_t* __restrict__ order,
                                                      int N, int64_t Lp, float scale) {
#pragma clang fp contract(off)
  const int k = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * N + k;
  const float sc = k < N ? score[r] : -INFINITY;
  const bool live = k < N && !mbr_dead(sc, n[r], Lp);
  const unsigned long long live_mask = __ballot(live);
  const float pk = nbest_posterior(sc, live, N, scale);  // (posterior.hpp: the one statement of it)
  float rk = live ? 0.f : INFINITY;
  for (int j = 0; j < N; ++j) {  // (wave-uniform bounds)
    const float pj = __shfl(pk, j, 64);
    if (live && ((live_mask >> j) & 1) && j != k) rk += pj * (float)dist[r * N + j];
  }
  const int rank = nbest_rank(-rk, k, N);
  if (k < N) {
    dist[r * N + k] = live ? 0 : -1;
    posterior[r] = pk;
    risk[r] = rk;
    order[(int64_t)blockIdx.x * N + rank] = k;
  }
}

}  // namespace

extern "C" int js2t_edit_max_len(void) { return JS2T_EDIT_MAX_LEN; }

extern "C" int js2t_edit_distance(const int64_t* a, int64_t a_stride, const int32_t* a_len, const int64_t* b, int64_t b_stride,
                                  const int32_t* b_len, int32_t* dist, int64_t R, int64_t group, int64_t a_max, int64_t b_max, js2t_stream stream) {
  JS2T_CHECK(group >= 1, "edit_distance: group %lld below 1", (long long)group);
  JS2T_CHECK(a_max >= 0 && a_max <= JS2T_EDIT_MAX_LEN && b_max >= 0 && b_max <= JS2T_EDIT_MAX_LEN, "edit_distance: a_max %lld / b_max %lld outside 0..%d",
             (long long)a_max, (long long)b_max, JS2T_EDIT_MAX_LEN);
  JS2T_CHECK(R >= 0 && R < (int64_t(1) << 31), "edit_distance: bad R %lld", (long long)R);
  JS2T_CHECK(a_stride >= 0 && b_stride >= 0, "edit_distance: negative stride (%lld, %lld)", (long long)a_stride, (long long)b_stride);
  if (R == 0) return JS2T_OK;
  JS2T_CHECK(a_len && b_len && dist && (a || a_max == 0) && (b || b_max == 0), "edit_distance: null pointer");
  hipLaunchKernelGGL(edit_rows_kernel, dim3((unsigned)cdiv(R, 4)), dim3(256), 0, (hipStream_t)stream, a, a_stride, a_len, b, b_stride, b_len,
                     dist, R, group, (int)a_max, (int)b_max);
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}

extern "C" int js2t_mbr_rescore(const int64_t* ids, int64_t ids_stride, const int32_t* n, const float* score, int32_t* dist,
                                float* posterior, float* risk, int32_t* order, int64_t B, int32_t N, int64_t Lp, float scale,
                                js2t_stream stream) {
  if (const int rc = posterior_args("mbr_rescore", Lp, scale, "an edit distance")) return rc;
  if (const int rc = nbest_list_args("mbr_rescore", B, N, Lp, ids_stride, NBEST_PAIRS)) return rc;
  if (B == 0) return JS2T_OK;
  JS2T_CHECK(n && score && dist && posterior && risk && order && (ids || Lp == 1), "mbr_rescore: null pointer");
  const int64_t pairs = B * (N * (N - 1) / 2);
  if (pairs) {
    hipLaunchKernelGGL(mbr_pairs_kernel, dim3((unsigned)cdiv(pairs, 4)), dim3(256), 0, (hipStream_t)stream, ids, ids_stride, n, score, dist,
                       pairs, (int)N, Lp);
    JS2T_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(mbr_risk_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, n, score, dist, posterior, risk, order, (int)N, Lp,
                     scale);
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}
