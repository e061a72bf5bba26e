// Token confidence from an n-best list (EXTENSION; the reference has no n-best list): the posterior mass of the list entries that
// agree with a hypothesis at each of its tokens.  The semantics are stated in the header; the alignment itself is editalign.hpp's
// wave_edit_align, the posterior posterior.hpp's - the statement js2t_mbr_rescore uses.
//
//   js2t_nbest_confidence: two launches.
//     1. conf_pairs_kernel: one wave per (utterance, pivot, slot) and four per block, no block barrier.  The wave aligns the pivot's
//        row (always the row `a` of the rule) with the slot's and stores the pivot's match mask, ceil((Lp - 1) / 32) words, in the
//        workspace; with `match` it expands the mask into bytes as well.  The pivot against itself is all ones without a DP; a dead
//        slot, and every slot of a dead pivot, stores zeros and reads no ids.
//     2. conf_sum_kernel: one wave per (utterance, pivot).  Lane k = slot k for the posterior, then lane = token position: the
//        votes are added over the live slots in ascending order, no contraction.  The wave of pivot 0 stores the utterance's
//        posterior.
//
// Workspace: [pairs][mask words] u32, then [pairs][align_code_words(Lp - 1)] u32 for the 2-bit direction codes of each pair's table
// (a table of one tile and at most 256 rows keeps them in LDS and leaves its region untouched).
//
// No atomics, no allocation, no host synchronisation: bit-reproducible, capturable.
#include "common.hpp"
#include "nbest.hpp"
#include "posterior.hpp"
#include "editalign.hpp"

namespace {

__global__ __launch_bounds__(256) void conf_pairs_kernel(const int64_t* __restrict__ ids, int64_t ids_stride, const int32_t* __restrict__ n,
                                                         const float* __restrict__ score, const int32_t* __restrict__ pivot,
                                                         uint32_t* __restrict__ masks, uint32_t* codes, uint8_t* __restrict__ match,
                                                         int64_t pairs, int N, int P, int64_t Lp, int words, int64_t code_words) {
  __shared__ __align__(16) uint16_t bnd[4][EDIT_CELLS];  // per wave: the boundary column, or the codes of a table that fits (editalign.hpp)
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + w;
  if (q >= pairs) return;  // (wave-uniform; no barriers below)
  const int64_t bp = q / N, b = bp / P;
  const int j = (int)(q - bp * N);
  const int pv = __builtin_amdgcn_readfirstlane(pivot[bp]);
  uint32_t mask = 0u;
  if (pv >= 0 && pv < N) {  // (a pivot outside the list is dead: nothing of it is read)
    const int64_t ra = b * N + pv, rj = b * N + j;
    const int na = __builtin_amdgcn_readfirstlane(n[ra]);
    if (!mbr_dead(score[ra], na, Lp)) {
      if (j == pv) {
        mask = align_range_bits(lane, 0, na);
      } else {
        const int nj = __builtin_amdgcn_readfirstlane(n[rj]);
        if (!mbr_dead(score[rj], nj, Lp))
          mask = wave_edit_align(ids + ra * ids_stride, na, ids + rj * ids_stride, nj, bnd[w], codes + q * code_words);
      }
    }
  }
  if (lane < words) masks[q * words + lane] = mask;
  if (match) {
    for (int64_t l0 = 0; l0 < Lp - 1; l0 += 64) {  // (wave-uniform bounds: all lanes reach the shuffle)
      const int64_t l = l0 + lane;
      const uint32_t mw = (uint32_t)__shfl((int)mask, (int)(l >> 5) & 63, 64);
      if (l < Lp - 1) match[q * (Lp - 1) + l] = (uint8_t)((mw >> (l & 31)) & 1u);
    }
  }
}

__global__ __launch_bounds__(64) void conf_sum_kernel(const int32_t* __restrict__ n, const float* __restrict__ score,
                                                      const int32_t* __restrict__ pivot, const uint32_t* __restrict__ masks,
                                                      float* __restrict__ posterior, float* __restrict__ conf, float* __restrict__ hyp_conf,
                                                      int N, int P, int64_t Lp, int words, float scale) {
#pragma clang fp contract(off)
  const int k = threadIdx.x;
  const int64_t bp = blockIdx.x, b = bp / P;
  const int64_t r = b * N + k;
  const float sc = k < N ? score[r] : -INFINITY;
  const bool live = k < N && !mbr_dead(sc, n[r], Lp);
  const unsigned long long live_mask = __ballot(live);
  const float pk = nbest_posterior(sc, live, N, scale);
  if (bp - b * P == 0 && k < N) posterior[r] = pk;
  const int pv = __builtin_amdgcn_readfirstlane(pivot[bp]);
  const bool pivot_live = pv >= 0 && pv < N && ((live_mask >> pv) & 1);
  const float ppv = __shfl(pk, pivot_live ? pv : 0, 64);
  if (k == 0) hyp_conf[bp] = pivot_live ? ppv : 0.f;
  for (int64_t l0 = 0; l0 < Lp - 1; l0 += 64) {  // (wave-uniform bounds)
    const int64_t l = l0 + k;
    float c = 0.f;
    for (int j = 0; j < N; ++j) {
      const float pj = __shfl(pk, j, 64);
      if (((live_mask >> j) & 1) && l < Lp - 1) {
        const uint32_t mw = masks[(bp * N + j) * words + (l >> 5)];
        c += pj * (float)((mw >> (l & 31)) & 1u);
      }
    }
    if (l < Lp - 1) conf[bp * (Lp - 1) + l] = c;
  }
}

bool conf_shape_ok(int64_t B, int32_t P, int32_t N, int64_t Lp) {
  return N >= 1 && N <= NBEST_MAX_N && P >= 1 && P <= N && Lp >= 1 && Lp - 1 <= JS2T_EDIT_MAX_LEN && B >= 0 && B < (int64_t(1) << 31) / (N * N);
}

}  // namespace

extern "C" int64_t js2t_nbest_confidence_workspace(int64_t B, int32_t P, int32_t N, int64_t Lp) {
  if (!conf_shape_ok(B, P, N, Lp)) return -1;
  return B * P * N * (align_mask_words(Lp - 1) + align_code_words(Lp - 1)) * (int64_t)sizeof(uint32_t);
}

extern "C" int js2t_nbest_confidence(const int64_t* ids, int64_t ids_stride, const int32_t* n, const float* score, const int32_t* pivot,
                                     float* posterior, float* conf, float* hyp_conf, uint8_t* match, void* workspace,
                                     int64_t workspace_bytes, int64_t B, int32_t N, int32_t P, int64_t Lp, float scale, js2t_stream stream) {
  if (const int rc = posterior_args("nbest_confidence", Lp, scale, "an alignment")) return rc;
  if (const int rc = nbest_list_args("nbest_confidence", B, N, Lp, ids_stride, NBEST_PAIRS)) return rc;
  JS2T_CHECK(P >= 1 && P <= N, "nbest_confidence: P %d outside 1..N (%d)", (int)P, (int)N);
  const int64_t need = js2t_nbest_confidence_workspace(B, P, N, Lp);
  JS2T_CHECK(workspace_bytes >= need, "nbest_confidence: workspace of %lld bytes below the %lld that B %lld, P %d, N %d, Lp %lld need",
             (long long)workspace_bytes, (long long)need, (long long)B, (int)P, (int)N, (long long)Lp);
  if (B == 0) return JS2T_OK;
  JS2T_CHECK(n && score && pivot && posterior && hyp_conf && (conf || Lp == 1) && (ids || Lp == 1) && (workspace || need == 0),
             "nbest_confidence: null pointer");
  JS2T_CHECK(((uintptr_t)workspace & 3) == 0, "nbest_confidence: workspace not aligned to 4 bytes");
  const int64_t pairs = B * P * N;
  const int words = (int)align_mask_words(Lp - 1);
  uint32_t* masks = (uint32_t*)workspace;
  hipLaunchKernelGGL(conf_pairs_kernel, dim3((unsigned)cdiv(pairs, 4)), dim3(256), 0, (hipStream_t)stream, ids, ids_stride, n, score, pivot, masks,
                     masks + pairs * words, match, pairs, (int)N, (int)P, Lp, words, align_code_words(Lp - 1));
  JS2T_LAUNCH_CHECK();
  hipLaunchKernelGGL(conf_sum_kernel, dim3((unsigned)(B * P)), dim3(64), 0, (hipStream_t)stream, n, score, pivot, (const uint32_t*)masks, posterior,
                     conf, hyp_conf, (int)N, (int)P, Lp, words, scale);
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}
