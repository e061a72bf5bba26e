// The rules the n-best entry points share (EXTENSION; the reference has no n-best list): js2t_ctc_beam_search(_lm, _ctx) writes the list,
// js2t_rescore, js2t_ngram_rescore, js2t_context_rescore and js2t_mbr_rescore re-rank it, js2t_nbest_confidence votes over it, and they compose because each of
// these rules exists once, here: the limit on N, the shape a list may have (nbest_list_args, host), the dead slot, the ranking, the fused score, the hash.
// The semantics are stated in the header; rescore.hip, ngram.hip, context.hip, ctc_beam.hip, mbr.hip and confidence.hip are the files that apply them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "common.hpp"

constexpr int NBEST_MAX_N = 32;  // slots of one utterance: one lane each, half a wave

// The shape of a list an entry point takes, refused through JS2T_CHECK's path: N in 1 .. NBEST_MAX_N, Lp >= 1 positions (labels and EOS) per row,
// rows of ids at least Lp - 1 apart, and B small enough for what the entry point's grids and 32-bit offsets count beside the B * NBEST_MAX_N slots -
// NBEST_ROWS: the B * N * Lp positions; NBEST_PAIRS (quadratic in N; B may be 0): the B * N * N pairs; NBEST_SLOTS: nothing more.
enum nbest_extent { NBEST_SLOTS, NBEST_ROWS, NBEST_PAIRS };
inline int nbest_list_args(const char* who, int64_t B, int32_t N, int64_t Lp, int64_t ids_stride, nbest_extent extent) {
  JS2T_CHECK(N >= 1 && N <= NBEST_MAX_N, "%s: N %d outside 1..%d", who, (int)N, NBEST_MAX_N);
  JS2T_CHECK(Lp >= 1, "%s: Lp %lld below 1", who, (long long)Lp);
  JS2T_CHECK(ids_stride >= Lp - 1, "%s: ids_stride %lld below Lp - 1 (%lld)", who, (long long)ids_stride, (long long)(Lp - 1));
  if (extent == NBEST_PAIRS)
    JS2T_CHECK(B >= 0 && B < (int64_t(1) << 31) / (N * N), "%s: bad shape (B %lld, N %d: B * N * N must stay below 2^31)", who, (long long)B, (int)N);
  else
    JS2T_CHECK(B > 0 && B < (int64_t(1) << 31) / NBEST_MAX_N && Lp < (int64_t(1) << 31) && (extent == NBEST_SLOTS || B * N * Lp < (int64_t(1) << 31)),
               "%s: bad shape (B %lld, Lp %lld)", who, (long long)B, (long long)Lp);
  return JS2T_OK;
}

// a slot that holds no hypothesis: no score, or a length that does not fit the Lp positions (labels and EOS) of its row
__device__ __forceinline__ bool nbest_dead(float score, int n, int64_t Lp) { return score == -INFINITY || n < 0 || (int64_t)n > Lp - 1; }

// rank of lane k's score among lanes 0 .. N-1 of its wave, by counting: the larger score first, equal scores in slot order, a NaN
// as -inf - so the ranks of the N lanes are a permutation whatever the data.  Every lane of the wave calls it (N is wave-uniform,
// a lane >= N passes -inf); no barrier.
__device__ __forceinline__ int nbest_rank(float score, int k, int N) {
  const float key = score == score ? score : -INFINITY;
  int rank = 0;
  for (int j = 0; j < N; ++j) {  // (wave-uniform bounds)
    const float kj = __shfl(key, j, 64);
    rank += (kj > key || (kj == key && j < k)) ? 1 : 0;
  }
  return rank;
}

// base + lm_weight * lm + length_bonus * len, each product rounded to f32 and added in that order; a term of weight 0 is left
// out, not multiplied (an lm of -inf or NaN does not reach the score then)
__device__ __forceinline__ float nbest_fuse(float base, float lm, int len, float lm_weight, float length_bonus) {
#pragma clang fp contract(off)
  float s = base;
  if (lm_weight != 0.f) s += lm_weight * lm;
  if (length_bonus != 0.f) s += length_bonus * (float)len;
  return s;
}

// nbest_fuse with the context term (js2t_ctc_beam_search_ctx, js2t_context_rescore): base + lm_weight * lm + context_weight *
// (float)count + length_bonus * len under the same rules - and with context_weight == 0 it is nbest_fuse, bit for bit.  The count is
// an integer: exact in f32 whatever the order it was summed in.
__device__ __forceinline__ float nbest_fuse_ctx(float base, float lm, int count, int len, float lm_weight, float context_weight,
                                                float length_bonus) {
#pragma clang fp contract(off)
  float s = base;
  if (lm_weight != 0.f) s += lm_weight * lm;
  if (context_weight != 0.f) s += context_weight * (float)count;
  if (length_bonus != 0.f) s += length_bonus * (float)len;
  return s;
}

// the finaliser of splitmix64, a bijection of 64-bit words: the n-gram table's home slot and the beam's prefix hash
__host__ __device__ __forceinline__ uint64_t nbest_fmix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
