// The rules the n-best entry points share (EXTENSION; the reference has no n-best list): js2t_ctc_beam_search(_lm, _ctx) writes the list,
// js2t_rescore, js2t_ngram_rescore, js2t_context_rescore and js2t_mbr_rescore re-rank it, and they compose because each of these rules exists once, here.
// The semantics are stated in the header; rescore.hip, ngram.hip, context.hip, ctc_beam.hip and mbr.hip are the files that apply them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

constexpr int NBEST_MAX_N = 32;  // slots of one utterance: one lane each, half a wave

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
