// N-gram language-model rescoring of an n-best list (EXTENSION; the reference has no language model): R = B * N hypotheses -> the
// back-off log-probability of every token and of EOS behind them, their sum per hypothesis, the combination with the first pass's
// score and a length bonus, and the rank of every slot within its utterance.  The semantics are stated in the header; the table
// and the lookup are ngram.hpp's.  Two launches:
//
//   1. ngram_score_kernel: one wave per hypothesis and four per block; lane i takes positions i, i + 64, ..., one lane per position
//      for every hypothesis of up to 63 labels.  A position's table probes are independent of every other position's, so a wave
//      has up to 64 x 7 loads in flight and the block no barrier.  The lane sums its own positions in ascending order and the wave
//      adds the 64 partial sums in the fixed butterfly of wave_sum: the order depends on n[r] alone.  The same wave combines.
//      A dead slot, and every slot when lm_weight is 0, stores its zeros and reads neither ids nor the model.
//   2. ngram_rank_kernel: one wave per utterance; lane k < N ranks its slot by nbest.hpp's rule.
//
// The dead-slot rule, the fusion rule, the ranking and the limit on N are nbest.hpp's, shared with rescore.hip and ctc_beam.hip; the
// checks of the LM arguments are ngram.hpp's ngram_args, shared with ctc_beam.hip.
//
// No atomics, no allocation, no workspace, no host synchronisation: bit-reproducible, capturable.
#include "common.hpp"
#include "nbest.hpp"
#include "ngram.hpp"

namespace {

__global__ __launch_bounds__(256) void ngram_score_kernel(const int64_t* __restrict__ ids, int64_t ids_stride, const int32_t* __restrict__ n,
                                                          const float* __restrict__ base_score, const ngram_view lm,
                                                          float* __restrict__ lm_tok, float* __restrict__ lm_score,
                                                          float* __restrict__ score, int64_t R, int64_t Lp, int64_t bos, int64_t eos,
                                                          float lm_weight, float length_bonus) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;  // (wave-uniform; no barriers below)
  const int nr = n[r];
  const float bs = base_score[r];
  const bool dead = nbest_dead(bs, nr, Lp);
  float sum = 0.f;
  if (dead || lm_weight == 0.f) {  // (wave-uniform) nothing of the ids or of the model is read
    if (lm_tok)
      for (int64_t l = lane; l < Lp; l += 64) lm_tok[r * Lp + l] = 0.f;
  } else {
    const int64_t* idr = ids + r * ids_stride;
    float part = 0.f;
    for (int64_t l = lane; l < Lp; l += 64) {  // (a wave-uniform bound: every lane reaches the reduction)
      float v = 0.f;
      if (l <= (int64_t)nr) {
        const int64_t w = l < (int64_t)nr ? idr[l] : eos;
        int64_t c[NGRAM_MAX_CTX];
#pragma unroll
        for (int j = 0; j < NGRAM_MAX_CTX; ++j) c[j] = l - 1 - j >= 0 ? idr[l - 1 - j] : l - 1 - j == -1 ? bos : -1;
        v = ngram_token_logp(lm, w, c, (int)(l + 1 < NGRAM_MAX_CTX ? l + 1 : NGRAM_MAX_CTX));
        part += v;
      }
      if (lm_tok) lm_tok[r * Lp + l] = v;
    }
    sum = wave_sum(part);
  }
  if (lane == 0) {
    float sc = -INFINITY;
    if (!dead) sc = nbest_fuse(bs, sum, nr, lm_weight, length_bonus);
    lm_score[r] = dead ? -INFINITY : sum;
    score[r] = sc;
  }
}

__global__ __launch_bounds__(64) void ngram_rank_kernel(const float* __restrict__ score, int32_t* __restrict__ order, int N) {
  const int k = threadIdx.x;
  const float sc = k < N ? score[(int64_t)blockIdx.x * N + k] : -INFINITY;
  const int rank = nbest_rank(sc, k, N);
  if (k < N) order[(int64_t)blockIdx.x * N + rank] = k;
}

}  // namespace

extern "C" int js2t_ngram_rescore(const int64_t* ids, int64_t ids_stride, const int32_t* n, const float* base_score, const float* uni,
                                  const void* table, int64_t capacity, int32_t max_probe, int32_t lm_order, float* lm_tok,
                                  float* lm_score, float* score, int32_t* order, int64_t B, int32_t N, int64_t Lp, int64_t V, int64_t bos,
                                  int64_t eos, float lm_weight, float length_bonus, js2t_stream stream) {
  if (B == 0) return JS2T_OK;
  JS2T_CHECK(ids && n && base_score && lm_score && score && order, "ngram_rescore: null pointer");
  if (const int rc = nbest_list_args("ngram_rescore", B, N, Lp, ids_stride, NBEST_ROWS)) return rc;
  ngram_view lm;
  if (const int rc = ngram_args("ngram_rescore", uni, table, capacity, max_probe, lm_order, V, bos, eos, lm_weight, length_bonus, &lm)) return rc;
  const int64_t R = B * N;
  hipLaunchKernelGGL(ngram_score_kernel, dim3((unsigned)cdiv(R, 4)), dim3(256), 0, (hipStream_t)stream, ids, ids_stride, n, base_score, lm,
                     lm_tok, lm_score, score, R, Lp, bos, eos, lm_weight, length_bonus);
  JS2T_LAUNCH_CHECK();
  hipLaunchKernelGGL(ngram_rank_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, score, order, (int)N);
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}
