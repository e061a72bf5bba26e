// Attention rescoring of an n-best list (EXTENSION; the reference has no consumer of ctc_out, model.py:162-166): the teacher-forced
// decoder logits of R = B * N hypotheses -> the log-probability of every gold token, their sum per hypothesis, the combination with
// the CTC score and the rank of every slot within its utterance.  The semantics are stated in the header.  Two launches:
//
//   1. rescore_tok_kernel: one wave per (hypothesis, position) row and four rows per block, the pattern of loss.hip's
//      xent_fwd_wave_kernel - one pass of 16-byte loads with an online maximum and sum per lane, wave reductions only, no barrier.  A
//      wave whose position lies behind the hypothesis' length, or whose slot is dead, stores its 0 and returns without a load.
//      The gold id comes from the beam kernel's id table and the length (EOS at position n), never from a sentinel id.
//      The row is walked in chunks of 16 bytes, chunk c by lane c % 64.  A row whose address is 16-byte aligned loads its full chunks
//      with one instruction each; any other row (a V that is no multiple of the chunk, a view at an odd offset) loads the same
//      chunks element by element, and so does the tail chunk of every row.  Both forms feed the same arithmetic in the same order:
//      the bits do not depend on the alignment.
//   2. rescore_rank_kernel: one wave per utterance; lane k < N sums its slot's token log-probabilities in ascending position, combines
//      and ranks by nbest.hpp's rule.
//
// The dead-slot rule, the ranking and the limit on N are nbest.hpp's, shared with ngram.hip and ctc_beam.hip.
//
// No atomics, no allocation, no workspace, no host synchronisation: bit-reproducible, capturable.
#include "common.hpp"
#include "nbest.hpp"

namespace {

template <typename T> struct rs_chunk;  // E elements = 16 bytes
template <> struct rs_chunk<float> {
  static constexpr int E = 4;
  static __device__ __forceinline__ void ld16(const float* p, float (&q)[4]) {
    const float4 v = *(const float4*)p;
    q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
  }
};
template <> struct rs_chunk<uint16_t> {
  static constexpr int E = 8;
  static __device__ __forceinline__ void ld16(const uint16_t* p, float (&q)[8]) {
    const uint4 v = *(const uint4*)p;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) q[2 * i] = __uint_as_float(w[i] << 16), q[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
};

template <typename T>
__global__ __launch_bounds__(256) void rescore_tok_kernel(const T* __restrict__ x, const int64_t* __restrict__ ids, int64_t ids_stride,
                                                          const int32_t* __restrict__ n, const float* __restrict__ ctc_score,
                                                          float* __restrict__ tok_lp, int64_t rows, int64_t Lp, int64_t V, int64_t eos) {
#pragma clang fp contract(off)  // the 16-byte and the element-wise walk must round alike: no fused multiply-add in one of them only
  constexpr int E = rs_chunk<T>::E;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // (no barriers below)
  const int64_t r = row / Lp, l = row - r * Lp;
  const int nr = n[r];
  if (nbest_dead(ctc_score[r], nr, Lp) || l > (int64_t)nr) {  // (wave-uniform) nothing of this row is read
    if (lane == 0) tok_lp[row] = 0.f;
    return;
  }
  const int64_t g = l < (int64_t)nr ? ids[r * ids_stride + l] : eos;
  if (g < 0 || g >= V) {
    if (lane == 0) tok_lp[row] = -INFINITY;
    return;
  }
  const T* xr = x + row * V;
  const bool vec = ((uintptr_t)xr & 15) == 0;
  const int nfull = (int)(V / E), nchunk = (int)((V + E - 1) / E);
  float m = -INFINITY, s = 0.f;
  auto take = [&](const float (&q)[E]) {
#pragma clang fp contract(off)
    float m4 = q[0];
#pragma unroll
    for (int i = 1; i < E; ++i) m4 = fmaxf(m4, q[i]);
    if (m4 > m) {
      s *= __expf(m - m4);  // (m = -inf: s is 0 and stays 0)
      m = m4;
    }
    const float mm = m == -INFINITY ? 0.f : m;  // a chunk of -inf adds 0; a NaN element makes s NaN
    float e[E];
#pragma unroll
    for (int i = 0; i < E; ++i) e[i] = __expf(q[i] - mm);
#pragma unroll
    for (int st = 1; st < E; st *= 2)
#pragma unroll
      for (int i = 0; i < E; i += 2 * st) e[i] += e[i + st];
    s += e[0];
  };
  auto take_scalar = [&](int c) {  // chunk c element by element; behind V: -inf
    float q[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int64_t v = (int64_t)c * E + i;
      q[i] = v < V ? io<T>::ld(xr + v) : -INFINITY;
    }
    take(q);
  };
  int c = lane;
  if (vec) {
    for (; c + 448 < nfull; c += 512) {  // eight 16-byte loads in flight per lane
      float q[8][E];
#pragma unroll
      for (int i = 0; i < 8; ++i) rs_chunk<T>::ld16(xr + (int64_t)(c + 64 * i) * E, q[i]);
#pragma unroll
      for (int i = 0; i < 8; ++i) take(q[i]);
    }
    for (; c + 192 < nfull; c += 256) {
      float q[4][E];
#pragma unroll
      for (int i = 0; i < 4; ++i) rs_chunk<T>::ld16(xr + (int64_t)(c + 64 * i) * E, q[i]);
#pragma unroll
      for (int i = 0; i < 4; ++i) take(q[i]);
    }
    for (; c < nfull; c += 64) {
      float q[E];
      rs_chunk<T>::ld16(xr + (int64_t)c * E, q);
      take(q);
    }
  }
  for (; c < nchunk; c += 64) take_scalar(c);  // every chunk of an unaligned row; the tail chunk of an aligned one
  const float bmx = wave_max(m);
  s = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - bmx));
  if (lane == 0) tok_lp[row] = io<T>::ld(xr + g) - (bmx + logf(s));
}

__global__ __launch_bounds__(64) void rescore_rank_kernel(const int32_t* __restrict__ n, const float* __restrict__ ctc_score,
                                                          const float* __restrict__ tok_lp, float* __restrict__ att_score,
                                                          float* __restrict__ score, int32_t* __restrict__ order, int N, int64_t Lp,
                                                          float w) {
  const int k = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * N + k;
  float sc = -INFINITY;
  if (k < N) {
    const float cs = ctc_score[r];
    const int nr = n[r];
    float att = -INFINITY;
    if (!nbest_dead(cs, nr, Lp)) {
      att = 0.f;
      const float* tp = tok_lp + r * Lp;
      for (int l0 = 0; l0 <= nr; l0 += 8) {  // eight independent loads at a time; the additions in ascending l, one fixed order
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = l0 + i <= nr ? tp[l0 + i] : 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (l0 + i <= nr) att += v[i];
      }
      sc = w == 1.f ? cs : w == 0.f ? att : w * cs + (1.f - w) * att;  // a term of weight 0 is left out, not multiplied
    }
    att_score[r] = att;
    score[r] = sc;
  }
  const int rank = nbest_rank(sc, k, N);  // (every lane: a lane >= N holds -inf)
  if (k < N) order[(int64_t)blockIdx.x * N + rank] = k;
}

}  // namespace

extern "C" int js2t_rescore(const void* logits, int dt, const int64_t* ids, int64_t ids_stride, const int32_t* n, const float* ctc_score,
                            float* tok_lp, float* att_score, float* score, int32_t* order, int64_t B, int32_t N, int64_t Lp, int64_t V,
                            int64_t eos, float ctc_weight, js2t_stream stream) {
  if (B == 0) return JS2T_OK;
  JS2T_CHECK(logits && ids && n && ctc_score && tok_lp && att_score && score && order, "rescore: null pointer");
  if (const int rc = nbest_list_args("rescore", B, N, Lp, ids_stride, NBEST_ROWS)) return rc;
  JS2T_CHECK(V >= 2 && V < 0x7fffffff, "rescore: V %lld outside 2..2^31-2", (long long)V);
  JS2T_CHECK(eos >= 0 && eos < V, "rescore: eos %lld outside the vocabulary", (long long)eos);
  JS2T_CHECK(ctc_weight >= 0.f && ctc_weight <= 1.f, "rescore: ctc_weight %g outside [0, 1]", (double)ctc_weight);  // (NaN fails too)
  JS2T_CHECK(dt == JS2T_F32 || dt == JS2T_BF16, "bad dtype %d", dt);
  const int64_t rows = B * N * Lp;
  if (dt == JS2T_F32)
    hipLaunchKernelGGL(rescore_tok_kernel<float>, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, (const float*)logits, ids,
                       ids_stride, n, ctc_score, tok_lp, rows, Lp, V, eos);
  else
    hipLaunchKernelGGL(rescore_tok_kernel<uint16_t>, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)logits, ids, ids_stride, n, ctc_score, tok_lp, rows, Lp, V, eos);
  JS2T_LAUNCH_CHECK();
  hipLaunchKernelGGL(rescore_rank_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, n, ctc_score, tok_lp, att_score, score, order,
                     (int)N, Lp, ctc_weight);
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}
