// The row statistics of js2t_row_lse - maximum, first index of the maximum, log-sum-exp - stated once for every kernel that has to
// give the same BITS for the same f32 row (js2t_row_lse itself, js2t_ctc_stitch).
//
// The order of the sum is the contract: 256 accumulators, accumulator t adds exp(x[v] - max) for v = t, t + 256, ... in
// ascending v; each group of 64 accumulators is folded by wave_sum's butterfly; the four group sums are added in the order
// (((0 + g0) + g1) + g2) + g3; lse = max + log(sum).  A block of 256 threads keeps one accumulator per thread (row_stats_block*); one
// wave keeps four per lane, lane l those of t = l, l + 64, l + 128, l + 192 (row_stats_wave_tail) - the same additions in the same order.
#pragma once
#include "common.hpp"

constexpr int ROW_LSE_THREADS = 256;
constexpr int ROW_LSE_NONE = 0x7fffffff;  // "no maximum seen" (an empty accumulator, or a row of -inf / NaN only)

// The maximum and the first index that reaches it do not depend on the order the elements are looked at, so a caller may find
// them over any split of the row (js2t_ctc_stitch does while it loads) and hand them to the *_tail forms below.  Element (f, v)
// into the running pair: strictly greater replaces, an equal value keeps the lower index; NaN and a first -inf change nothing.
__device__ __forceinline__ void row_lse_take(float f, int v, float& mx, int& mi) {
  if (f > mx || (f == mx && v < mi && mi != ROW_LSE_NONE)) { mx = f; mi = v; }
}
// accumulator t, first pass: its maximum and the first index that reaches it (ascending v: strictly greater alone keeps the first)
template <typename Ld>
__device__ __forceinline__ void row_lse_max(Ld ld, int64_t V, int t, float& mx, int& mi) {
  for (int64_t v = t; v < V; v += ROW_LSE_THREADS) {
    const float f = ld(v);
    if (f > mx) { mx = f; mi = (int)v; }
  }
}
// accumulator t, second pass: THE ORDER OF THIS SUM IS THE CONTRACT
template <typename Ld>
__device__ __forceinline__ float row_lse_expsum(Ld ld, int64_t V, int t, float bmx) {
  float s = 0.f;
  for (int64_t v = t; v < V; v += ROW_LSE_THREADS) s += __expf(ld(v) - bmx);
  return s;
}
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// One row per block of ROW_LSE_THREADS threads, all of which call this (it holds two barriers); red: __shared__ float
// [ROW_LSE_RED], redi: __shared__ int [ROW_LSE_THREADS / 64], used once per kernel - the maxima, the sums and the indices each have
// their own words, so no barrier is spent on protecting a reuse; (mx, mi): the thread's share of the maximum search, the shares
// covering the row.  Every thread gets lse and, with want_argmax, the first index of the maximum.
constexpr int ROW_LSE_RED = 2 * ROW_LSE_THREADS / 64;
template <typename Ld>
__device__ __forceinline__ void row_stats_block_tail(float mx, int mi, Ld ld, int64_t V, float* red, int* redi, bool want_argmax, float& lse,
                                                     int& best) {
  constexpr int NW = ROW_LSE_THREADS / 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float wmx = wave_max(mx);
  if (lane == 0) red[wv] = wmx;
  __syncthreads();
  float bmx = -INFINITY;
#pragma unroll
  for (int i = 0; i < NW; ++i) bmx = fmaxf(bmx, red[i]);
  const float ws = wave_sum(row_lse_expsum(ld, V, threadIdx.x, bmx));
  const int cand = want_argmax ? wave_min_int((mx == bmx) ? mi : ROW_LSE_NONE) : ROW_LSE_NONE;
  if (lane == 0) {
    red[NW + wv] = ws;
    redi[wv] = cand;
  }
  __syncthreads();
  float s = 0.f;
  best = ROW_LSE_NONE;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    s += red[NW + i];  // (((0 + g0) + g1) + g2) + g3
    best = min(best, redi[i]);
  }
  lse = bmx + __logf(s);
}
template <typename Ld>
__device__ __forceinline__ void row_stats_block(Ld ld, int64_t V, float* red, int* redi, bool want_argmax, float& lse, int& best) {
  float mx = -INFINITY;
  int mi = ROW_LSE_NONE;
  row_lse_max(ld, V, threadIdx.x, mx, mi);
  row_stats_block_tail(mx, mi, ld, V, red, redi, want_argmax, lse, best);
}

// One row per wave, (mx, mi) the lane's share; every lane gets the results.  No barrier, no LDS of its own.
template <typename Ld>
__device__ __forceinline__ void row_stats_wave_tail(float mx, int mi, Ld ld, int64_t V, int lane, float& lse, int& best) {
  const float bmx = wave_max(mx);
  float s = 0.f;
#pragma unroll
  for (int g = 0; g < ROW_LSE_THREADS / 64; ++g) s += wave_sum(row_lse_expsum(ld, V, lane + 64 * g, bmx));
  best = wave_min_int((mx == bmx) ? mi : ROW_LSE_NONE);
  lse = bmx + __logf(s);
}
