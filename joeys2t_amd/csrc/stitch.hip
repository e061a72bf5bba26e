// Long-form CTC (EXTENSION; the reference decodes utterances, model.py:162-166 hands out ctc_out without a consumer):
//   js2t_ctc_stitch   the kept centre frames of overlapping encoder windows -> one packed f32 posterior stream with the row
//                     statistics every CTC consumer wants (lse, arg-max, log-probability of the blank), one HBM read per logit;
//   js2t_ctc_segment  that stream cut into utterances at long blank runs: one block, ballot scans, one wave over the pauses.
// Both are bandwidth / latency bound; neither uses atomics, so the bits do not depend on the launch around them.
#include "common.hpp"
#include "row_lse.hpp"

namespace {

// ---------------------------------------------------------------- stitch
// A row passes through registers once: 128-bit loads (scalar head up to the first 16-byte boundary of the SOURCE row, scalar tail);
// each value is looked at for the maximum (any order gives the same maximum and first index, row_lse.hpp), staged in LDS as f32 -
// shifted so that the 128-bit chunks are aligned there too - and, where the DESTINATION row has the source's 16-byte phase (always
// when V and both bases are multiples of 4 elements), written out from the registers by 128-bit stores.  Otherwise the row is written
// from LDS behind the barrier, with head and tail by the destination's alignment.  The sum of exponentials then reads LDS in
// js2t_row_lse's order, which is why lse has that entry point's bits.
constexpr int ST_THREADS = ROW_LSE_THREADS;
constexpr int ST_WAVE_V = 1024;    // up to here: one wave per row, four rows per block (16 floats per lane at the limit)
constexpr int ST_MAX_V = 12000;    // one block per row; the row and the reduction's scratch stay inside 48 KB of LDS
inline int st_slot(int V) { return (V + 6) & ~3; }  // floats of LDS per row: V, at most 3 of shift, rounded to 16 bytes

template <typename T> struct st_elems;  // the elements of one 128-bit load as f32
template <> struct st_elems<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void widen(const uint4 q, float (&f)[4]) {
    f[0] = __uint_as_float(q.x); f[1] = __uint_as_float(q.y); f[2] = __uint_as_float(q.z); f[3] = __uint_as_float(q.w);
  }
};
template <> struct st_elems<uint16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void widen(const uint4 q, float (&f)[8]) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __uint_as_float(w[i] << 16);
      f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
};

// thread t of the G that own the row: load, stage at st[v + sh], take the maximum, and with `direct` write to dst
template <typename T>
__device__ __forceinline__ void st_in_row(const T* __restrict__ src, float* __restrict__ dst, float* st, int sh, bool direct, int V, int head,
                                          int t, int G, float& mx, int& mi) {
  constexpr int N = st_elems<T>::N;
  const int nvec = (V - head) / N;
  const auto one = [&](int v) {
    const float f = io<T>::ld(src + v);
    st[v + sh] = f;
    row_lse_take(f, v, mx, mi);
    if (direct) dst[v] = f;
  };
  for (int v = t; v < head; v += G) one(v);
  const uint4* s16 = (const uint4*)(src + head);
  for (int c = t; c < nvec; c += G) {
    float f[N];
    st_elems<T>::widen(s16[c], f);
    const int v0 = head + N * c;
#pragma unroll
    for (int i = 0; i < N; i += 4) {
      const float4 q = make_float4(f[i], f[i + 1], f[i + 2], f[i + 3]);
      *(float4*)(st + v0 + i + sh) = q;  // (head + sh) % 4 == 0 and the slot is 16-byte aligned
      if (direct) *(float4*)(dst + v0 + i) = q;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) row_lse_take(f[i], v0 + i, mx, mi);
  }
  for (int v = head + N * nvec + t; v < V; v += G) one(v);
}
__device__ __forceinline__ void st_out_row(const float* st, float* __restrict__ dst, int V, int t, int G) {
  const int head = min(V, (int)((4 - (((uintptr_t)dst >> 2) & 3)) & 3));
  const int nvec = (V - head) >> 2;
  for (int v = t; v < head; v += G) dst[v] = st[v];
  float4* d4 = (float4*)(dst + head);
  for (int c = t; c < nvec; c += G) {
    const float* s = st + head + 4 * c;
    d4[c] = make_float4(s[0], s[1], s[2], s[3]);
  }
  for (int v = head + 4 * nvec + t; v < V; v += G) dst[v] = st[v];
}

// G threads per row (64: a wave, 256: the block); block (x, y) = frames x * (256 / G) .. of window y.  A frame outside its window's
// keep range, or whose destination lies outside 0 .. rows - 1, is neither read nor written.
template <typename T, int G>
__global__ __launch_bounds__(ST_THREADS) void ctc_stitch_kernel(const T* __restrict__ x, const int32_t* __restrict__ keep_lo,
                                                                const int32_t* __restrict__ keep_hi, const int32_t* __restrict__ out_row,
                                                                float* __restrict__ out, float* __restrict__ lse, int64_t* __restrict__ argmax,
                                                                float* __restrict__ blank_lp, int S, int V, int slot, int64_t rows, int blank) {
  extern __shared__ float4 st_stage[];
  __shared__ float red[ROW_LSE_RED];
  __shared__ int redi[ST_THREADS / 64];
  constexpr int RPB = ST_THREADS / G;
  const int g = threadIdx.x / G, t = threadIdx.x % G;
  const int w = blockIdx.y, j = blockIdx.x * RPB + g;
  const int lo = max(keep_lo[w], 0), hi = min(keep_hi[w], S);
  const int64_t row = (int64_t)out_row[w] + (j - lo);
  const bool on = j >= lo && j < hi && row >= 0 && row < rows;  // uniform over the G threads of a row
  const T* src = x + ((int64_t)w * S + j) * V;
  float* dst = out + row * V;
  constexpr int N = st_elems<T>::N;
  const int head = min(V, (int)(((16 - ((uintptr_t)src & 15)) & 15) / sizeof(T)));  // elements up to the source's 16-byte boundary
  const int sh = (4 - (head & 3)) & 3;
  const bool direct = (((uintptr_t)(dst + head)) & 15) == 0;
  float* slot_base = (float*)st_stage + (size_t)g * slot;
  float mx = -INFINITY;
  int mi = ROW_LSE_NONE;
  if (on) st_in_row<T>(src, dst, slot_base, sh, direct, V, head, t, G, mx, mi);
  __syncthreads();
  if (!on) return;  // (G == 256: the whole block; G == 64: whole waves, and no barrier follows for them)
  const float* st = slot_base + sh;
  if (!direct) st_out_row(st, dst, V, t, G);
  const auto ld = [st](int64_t v) { return st[v]; };
  float l;
  int best;
  if constexpr (G == ST_THREADS) row_stats_block_tail(mx, mi, ld, V, red, redi, true, l, best);
  else row_stats_wave_tail(mx, mi, ld, V, t, l, best);
  if (t == 0) {
    lse[row] = l;
    argmax[row] = best;
    blank_lp[row] = st[blank] - l;
  }
}

// ---------------------------------------------------------------- segment
constexpr int SEG_THREADS = 1024, SEG_WAVES = SEG_THREADS / 64;

// Per frame one word: ((last frame <= t in the OTHER state) + 1) << 1 | silent.  It answers both scans the rule needs in O(1).
__device__ __forceinline__ int seg_last_silent(const int32_t* fr, int t) {
  const int p = fr[t];
  return (p & 1) ? t : (p >> 1) - 1;
}
__device__ __forceinline__ int seg_last_speech(const int32_t* fr, int t) {
  const int p = fr[t];
  return (p & 1) ? (p >> 1) - 1 : t;
}
__device__ __forceinline__ int seg_top(uint64_t m) { return 63 - __clzll((long long)m); }

// the pieces of the widened region [a, b): returns their count; WRITE: piece i goes to slot at + i, `end` = one past the last one
template <bool WRITE>
__device__ __forceinline__ int seg_walk(const int32_t* fr, int a, int b, int max_len, int32_t* seg_off, int64_t* seg_len, int at, int& end) {
  int n = 0, start = a;
  while (start < b) {
    int c = b;
    if (b - start > max_len) {
      const int f = seg_last_silent(fr, start + max_len - 1);  // cut behind the last silent frame of the upper half, if any
      c = f >= start + max_len / 2 ? f + 1 : start + max_len;
    }
    if (seg_last_speech(fr, c - 1) >= start) {  // (a piece of silent frames only is dropped)
      if (WRITE) {
        seg_off[at + n] = start;
        seg_len[at + n] = c - start;
        end = c;
      }
      ++n;
    }
    start = c;
  }
  return n;
}

__global__ __launch_bounds__(SEG_THREADS) void ctc_segment_kernel(const float* __restrict__ blank_lp, const int64_t* __restrict__ argmax, int T,
                                                                  int64_t blank, float thr, int min_sil, int margin, int max_len, int max_seg,
                                                                  int32_t* __restrict__ n_seg, int32_t* __restrict__ seg_off,
                                                                  int64_t* __restrict__ seg_len, int32_t* work) {
  __shared__ int w_sil[SEG_WAVES], w_non[SEG_WAVES], w_cnt[SEG_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t below = (uint64_t(1) << lane) - 1;
  int32_t* fr = work;        // [T] the per-frame words
  int32_t* pend = work + T;  // [<= T] one past the last frame of every pause, ascending

  // 1. silent bits and the last frame in the other state: ballot inside a wave, the waves before it and the chunks before through LDS
  int c_sil = -1, c_non = -1;  // last silent / speech frame of the chunks done (uniform)
  for (int base = 0; base < T; base += SEG_THREADS) {
    const int t = base + tid, wbase = base + (wv << 6);
    const bool in = t < T;
    const bool sil = in && argmax[t] == blank && blank_lp[t] >= thr;  // (NaN: not silent)
    const uint64_t m = __ballot(sil), non = __ballot(in && !sil);
    if (lane == 0) {
      w_sil[wv] = m ? wbase + seg_top(m) : -1;
      w_non[wv] = non ? wbase + seg_top(non) : -1;
    }
    __syncthreads();
    int p_sil = c_sil, p_non = c_non;
    for (int i = 0; i < SEG_WAVES; ++i) {
      if (i == wv) { p_sil = c_sil; p_non = c_non; }  // (what lies before this wave)
      c_sil = max(c_sil, w_sil[i]);
      c_non = max(c_non, w_non[i]);
    }
    if (in) {
      const uint64_t oth = (sil ? non : m) & below;
      const int last = oth ? wbase + seg_top(oth) : (sil ? p_non : p_sil);
      fr[t] = ((last + 1) << 1) | (sil ? 1 : 0);
    }
    __syncthreads();
  }

  // 2. the pauses: silent runs of at least min_sil frames, found at their last frame and compacted in order
  int n_p = 0;
  for (int base = 0; base < T; base += SEG_THREADS) {
    const int t = base + tid;
    bool e = false;
    if (t < T) {
      const int p = fr[t];
      e = (p & 1) && !(t + 1 < T && (fr[t + 1] & 1)) && t - ((p >> 1) - 1) >= min_sil;
    }
    const uint64_t m = __ballot(e);
    if (lane == 0) w_cnt[wv] = __popcll(m);
    __syncthreads();
    int off = n_p;
    for (int i = 0; i < SEG_WAVES; ++i) {
      if (i < wv) off += w_cnt[i];
      n_p += w_cnt[i];
    }
    if (e) pend[off + __popcll(m & below)] = t + 1;
    __syncthreads();
  }
  if (wv != 0) return;

  // 3. one wave, a lane per speech region (region r lies between pause r - 1 and pause r): widen, cut, count; then the same walk again
  //    behind a prefix sum of the counts, writing.  Nothing is written before the total is known to fit.
  int total = 0, base_out = 0, last_end = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int r0 = 0; r0 <= n_p; r0 += 64) {
      const int r = r0 + lane;
      int a = 0, b = 0;  // empty
      if (r <= n_p) {
        const int pa = r == 0 ? 0 : pend[r - 1], pb = r == n_p ? T : seg_last_speech(fr, pend[r] - 1) + 1;
        if (pa < pb) {
          a = pa, b = pb;
          if (r > 0) {  // the pause in front: [s, pa); one that opens the recording has no region before it to share with
            const int s = seg_last_speech(fr, pa - 1) + 1;
            a = max(pa - margin, s == 0 ? 0 : s + (pa - s) / 2);
          }
          if (r < n_p) {  // the pause behind: [pb, e)
            const int e = pend[r];
            b = min(pb + margin, e == T ? T : pb + (e - pb) / 2);
          }
        }
      }
      int end = 0;
      const int cnt = seg_walk<false>(fr, a, b, max_len, seg_off, seg_len, 0, end);
      int incl = cnt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
      }
      const int chunk = __shfl(incl, 63, 64);
      if (pass == 0) {
        total += chunk;
      } else {
        seg_walk<true>(fr, a, b, max_len, seg_off, seg_len, base_out + incl - cnt, end);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) end = max(end, __shfl_xor(end, o, 64));
        last_end = max(last_end, end);
        base_out += chunk;
      }
    }
    if (pass == 0 && total > max_seg) {
      if (lane == 0) n_seg[0] = -1;
      return;
    }
  }
  if (lane == 0) {
    n_seg[0] = total;
    seg_off[total] = last_end;
  }
}

template <typename T>
void stitch_launch(hipStream_t s, const void* x, const int32_t* lo, const int32_t* hi, const int32_t* out_row, float* out, float* lse,
                   int64_t* argmax, float* blank_lp, int64_t W, int S, int V, int64_t rows, int blank) {
  const int slot = st_slot(V);
  if (V <= ST_WAVE_V)
    hipLaunchKernelGGL((ctc_stitch_kernel<T, 64>), dim3((unsigned)cdiv(S, ST_THREADS / 64), (unsigned)W), dim3(ST_THREADS),
                       (size_t)(ST_THREADS / 64) * slot * sizeof(float), s, (const T*)x, lo, hi, out_row, out, lse, argmax, blank_lp, S, V, slot,
                       rows, blank);
  else
    hipLaunchKernelGGL((ctc_stitch_kernel<T, ST_THREADS>), dim3((unsigned)S, (unsigned)W), dim3(ST_THREADS), (size_t)slot * sizeof(float), s,
                       (const T*)x, lo, hi, out_row, out, lse, argmax, blank_lp, S, V, slot, rows, blank);
}

}  // namespace

extern "C" int js2t_ctc_stitch(const void* logits, int dt, const int32_t* keep_lo, const int32_t* keep_hi, const int32_t* out_row,
                               float* out, float* lse, int64_t* argmax, float* blank_lp, int64_t W, int64_t S, int64_t V, int64_t rows,
                               int64_t blank, js2t_stream stream) {
  JS2T_CHECK(W >= 0 && S >= 0 && rows >= 0, "ctc_stitch: negative shape");
  if (W == 0 || S == 0 || rows == 0) return JS2T_OK;
  JS2T_CHECK(logits && keep_lo && keep_hi && out_row && out && lse && argmax && blank_lp, "ctc_stitch: null pointer");
  JS2T_CHECK(dt == JS2T_F32 || dt == JS2T_BF16, "bad dtype %d", dt);
  JS2T_CHECK(V >= 1 && V <= ST_MAX_V, "ctc_stitch: V %lld outside 1 .. %d (a row is staged in LDS)", (long long)V, ST_MAX_V);
  JS2T_CHECK(blank >= 0 && blank < V, "ctc_stitch: blank %lld outside 0 .. V - 1", (long long)blank);
  JS2T_CHECK(W <= 65535 && S < (int64_t(1) << 31) && rows < (int64_t(1) << 31), "ctc_stitch: at most 65535 windows, S and rows below 2^31");
  JS2T_CHECK(((uintptr_t)logits & (dt == JS2T_F32 ? 3 : 1)) == 0 && ((uintptr_t)out & 3) == 0, "ctc_stitch: logits / out not aligned to their element");
  if (dt == JS2T_F32)
    stitch_launch<float>((hipStream_t)stream, logits, keep_lo, keep_hi, out_row, out, lse, argmax, blank_lp, W, (int)S, (int)V, rows, (int)blank);
  else
    stitch_launch<uint16_t>((hipStream_t)stream, logits, keep_lo, keep_hi, out_row, out, lse, argmax, blank_lp, W, (int)S, (int)V, rows, (int)blank);
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}

extern "C" int64_t js2t_ctc_segment_workspace_bytes(int64_t T) { return T > 0 ? 2 * T * (int64_t)sizeof(int32_t) : 0; }

extern "C" int js2t_ctc_segment(const float* blank_lp, const int64_t* argmax, int64_t T, int64_t blank, float log_threshold,
                                int32_t min_silence, int32_t margin, int32_t max_len, int32_t max_segments, int32_t* n_seg, int32_t* seg_off,
                                int64_t* seg_len, void* workspace, js2t_stream stream) {
  JS2T_CHECK(T >= 0 && T < (int64_t(1) << 30), "ctc_segment: T %lld outside 0 .. 2^30 - 1", (long long)T);
  JS2T_CHECK(n_seg && seg_off && (max_segments == 0 || seg_len) && (T == 0 || (blank_lp && argmax && workspace)), "ctc_segment: null pointer");
  JS2T_CHECK(min_silence >= 1 && margin >= 0 && max_len >= 1 && max_segments >= 0,
             "ctc_segment: 1 <= min_silence (%d), 0 <= margin (%d), 1 <= max_len (%d), 0 <= max_segments (%d) expected", (int)min_silence,
             (int)margin, (int)max_len, (int)max_segments);
  JS2T_CHECK(log_threshold == log_threshold, "ctc_segment: log_threshold is NaN");
  JS2T_CHECK(((uintptr_t)workspace & 3) == 0, "ctc_segment: workspace not aligned to 4 bytes");
  // beyond T the three lengths all mean "never" / "everything": clamped so that frame arithmetic stays inside int32
  const int Ti = (int)T, cap = Ti + 1;
  hipLaunchKernelGGL(ctc_segment_kernel, dim3(1), dim3(SEG_THREADS), 0, (hipStream_t)stream, blank_lp, argmax, Ti, blank, log_threshold,
                     min(min_silence, cap), min(margin, cap), min(max_len, cap), max_segments, n_seg, seg_off, seg_len, (int32_t*)workspace);
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}
