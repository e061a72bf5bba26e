// CTC forced alignment (EXTENSION; the reference has no aligner): the best path through the extended label sequence of the CTC
// loss (loss.hip) - the alpha recursion with max in place of logaddexp, 2-bit back-pointers, and the back-trace in the same launch.
// One block per utterance, like the loss: the recursion is a chain of T dependent steps, and so is the back-trace (one back-pointer
// read per frame) - which is why the back-pointers stay in LDS whenever those of the utterance fit, and go to the caller's
// workspace in HBM only when they do not.  No atomics anywhere: two runs give the same bits.
#include "common.hpp"

namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_MAX_S = 1024;           // limit on 2 * Lmax + 1: the one of js2t_ctc_alpha (loss.hip CTC_MAX_S)
constexpr int AL_CHUNK_FLOATS = 8192;    // block form: emission staging, 32 KB of LDS
constexpr int ALW_S = 192;               // one-wave form: 2 * Lmax + 1 <= 192 (loss.hip CTCW_S)
constexpr int ALW_CHUNK = 32;            // time steps staged per chunk: 2 x 32 x 192 floats = 48 KB of LDS
constexpr int AL_BP_LDS_BYTES = 88 * 1024;  // most LDS the back-pointers of one utterance may take (beside <= 52 KB of staging)

// Back-pointers: code 0 = stay, 1 = from s-1, 2 = from s-2; word (t >> 4) * S + s holds the codes of state s at frames
// 16 (t >> 4) .. + 15, two bits each, frame t at bits 2 (t & 15).  The thread that owns a state collects sixteen frames in a
// register and stores the word once: every word (g, s < S) with 16 g < T_b is written, none is ever read-modified.
// All LDS is dynamic (one extern array, carved below): fixed part + the back-pointer words the launch was given.

// a predecessor replaces the best so far only if STRICTLY greater (tie rule of the header: stay, s-1, s-2)
__device__ __forceinline__ void al_take(float& best, uint32_t& code, float cand, uint32_t c) {
  if (cand > best) { best = cand; code = c; }
}

// thread 0: final state by the tie rule, then T_b dependent back-pointer reads; path row written with plain stores
__device__ __forceinline__ void al_backtrace(const uint32_t* bp, int S, int64_t Tb, int s, int32_t* __restrict__ prow) {
  for (int64_t t = Tb - 1; t >= 0; --t) {
    prow[t] = s;
    if (t > 0) s -= (int)((bp[(t >> 4) * S + s] >> (2 * (int)(t & 15))) & 3u);
  }
}

// all threads, parallel over t: frame log-probabilities and token spans from the path row (written by thread 0 before the barrier
// in front of this call); frames behind the length, unused token slots and infeasible utterances get their fill values
template <typename T>
__device__ __forceinline__ void al_outputs(const T* __restrict__ x, const float* __restrict__ lse, const int* ext, int64_t r0, int64_t V,
                                           int64_t Tmax, int64_t Tb, int L, int64_t Lmax, bool ok, int32_t* prow, int32_t* __restrict__ ts,
                                           int32_t* __restrict__ te, float* __restrict__ fl) {
  for (int64_t t = threadIdx.x; t < Tmax; t += AL_THREADS) {
    if (ok && t < Tb) {
      const int s = prow[t];
      const int lab = ext[s];
      fl[t] = (lab >= 0 && lab < V) ? io<T>::ld(x + (r0 + t) * V + lab) - lse[r0 + t] : -INFINITY;
      if (s & 1) {  // a label state: every one is visited, in one run of frames (a skip goes from label to label)
        if (t == 0 || prow[t - 1] != s) ts[s >> 1] = (int32_t)t;
        if (t == Tb - 1 || prow[t + 1] != s) te[s >> 1] = (int32_t)t + 1;
      }
    } else {
      prow[t] = -1;
      fl[t] = 0.f;
    }
  }
  for (int64_t l = (ok ? L : 0) + threadIdx.x; l < Lmax; l += AL_THREADS) { ts[l] = -1; te[l] = -1; }
}

// thread 0 after the recursion: fin = v_{T_b - 1}(0 .. S-1).  Returns through ok_s whether the utterance has a path at all.
// (inlined at two call sites, one per home of the back-pointers, so that the chain of reads is LDS reads where they are in LDS)
__device__ __forceinline__ void al_finish(const float* fin, const uint32_t* bp, int S, int64_t Tb, int32_t* __restrict__ prow,
                                          float* __restrict__ score_b, int* ok_s) {
  int s = S - 1;
  if (S > 1 && fin[S - 2] > fin[S - 1]) s = S - 2;
  const float sc = fin[s];
  const bool ok = sc > -INFINITY;  // (not NaN either)
  *score_b = ok ? sc : -INFINITY;
  *ok_s = ok ? 1 : 0;
  if (ok) al_backtrace(bp, S, Tb, s, prow);
}

// ---------------------------------------------------------------- one-wave form: 2 Lmax + 1 <= 192
// ctc_wave_kernel's shape (loss.hip): wave 0 runs the recursion with three states per lane in registers, neighbours by lane
// shuffle; waves 1..3 gather the emissions of the next chunk of time steps into LDS meanwhile.
template <typename T>
__global__ __launch_bounds__(AL_THREADS) void ctc_align_wave_kernel(
    const T* __restrict__ x, const float* __restrict__ lse, const int64_t* __restrict__ targets, const int64_t* __restrict__ in_len,
    const int64_t* __restrict__ tgt_len, int32_t* __restrict__ path, int32_t* __restrict__ tok_start, int32_t* __restrict__ tok_end,
    float* __restrict__ frame_logp, float* __restrict__ score, uint32_t* __restrict__ ws, int64_t ws_words, int bp_lds_words, int64_t Tmax,
    int64_t V, int64_t Lmax, int64_t blank, const int32_t* __restrict__ rowoff) {
  extern __shared__ __align__(16) unsigned char al_lds[];
  float(*em)[ALW_CHUNK * ALW_S] = (float(*)[ALW_CHUNK * ALW_S])al_lds;   // [2][...]
  int* ext = (int*)(al_lds + 2 * ALW_CHUNK * ALW_S * 4);                  // [ALW_S + 2]
  float* fin = (float*)(ext + ALW_S + 2);                                 // [ALW_S]
  int* ok_s = (int*)(fin + ALW_S);                                        // [2]
  uint32_t* bp_lds = (uint32_t*)(ok_s + 2);                               // [bp_lds_words]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t Tb = min(in_len[b], Tmax);
  const int L = (int)max((int64_t)0, min(tgt_len[b], Lmax));
  const int S = 2 * L + 1;
  const int64_t r0 = rowoff ? (int64_t)rowoff[b] : (int64_t)b * Tmax;  // first logits / lse row of the utterance
  int32_t* prow = path + (int64_t)b * Tmax;
  int32_t* ts = tok_start + (int64_t)b * Lmax;
  int32_t* te = tok_end + (int64_t)b * Lmax;
  float* fl = frame_logp + (int64_t)b * Tmax;
  for (int s2 = tid; s2 < ALW_S + 2; s2 += AL_THREADS) ext[s2] = (s2 < S) ? ((s2 & 1) ? (int)targets[b * Lmax + (s2 >> 1)] : (int)blank) : -1;
  if (tid == 0) ok_s[0] = 0;
  __syncthreads();
  if (Tb <= 0) {  // (block-uniform)
    if (tid == 0) score[b] = -INFINITY;
    al_outputs<T>(x, lse, ext, r0, V, Tmax, Tb, L, Lmax, false, prow, ts, te, fl);
    return;
  }
  const bool in_lds = ((Tb + 15) >> 4) * S <= (int64_t)bp_lds_words;
  uint32_t* bp_ws = ws + (int64_t)b * ws_words;
  auto stage = [&](int chunk, int t0, int nthreads) {
    const int64_t c0 = (int64_t)chunk * ALW_CHUNK;
    const int nt = (int)min((int64_t)ALW_CHUNK, Tb - c0);
    float* dst = em[chunk & 1];
    for (int i = t0; i < nt * S; i += nthreads) {
      const int tt = i / S, s2 = i - tt * S;
      const int64_t t = c0 + tt;
      const int lab = ext[s2];
      dst[tt * ALW_S + s2] = (lab >= 0 && lab < V) ? io<T>::ld(x + (r0 + t) * V + lab) - lse[r0 + t] : -INFINITY;
    }
  };
  const int nchunks = (int)((Tb + ALW_CHUNK - 1) / ALW_CHUNK);
  stage(0, tid, AL_THREADS);
  __syncthreads();
  // wave 0: the recursion; lane l owns states 3l, 3l+1, 3l+2
  const int s0 = 3 * lane;
  bool skip[3];  // may the state take the path that jumps over a blank? (ctc_recursion_body's condition)
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int s2 = s0 + j;
    skip[j] = s2 >= 2 && s2 < S && ext[s2] != (int)blank && ext[s2] != ext[s2 - 2];
  }
  float a0 = -INFINITY, a1 = -INFINITY, a2 = -INFINITY;
  uint32_t w0 = 0u, w1 = 0u, w2 = 0u;  // back-pointer words of the lane's three states
  for (int c = 0; c < nchunks; ++c) {
    if (w != 0) {
      if (c + 1 < nchunks) stage(c + 1, tid - 64, AL_THREADS - 64);
    } else {
      const int64_t c0 = (int64_t)c * ALW_CHUNK;
      const int nt = (int)min((int64_t)ALW_CHUNK, Tb - c0);
      const float* e = em[c & 1];
      for (int tt = 0; tt < nt; ++tt) {
        const int64_t t = c0 + tt;
        const float e0 = s0 < S ? e[tt * ALW_S + s0] : -INFINITY, e1 = s0 + 1 < S ? e[tt * ALW_S + s0 + 1] : -INFINITY,
                    e2 = s0 + 2 < S ? e[tt * ALW_S + s0 + 2] : -INFINITY;
        float n0, n1, n2;
        uint32_t k0 = 0u, k1 = 0u, k2 = 0u;
        if (t == 0) {
          n0 = s0 < 2 ? e0 : -INFINITY;
          n1 = s0 + 1 < 2 ? e1 : -INFINITY;
          n2 = -INFINITY;
        } else {
          float p1 = __shfl_up(a1, 1, 64), p2 = __shfl_up(a2, 1, 64);  // states 3l-2, 3l-1
          if (lane == 0) { p1 = -INFINITY; p2 = -INFINITY; }
          float v0 = a0, v1 = a1, v2 = a2;
          al_take(v0, k0, p2, 1u);
          if (skip[0]) al_take(v0, k0, p1, 2u);
          al_take(v1, k1, a0, 1u);
          if (skip[1]) al_take(v1, k1, p2, 2u);
          al_take(v2, k2, a1, 1u);
          if (skip[2]) al_take(v2, k2, a0, 2u);
          n0 = v0 + e0, n1 = v1 + e1, n2 = v2 + e2;
        }
        a0 = s0 < S ? n0 : -INFINITY, a1 = s0 + 1 < S ? n1 : -INFINITY, a2 = s0 + 2 < S ? n2 : -INFINITY;
        const int sh = 2 * (int)(t & 15);
        w0 |= k0 << sh, w1 |= k1 << sh, w2 |= k2 << sh;
        if ((t & 15) == 15 || t == Tb - 1) {
          const int64_t g = (t >> 4) * S;
          if (in_lds) {
            if (s0 < S) bp_lds[g + s0] = w0;
            if (s0 + 1 < S) bp_lds[g + s0 + 1] = w1;
            if (s0 + 2 < S) bp_lds[g + s0 + 2] = w2;
          } else {
            if (s0 < S) bp_ws[g + s0] = w0;
            if (s0 + 1 < S) bp_ws[g + s0 + 1] = w1;
            if (s0 + 2 < S) bp_ws[g + s0 + 2] = w2;
          }
          w0 = w1 = w2 = 0u;
        }
      }
    }
    __syncthreads();
  }
  if (w == 0) {
    if (s0 < ALW_S) fin[s0] = a0;
    if (s0 + 1 < ALW_S) fin[s0 + 1] = a1;
    if (s0 + 2 < ALW_S) fin[s0 + 2] = a2;
  }
  __syncthreads();  // fin, and the back-pointer words (LDS or - workgroup scope - global), are visible to thread 0
  if (tid == 0) {
    if (in_lds) al_finish(fin, bp_lds, S, Tb, prow, score + b, ok_s);
    else al_finish(fin, bp_ws, S, Tb, prow, score + b, ok_s);
  }
  __syncthreads();  // the path row and ok_s are visible to the block
  al_outputs<T>(x, lse, ext, r0, V, Tmax, Tb, L, Lmax, ok_s[0] != 0, prow, ts, te, fl);
}

// ---------------------------------------------------------------- block form: up to 1023 states
// ctc_recursion_body's shape (loss.hip): states in two LDS rows, a block barrier per step; thread tid owns states tid + 256 k.
template <typename T>
__global__ __launch_bounds__(AL_THREADS) void ctc_align_block_kernel(
    const T* __restrict__ x, const float* __restrict__ lse, const int64_t* __restrict__ targets, const int64_t* __restrict__ in_len,
    const int64_t* __restrict__ tgt_len, int32_t* __restrict__ path, int32_t* __restrict__ tok_start, int32_t* __restrict__ tok_end,
    float* __restrict__ frame_logp, float* __restrict__ score, uint32_t* __restrict__ ws, int64_t ws_words, int bp_lds_words, int64_t Tmax,
    int64_t V, int64_t Lmax, int64_t blank, const int32_t* __restrict__ rowoff) {
  extern __shared__ __align__(16) unsigned char al_lds[];
  float(*a)[AL_MAX_S + 2] = (float(*)[AL_MAX_S + 2])al_lds;  // [2][...]
  int* ext = (int*)(al_lds + 2 * (AL_MAX_S + 2) * 4);         // [AL_MAX_S]
  float* em = (float*)(ext + AL_MAX_S);                       // [AL_CHUNK_FLOATS]
  int* ok_s = (int*)(em + AL_CHUNK_FLOATS);                   // [2]
  uint32_t* bp_lds = (uint32_t*)(ok_s + 2);                   // [bp_lds_words]
  constexpr int NK = AL_MAX_S / AL_THREADS;                   // states per thread
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t Tb = min(in_len[b], Tmax);
  const int L = (int)max((int64_t)0, min(tgt_len[b], Lmax));
  const int S = 2 * L + 1;
  const int64_t r0 = rowoff ? (int64_t)rowoff[b] : (int64_t)b * Tmax;
  int32_t* prow = path + (int64_t)b * Tmax;
  int32_t* ts = tok_start + (int64_t)b * Lmax;
  int32_t* te = tok_end + (int64_t)b * Lmax;
  float* fl = frame_logp + (int64_t)b * Tmax;
  for (int s = tid; s < S; s += AL_THREADS) ext[s] = (s & 1) ? (int)targets[b * Lmax + (s >> 1)] : (int)blank;
  if (tid == 0) ok_s[0] = 0;
  __syncthreads();
  if (Tb <= 0) {  // (block-uniform)
    if (tid == 0) score[b] = -INFINITY;
    al_outputs<T>(x, lse, ext, r0, V, Tmax, Tb, L, Lmax, false, prow, ts, te, fl);
    return;
  }
  const bool in_lds = ((Tb + 15) >> 4) * S <= (int64_t)bp_lds_words;
  uint32_t* bp_ws = ws + (int64_t)b * ws_words;
  bool skip[NK];
  uint32_t wk[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int s = tid + AL_THREADS * k;
    skip[k] = s >= 2 && s < S && ext[s] != (int)blank && ext[s] != ext[s - 2];
    wk[k] = 0u;
  }
  const int chunk_T = max(1, min(64, AL_CHUNK_FLOATS / S));
  int cur = 0;
  for (int64_t c0 = 0; c0 < Tb; c0 += chunk_T) {
    const int nt = (int)min((int64_t)chunk_T, Tb - c0);
    for (int i = tid; i < nt * S; i += AL_THREADS) {  // stage the emissions of this chunk of time steps
      const int tt = i / S, s = i - tt * S;
      const int64_t t = c0 + tt;
      const int lab = ext[s];
      em[i] = (lab >= 0 && lab < V) ? io<T>::ld(x + (r0 + t) * V + lab) - lse[r0 + t] : -INFINITY;
    }
    __syncthreads();
    for (int tt = 0; tt < nt; ++tt) {
      const int64_t t = c0 + tt;
      const float* prev = a[cur ^ 1];
      float* now = a[cur];
      const int sh = 2 * (int)(t & 15);
      const bool flush = (t & 15) == 15 || t == Tb - 1;
      const int64_t g = (t >> 4) * S;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int s = tid + AL_THREADS * k;
        if (s < S) {
          const float e = em[tt * S + s];
          float v;
          uint32_t code = 0u;
          if (t == 0) {
            v = s < 2 ? e : -INFINITY;
          } else {
            float best = prev[s];
            if (s >= 1) al_take(best, code, prev[s - 1], 1u);
            if (skip[k]) al_take(best, code, prev[s - 2], 2u);
            v = best + e;
          }
          now[s] = v;
          wk[k] |= code << sh;
          if (flush) {
            if (in_lds) bp_lds[g + s] = wk[k];
            else bp_ws[g + s] = wk[k];
            wk[k] = 0u;
          }
        }
      }
      __syncthreads();
      cur ^= 1;
    }
  }
  // (the barrier that closed the last step: the final row and the back-pointer words are visible to thread 0)
  if (tid == 0) {
    const float* fin = a[cur ^ 1];
    if (in_lds) al_finish(fin, bp_lds, S, Tb, prow, score + b, ok_s);
    else al_finish(fin, bp_ws, S, Tb, prow, score + b, ok_s);
  }
  __syncthreads();
  al_outputs<T>(x, lse, ext, r0, V, Tmax, Tb, L, Lmax, ok_s[0] != 0, prow, ts, te, fl);
}

constexpr size_t ALW_FIXED_LDS = (size_t)2 * ALW_CHUNK * ALW_S * 4 + (ALW_S + 2) * 4 + ALW_S * 4 + 8;
constexpr size_t ALB_FIXED_LDS = (size_t)2 * (AL_MAX_S + 2) * 4 + AL_MAX_S * 4 + AL_CHUNK_FLOATS * 4 + 8;

inline int64_t al_words_per_utt(int64_t T, int64_t Lmax) { return ((T + 15) >> 4) * (2 * Lmax + 1); }

template <typename T>
int al_launch(bool wave, size_t lds, hipStream_t s, int64_t B, const void* logits, const float* lse, const int64_t* targets,
              const int64_t* in_len, const int64_t* tgt_len, int32_t* path, int32_t* tok_start, int32_t* tok_end, float* frame_logp,
              float* score, uint32_t* ws, int64_t ws_words, int bp_words, int64_t T_, int64_t V, int64_t Lmax, int64_t blank,
              const int32_t* row_offsets) {
  auto kern = wave ? ctc_align_wave_kernel<T> : ctc_align_block_kernel<T>;
  if (lds > 48 * 1024 && js2t_lds_optin((const void*)kern, (int)lds) != JS2T_OK) return JS2T_ERR_LAUNCH;
  hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(AL_THREADS), lds, s, (const T*)logits, lse, targets, in_len, tgt_len, path, tok_start,
                     tok_end, frame_logp, score, ws, ws_words, bp_words, T_, V, Lmax, blank, row_offsets);
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}

}  // namespace

extern "C" int64_t js2t_ctc_align_workspace_bytes(int64_t B, int64_t T, int64_t Lmax) {
  if (B <= 0 || T <= 0 || Lmax < 0) return 0;
  return B * al_words_per_utt(T, Lmax) * 4;
}

extern "C" int js2t_ctc_align(const void* logits, int dt, const float* lse, const int64_t* targets, const int64_t* in_len,
                              const int64_t* tgt_len, int32_t* path, int32_t* tok_start, int32_t* tok_end, float* frame_logp,
                              float* score, void* workspace, int64_t B, int64_t T_, int64_t V, int64_t Lmax, int64_t blank,
                              const int32_t* row_offsets, js2t_stream stream) {
  if (B == 0) return JS2T_OK;
  JS2T_CHECK(logits && lse && in_len && tgt_len && path && frame_logp && score && (Lmax == 0 || (targets && tok_start && tok_end)),
             "ctc_align: null pointer");
  JS2T_CHECK(B > 0 && T_ > 0 && T_ < (int64_t(1) << 31) && V > 0 && Lmax >= 0, "ctc_align: bad shape");
  JS2T_CHECK(2 * Lmax + 1 <= AL_MAX_S, "ctc_align: target length %lld exceeds %d", (long long)Lmax, (AL_MAX_S - 1) / 2);
  JS2T_CHECK(dt == JS2T_F32 || dt == JS2T_BF16, "bad dtype %d", dt);
  const int64_t words = al_words_per_utt(T_, Lmax);
  const int64_t bp_words = words * 4 <= AL_BP_LDS_BYTES ? words : AL_BP_LDS_BYTES / 4;  // LDS words given to the back-pointers
  JS2T_CHECK(workspace || bp_words == words, "ctc_align: workspace needed (%lld bytes of back-pointers per utterance exceed the LDS budget)",
             (long long)(words * 4));
  const bool wave = 2 * Lmax + 1 <= ALW_S;
  const size_t lds = (wave ? ALW_FIXED_LDS : ALB_FIXED_LDS) + (size_t)bp_words * 4;
  if (dt == JS2T_F32)
    return al_launch<float>(wave, lds, (hipStream_t)stream, B, logits, lse, targets, in_len, tgt_len, path, tok_start, tok_end, frame_logp,
                            score, (uint32_t*)workspace, words, (int)bp_words, T_, V, Lmax, blank, row_offsets);
  return al_launch<uint16_t>(wave, lds, (hipStream_t)stream, B, logits, lse, targets, in_len, tgt_len, path, tok_start, tok_end, frame_logp,
                             score, (uint32_t*)workspace, words, (int)bp_words, T_, V, Lmax, blank, row_offsets);
}
