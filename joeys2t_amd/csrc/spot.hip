// Phrase spotting in a recording's CTC stream (EXTENSION): js2t_ctc_spot, whose header comment (include/joeys2t_hip.h) is the rule -
// a Viterbi recursion over the CTC states of a phrase with a free start in every frame, and a picker that turns the per-frame
// scores into disjoint hits.  One launch, one WAVEFRONT per phrase, one lane per state (S = 2 L - 1 <= 63): the state row lives in
// one VGPR, the left neighbours' (v, b) come by DPP wave shifts, nothing goes through LDS and there is no block barrier - the four
// waves of a block are four phrases that never meet.  The only memory traffic in the loop are the gathers logits[t, label_j] and
// norm[t]; a wave is sequential in t and so bound by their latency, hence the loads of the next SP_G frames are in flight while a
// group is computed (align_long.hip's ALL_G).  The picker's state is wave-uniform: every lane carries the same copy, read from lane
// S - 1 with a read-lane; lane 0 stores an emitted hit.  The dense outputs are buffered one frame per lane and stored 64 frames at a
// time.  Lanes >= S hold (-inf, -1) forever: values only ever move to the right, and nothing reads a lane behind S - 1.
#include "common.hpp"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / 64;  // phrases per block
constexpr int SP_MAX_L = 32;               // labels per phrase: 2 * 32 - 1 = 63 states, one wave
constexpr int SP_G = 16;                   // frames per prefetch group
static_assert(2 * SP_MAX_L - 1 <= 64 && 64 % SP_G == 0, "one lane per state; the dense outputs are flushed at group ends");

// the value of the lane to the left (wave shift right by one lane); lane 0 takes `edge`
__device__ __forceinline__ float sp_left(float v, float edge) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138, 0xf, 0xf, false));  // wave_shr:1
}
__device__ __forceinline__ int sp_left(int v, int edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x138, 0xf, 0xf, false); }

struct SpGroup {  // what SP_G frames need from memory: the lane's gathered logit and the frame's normaliser
  float x[SP_G], n[SP_G];
};

template <typename T>
__global__ __launch_bounds__(SP_THREADS) void ctc_spot_kernel(const T* __restrict__ x, const float* __restrict__ norm,
                                                              const int64_t* __restrict__ tokens, const int32_t* __restrict__ lengths, int K,
                                                              int Lmax, int32_t* __restrict__ hit_count, int32_t* __restrict__ hit_start,
                                                              int32_t* __restrict__ hit_end, float* __restrict__ hit_score, int max_hits,
                                                              float* __restrict__ frame_score, int32_t* __restrict__ frame_start, int Tn,
                                                              int64_t V, int64_t blank, float thr) {
  const int lane = threadIdx.x & 63;
  const int k = (int)blockIdx.x * SP_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (k >= K) return;  // (wave-uniform; no barrier below)
  const int L = __builtin_amdgcn_readfirstlane(min(max(lengths[k], 1), Lmax));
  const int S = 2 * L - 1;
  const bool on = lane < S;
  const int64_t* tok = tokens + (int64_t)k * Lmax;
  int64_t lab = -1;
  bool skip = false;  // the step over a blank: label states whose label differs from the one two states back
  if (on) {
    if (lane & 1) {
      lab = blank;
    } else {
      lab = tok[lane >> 1];  // lane >> 1 < L: padding behind the length is never read
      skip = lane >= 2 && lab != tok[(lane >> 1) - 1];
    }
  }
  const bool valid = on && lab >= 0 && lab < V;
  const int64_t col = valid ? lab : 0;

  auto load_group = [&](int gi) {
    SpGroup g;
#pragma unroll
    for (int i = 0; i < SP_G; ++i) {
      const int64_t t = min(gi * SP_G + i, Tn - 1);  // (frames behind the end: loaded in bounds, never used)
      g.x[i] = io<T>::ld(x + t * V + col);
      g.n[i] = norm[t];
    }
    return g;
  };

  float v = -INFINITY;
  int b = -1;
  bool have = false;  // the picker: wave-uniform
  float cs = 0.f;
  int cb = 0, ce = 0, last_end = -1, n = 0;
  float hbuf = 0.f;  // h, s of frame t in lane t & 63
  int sbuf = 0;
  auto emit = [&]() {
    if (lane == 0 && n < max_hits) {
      const int64_t o = (int64_t)k * max_hits + n;
      hit_start[o] = cb, hit_end[o] = ce + 1, hit_score[o] = cs;
    }
    ++n;
  };

  const int ngroups = (Tn + SP_G - 1) / SP_G;
  SpGroup cur = load_group(0);
#pragma unroll 1
  for (int gi = 0; gi < ngroups; ++gi) {
    SpGroup nxt = cur;
    if (gi + 1 < ngroups) nxt = load_group(gi + 1);
#pragma unroll
    for (int i = 0; i < SP_G; ++i) {
      const int t = gi * SP_G + i;
      if (t < Tn) {
        const float e = valid ? cur.x[i] - cur.n[i] : -INFINITY;
        const float p1v = sp_left(v, -INFINITY), p2v = sp_left(p1v, -INFINITY);  // states j - 1, j - 2
        const int p1b = sp_left(b, -1), p2b = sp_left(p1b, -1);
        float best = v;
        int bb = b;
        if (lane == 0 && !(v >= 0.f)) { best = 0.f; bb = t; }  // the free start
        if (p1v > best) { best = p1v; bb = p1b; }              // stay, then j - 1, then j - 2: a switch needs a strict >
        if (skip && p2v > best) { best = p2v; bb = p2b; }
        v = best + e;
        b = v == -INFINITY ? -1 : bb;
        const float h = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), S - 1));
        const int s = __builtin_amdgcn_readlane(b, S - 1);
        if (lane == (t & 63)) { hbuf = h; sbuf = s; }
        if (h >= thr && s > last_end) {  // a candidate
          if (!have) {
            have = true, cs = h, cb = s, ce = t;
          } else if (s > ce) {
            emit();
            last_end = ce, cs = h, cb = s, ce = t;
          } else if (h > cs || (h == cs && s == cb)) {
            cs = h, cb = s, ce = t;
          }
        }
      }
    }
    const int tend = min(Tn, (gi + 1) * SP_G);  // the dense outputs: 64 frames at a time, and what is left at the end
    if ((tend & 63) == 0 || tend == Tn) {
      const int t = ((tend - 1) & ~63) + lane;
      if (t < tend) {
        if (frame_score) frame_score[(int64_t)k * Tn + t] = hbuf;
        if (frame_start) frame_start[(int64_t)k * Tn + t] = sbuf;
      }
    }
    cur = nxt;
  }
  if (have) emit();
  if (lane == 0) hit_count[k] = n;
}

}  // namespace

extern "C" void js2t_ctc_spot_tiles(int32_t* out) { out[0] = SP_MAX_L, out[1] = SP_WAVES, out[2] = SP_G; }

extern "C" int js2t_ctc_spot(const void* logits, int dt, const float* norm, const int64_t* tokens, const int32_t* lengths, int64_t K,
                             int64_t Lmax, int32_t* hit_count, int32_t* hit_start, int32_t* hit_end, float* hit_score, int64_t max_hits,
                             float* frame_score, int32_t* frame_start, int64_t T_, int64_t V, int64_t blank, float log_threshold,
                             js2t_stream stream) {
  JS2T_CHECK(T_ >= 0 && T_ < (int64_t(1) << 31) && V >= 1 && K >= 0 && K <= 65535 && Lmax >= 1 && max_hits >= 1 &&
                 max_hits < (int64_t(1) << 31),
             "ctc_spot: bad shape (T %lld, V %lld, K %lld, Lmax %lld, max_hits %lld)", (long long)T_, (long long)V, (long long)K,
             (long long)Lmax, (long long)max_hits);
  JS2T_CHECK(Lmax <= SP_MAX_L, "ctc_spot: phrase length %lld exceeds %d", (long long)Lmax, SP_MAX_L);
  JS2T_CHECK(dt == JS2T_F32 || dt == JS2T_BF16, "bad dtype %d", dt);
  JS2T_CHECK(log_threshold - log_threshold == 0.f, "ctc_spot: the threshold must be finite");
  JS2T_CHECK(K == 0 || (tokens && lengths && hit_count && hit_start && hit_end && hit_score && (T_ == 0 || (logits && norm))),
             "ctc_spot: null pointer");
  if (K == 0) return JS2T_OK;
  hipStream_t st = (hipStream_t)stream;
  if (T_ == 0) {
    (void)hipMemsetAsync(hit_count, 0, (size_t)K * sizeof(int32_t), st);
    JS2T_LAUNCH_CHECK();
    return JS2T_OK;
  }
  const dim3 grid((unsigned)((K + SP_WAVES - 1) / SP_WAVES)), block(SP_THREADS);
  if (dt == JS2T_F32)
    hipLaunchKernelGGL(ctc_spot_kernel<float>, grid, block, 0, st, (const float*)logits, norm, tokens, lengths, (int)K, (int)Lmax, hit_count,
                       hit_start, hit_end, hit_score, (int)max_hits, frame_score, frame_start, (int)T_, V, blank, log_threshold);
  else
    hipLaunchKernelGGL(ctc_spot_kernel<uint16_t>, grid, block, 0, st, (const uint16_t*)logits, norm, tokens, lengths, (int)K, (int)Lmax,
                       hit_count, hit_start, hit_end, hit_score, (int)max_hits, frame_score, frame_start, (int)T_, V, blank, log_threshold);
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}
