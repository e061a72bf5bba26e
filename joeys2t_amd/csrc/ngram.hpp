// Back-off n-gram language model on the device: the table view, the key packing and the log-probability of one token given its
// history (EXTENSION; the reference has no language model).  The layout and the rules are stated in the header at
// js2t_ngram_rescore; this file is what a kernel includes to apply them (ngram.hip and ctc_beam.hip do), and its ngram_args is what
// their entry points check the LM arguments with.
//
//   uni   f32 [V, 2]: (logp, backoff) of every id, dense.
//   table `capacity` (a power of two) entries of 16 bytes {u64 key, f32 logp, f32 backoff}: the 2-grams .. order-grams, open
//         addressing with linear probing and wrap-around, home slot fmix(key) & (capacity - 1), fmix = the splitmix64 finaliser
//         (nbest.hpp's nbest_fmix).
//   key   of (w1 .. wk): field j (0 = newest = wk) = id + 1 in bits 16j .. 16j+15; 0 = an empty slot.  The key IS the n-gram:
//         a match is exact.
//
// ngram_token_logp issues the FIRST probe of every key a position can need (its up to three hit keys and two back-off keys, all
// computable from the ids alone) and the two unigram loads before it looks at any of them: one memory latency for the position,
// not one per back-off level.  Only a first probe that meets another key walks on, at most max_probe slots in all.
#pragma once
#include "common.hpp"
#include "nbest.hpp"

constexpr int NGRAM_MAX_ORDER = 4;
constexpr int NGRAM_MAX_CTX = NGRAM_MAX_ORDER - 1;

struct ngram_view {
  const float2* uni;   // [V] (logp, backoff)
  const uint4* table;  // [capacity] {key lo, key hi, logp bits, backoff bits}; NULL for order 1
  uint64_t mask;       // capacity - 1
  int max_probe;       // slots a lookup examines at most
  int order;           // 1 .. NGRAM_MAX_ORDER
  int V;               // 2 .. 65535
};

// (host) the LM arguments of the entry point `who` - js2t_ngram_rescore's, which js2t_ctc_beam_search_lm takes too: checked in
// this order with these messages, and the view filled
inline int ngram_args(const char* who, const float* uni, const void* table, int64_t capacity, int32_t max_probe, int32_t lm_order, int64_t V,
                      int64_t bos, int64_t eos, float lm_weight, float length_bonus, ngram_view* lm) {
  JS2T_CHECK(V >= 2 && V <= 65535, "%s: V %lld outside 2..65535", who, (long long)V);
  JS2T_CHECK(bos >= 0 && bos < V, "%s: bos %lld outside the vocabulary", who, (long long)bos);
  JS2T_CHECK(eos >= 0 && eos < V, "%s: eos %lld outside the vocabulary", who, (long long)eos);
  JS2T_CHECK(lm_order >= 1 && lm_order <= NGRAM_MAX_ORDER, "%s: order %d outside 1..%d", who, (int)lm_order, NGRAM_MAX_ORDER);
  JS2T_CHECK(capacity >= 0 && (capacity & (capacity - 1)) == 0, "%s: capacity %lld is neither 0 nor a power of two", who, (long long)capacity);
  JS2T_CHECK(isfinite(lm_weight) && isfinite(length_bonus), "%s: lm_weight %g / length_bonus %g not finite", who, (double)lm_weight,
             (double)length_bonus);
  if (lm_weight != 0.f) {  // a weight of exactly 0 leaves the model out: uni and table are not read and may be NULL
    JS2T_CHECK(uni, "%s: null pointer (uni, with lm_weight %g)", who, (double)lm_weight);
    if (lm_order > 1) {
      JS2T_CHECK(table && capacity >= 1, "%s: order %d needs a table (capacity %lld)", who, (int)lm_order, (long long)capacity);
      JS2T_CHECK(((uintptr_t)table & 15) == 0, "%s: table not 16-byte aligned", who);
      JS2T_CHECK(max_probe >= 1 && (int64_t)max_probe <= capacity, "%s: max_probe %d outside 1..capacity (%lld)", who, (int)max_probe,
                 (long long)capacity);
    }
  }
  lm->uni = (const float2*)uni, lm->table = (const uint4*)table, lm->mask = capacity > 0 ? (uint64_t)capacity - 1 : 0;
  lm->max_probe = max_probe, lm->order = lm_order, lm->V = (int)V;
  return JS2T_OK;
}

__host__ __device__ __forceinline__ uint64_t ngram_entry_key(const uint4 e) { return (uint64_t)e.x | ((uint64_t)e.y << 32); }

// the probing rule alone, for any table of this entry format (the LM's, and context.hpp's edge table): `e` holds the first probe
// (slot `home`) and, on return, the last entry examined; only a probe that met another key walks on, at most max_probe slots in all
__host__ __device__ __forceinline__ bool ngram_probe(const uint4* table, uint64_t mask, int max_probe, uint64_t key, uint64_t home, uint4& e) {
  uint64_t k = ngram_entry_key(e);
  for (int i = 1; key != 0 && k != key && k != 0 && i < max_probe; ++i) {
    e = table[(home + (uint64_t)i) & mask];
    k = ngram_entry_key(e);
  }
  return key != 0 && k == key;
}

struct ngram_hit {
  bool found;
  float logp, backoff;
};

// slot of a key's first probe (a key of 0, "no such level", probes slot 0: a valid address whose value is not used)
__device__ __forceinline__ uint64_t ngram_home(const ngram_view& lm, uint64_t key) { return key ? nbest_fmix(key) & lm.mask : 0; }

// the rest of a lookup whose first probe `e` (slot `home`) has been loaded; only a probe that met another key walks on
__device__ __forceinline__ ngram_hit ngram_resolve(const ngram_view& lm, uint64_t key, uint64_t home, uint4 e) {
  ngram_hit h;
  h.found = ngram_probe(lm.table, lm.mask, lm.max_probe, key, home, e);
  h.logp = __uint_as_float(e.z), h.backoff = __uint_as_float(e.w);
  return h;
}

// log p(w | history) in natural logarithms.  c[j] = the j-th newest token of the history (c[0] directly in front of w), navail = how
// many of them exist (the caller counts BOS); the last min(navail, order - 1) are the context, cut behind the newest id outside
// 0 .. V-1.  For k = context length down to 1: the (k+1)-gram (context's last k, w) stored -> acc + its logp; else acc += the
// back-off of the k-gram (context's last k) if stored, else 0.  No match: acc + uni[w].logp.  w outside 0 .. V-1: -inf.
__device__ __forceinline__ float ngram_token_logp(const ngram_view& lm, int64_t w, const int64_t (&c)[NGRAM_MAX_CTX], int navail) {
  if (w < 0 || w >= lm.V) return -INFINITY;
  const int use = navail < lm.order - 1 ? navail : lm.order - 1;
  const bool v1 = use > 0 && c[0] >= 0 && c[0] < lm.V;        // the context holds 1, 2, 3 tokens at least
  const bool v2 = v1 && use > 1 && c[1] >= 0 && c[1] < lm.V;
  const bool v3 = v2 && use > 2 && c[2] >= 0 && c[2] < lm.V;
  const uint64_t x1 = v1 ? (uint64_t)(c[0] + 1) : 0;          // the k-gram of the context's last k tokens
  const uint64_t x2 = v2 ? x1 | (uint64_t)(c[1] + 1) << 16 : 0;
  const uint64_t x3 = v3 ? x2 | (uint64_t)(c[2] + 1) << 32 : 0;
  const uint64_t ww = (uint64_t)(w + 1);
  const uint64_t k1 = v1 ? x1 << 16 | ww : 0, k2 = v2 ? x2 << 16 | ww : 0, k3 = v3 ? x3 << 16 | ww : 0;  // (context's last k, w)
  const float uw = lm.uni[w].x;
  const float ub = lm.uni[v1 ? c[0] : w].y;  // back-off of the 1-gram context (unused without one)
  if (lm.order == 1) return uw;              // (uniform) no table
  // every first probe, issued together: straight-line code, five independent 16-byte loads
  const uint64_t h1 = ngram_home(lm, k1), h2 = ngram_home(lm, k2), h3 = ngram_home(lm, k3), g2 = ngram_home(lm, x2), g3 = ngram_home(lm, x3);
  const uint4 e1 = lm.table[h1], e2 = lm.table[h2], e3 = lm.table[h3], f2 = lm.table[g2], f3 = lm.table[g3];
  float acc = 0.f;
  if (v3) {
    const ngram_hit h = ngram_resolve(lm, k3, h3, e3);
    if (h.found) return acc + h.logp;
    const ngram_hit b = ngram_resolve(lm, x3, g3, f3);
    acc += b.found ? b.backoff : 0.f;
  }
  if (v2) {
    const ngram_hit h = ngram_resolve(lm, k2, h2, e2);
    if (h.found) return acc + h.logp;
    const ngram_hit b = ngram_resolve(lm, x2, g2, f2);
    acc += b.found ? b.backoff : 0.f;
  }
  if (v1) {
    const ngram_hit h = ngram_resolve(lm, k1, h1, e1);
    if (h.found) return acc + h.logp;
    acc += ub;
  }
  return acc + uw;
}
