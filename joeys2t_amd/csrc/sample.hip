// Sampling step of the attention decoder (EXTENSION: the reference has no sampling; contract in include/joeys2t_hip.h,
// js2t_sample_step).  One launch per decoding step, one 256-thread block per row of the [rows, V] logits:
//   log-sum-exp of the whole row -> forbidden ids out -> temperature -> epsilon / top-k / nucleus truncation -> draw by the
//   row's uniform number -> the row's ids column, finished flag, score and length, all on the device.
// The row is staged ONCE in LDS (V <= SP_LDS_V: 40 KB; 16-byte loads where the row is aligned, element loads for a view) and every
// later pass reads it there; longer rows are re-read from L2.  Every pass computes from that image, so a view gives the bits of
// its contiguous copy.
// Order: the three truncations are prefixes of ONE order (raw logit descending, id ascending), so they are ONE kind of selection:
// a radix descent over monotone integer keys of the raw logit - level 0 over 256 linear bins of (max - logit) / temperature (a
// monotone function of the logit: it only spreads the histogram, f32 bit patterns of a row share their top byte), levels 1 - 4
// over the four bytes of the key inside the chosen bin - that looks for the prefix whose COUNT reaches n0 = min(n_eps, n_k), and
// once more for the prefix whose MASS reaches top_p * mass(n0).  A selection that cannot cut (no top-k / epsilon; top_p == 1) is
// left out.
// Masses are 2^-40 fixed point in 64-bit integers: e_v = exp((logit_v - max) / temperature) <= 1 truncated to 2^-40, at most
// V * 2^-40 <= 6e-8 of the total (which is >= 1) for the whole row.  Integer sums are exact and commute, so the per-bin LDS
// atomics, the scans and the draw give the same bits in any thread order: no floating-point atomics, nothing scheduling-dependent,
// no chain of float additions at all behind the per-element exp.  (The float sum of the row's log-sum-exp is strided, <= 256
// sequential additions per thread, then a fixed tree.)
// Draw: blocked scan in id order over the kept masses (thread t owns ids [t * C, (t + 1) * C)); the id is the first kept one whose
// inclusive sum exceeds floor(u * W).
#include <float.h>

#include "common.hpp"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_MAX_FORBID = 16;
constexpr int SP_LDS_V = 10240;  // rows up to this length are staged in LDS (40 KB)
constexpr int SP_MAX_V = 65536;
constexpr uint32_t SP_KEY_NEGINF = 0x007fffffu;  // sp_key(-inf): every eligible id has a larger key
constexpr float SP_FIX = 1099511627776.f;        // 2^40
constexpr float SP_BIN_SCALE = 8.f;              // level 0: 256 bins over 32 nats below the maximum

struct SampleForbid {
  int32_t n;
  int32_t ids[SP_MAX_FORBID];
};

struct SampleArgs {
  const float* logits;
  int64_t ld;
  const float* u;
  uint8_t* finished;
  int64_t* ids;
  int64_t ids_ld;
  int32_t step;
  float* out_logp;
  float* out_q;
  float* score;
  int32_t* length;
  int32_t* out_kept;
  float* out_cdf;
  int32_t V;
  float inv_t;
  int32_t top_k;
  float top_p;
  float epsilon;
  int64_t eos, pad;
  SampleForbid fb;
};

// monotone integer key of a float: a > b  <=>  sp_key(a) > sp_key(b) (no NaN, no -0 behind sp_clean)
__device__ __forceinline__ uint32_t sp_key(float x) {
  const uint32_t b = __float_as_uint(x);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float sp_unkey(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
// NaN counts as -inf; +inf (not supported input) is carried as the largest finite value; -0 becomes +0 (equal logits, equal keys)
__device__ __forceinline__ float sp_clean(float x) {
  x = x != x ? -INFINITY : fminf(x, FLT_MAX);
  return x + 0.f;
}

struct SampleRow {
  const float* row;  // global
  const float* xs;   // LDS image (IN_LDS)
  float mx;          // maximum over the eligible ids
  float inv_t;
  uint32_t bin0;     // level-0 bin of the selection in progress
  SampleForbid fb;
};

template <bool IN_LDS>
__device__ __forceinline__ float sp_raw(const SampleRow& c, int i) { return IN_LDS ? c.xs[i] : sp_clean(c.row[i]); }
// the logit of id i with the forbidden ids at -inf (the LDS image has them written in after the log-sum-exp)
template <bool IN_LDS>
__device__ __forceinline__ float sp_get(const SampleRow& c, int i) {
  float x = sp_raw<IN_LDS>(c, i);
  if (!IN_LDS) {
#pragma unroll  // static indices: the list stays in scalar registers (unused entries are -1)
    for (int f = 0; f < SP_MAX_FORBID; ++f)
      if (i == c.fb.ids[f]) x = -INFINITY;
  }
  return x;
}
__device__ __forceinline__ unsigned long long sp_mass(const SampleRow& c, float x) {
  return (unsigned long long)(__expf((x - c.mx) * c.inv_t) * SP_FIX);
}
__device__ __forceinline__ int sp_bin0(const SampleRow& c, float x) {
  const int b = (int)fminf((c.mx - x) * (SP_BIN_SCALE * c.inv_t), 255.f);
  return min(max(b, 0), 255);
}

// block-wide inclusive scan of one 64-bit value per thread, in thread order; `total` = the sum over the block
__device__ __forceinline__ unsigned long long sp_scan(unsigned long long v, unsigned long long* wsum, unsigned long long& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long n = __shfl_up(v, o, 64);
    if (lane >= o) v += n;
  }
  __syncthreads();
  if (lane == 63) wsum[w] = v;
  __syncthreads();
  unsigned long long base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < SP_THREADS / 64; ++i) {
    if (i < w) base += wsum[i];
    total += wsum[i];
  }
  return v + base;
}

struct SampleShared {
  unsigned long long hmass[256];
  unsigned long long wsum[SP_THREADS / 64];
  unsigned long long res_mass;
  unsigned int hcnt[256];
  unsigned int res_bin, res_cnt, res_n;
  float red[SP_THREADS / 64];
  int pick, last_kept;
  unsigned long long pick_e, pick_c;
};

// The prefix of the order (key descending, id ascending) at which the running count (by_mass = false) or the running mass reaches
// `target` (>= 1 and at most the row's total).  Returns its last key `key`, how many of the ids with exactly that key belong to it
// (r >= 1, in id order), and count / mass of the ids with a larger key.
template <bool IN_LDS>
__device__ void sp_select(SampleRow& c, SampleShared& sh, int V, bool by_mass, unsigned long long target, uint32_t& key, uint32_t& r,
                          uint32_t& above_cnt, unsigned long long& above_mass) {
  const int t = threadIdx.x;
  uint32_t pref = 0, ties = 0;
  above_cnt = 0;
  above_mass = 0;
  for (int level = 0; level < 5; ++level) {
    const int shift = 32 - 8 * level;  // levels 1..4: the byte at `shift`
    sh.hcnt[t] = 0;
    sh.hmass[t] = 0;
    __syncthreads();
    for (int i = t; i < V; i += SP_THREADS) {
      const float x = sp_get<IN_LDS>(c, i);
      if (!(x > -INFINITY)) continue;
      int bin = sp_bin0(c, x);
      if (level > 0) {
        const uint32_t k = sp_key(x);
        if ((uint32_t)bin != c.bin0) continue;
        if (level > 1 && (k >> (shift + 8)) != (pref >> (shift + 8))) continue;
        bin = 255 - (int)((k >> shift) & 255u);
      }
      atomicAdd(&sh.hcnt[bin], 1u);
      atomicAdd(&sh.hmass[bin], sp_mass(c, x));
    }
    __syncthreads();
    const unsigned long long n = sh.hcnt[t], m = sh.hmass[t];
    unsigned long long tot;
    const unsigned long long ec = sp_scan(n, sh.wsum, tot) - n + above_cnt;
    const unsigned long long em = sp_scan(m, sh.wsum, tot) - m + above_mass;
    const bool hit = by_mass ? (em < target && em + m >= target) : (ec < target && ec + n >= target);
    if (hit) {
      sh.res_bin = t;
      sh.res_cnt = (unsigned int)ec;
      sh.res_mass = em;
      sh.res_n = (unsigned int)n;
    }
    __syncthreads();
    above_cnt = sh.res_cnt;
    above_mass = sh.res_mass;
    ties = sh.res_n;
    if (level == 0) c.bin0 = sh.res_bin;
    else pref |= (255u - sh.res_bin) << shift;
    __syncthreads();
  }
  key = pref;
  if (by_mass) {
    const unsigned long long e = max(sp_mass(c, sp_unkey(key)), 1ull);
    r = (uint32_t)min((target - above_mass + e - 1) / e, (unsigned long long)ties);
  } else {
    r = (uint32_t)(target - above_cnt);
  }
  r = max(r, 1u);
}

template <bool IN_LDS>
__global__ __launch_bounds__(SP_THREADS) void sample_step_kernel(SampleArgs a) {
  extern __shared__ float sp_xs[];
  __shared__ SampleShared sh;
  const int r = blockIdx.x, t = threadIdx.x, V = a.V;
  int64_t* id_out = a.ids + (int64_t)r * a.ids_ld + a.step;
  if (a.finished && a.finished[r]) {  // nothing of the row's logits or its u is read
    if (t == 0) {
      *id_out = a.pad;
      a.out_logp[r] = 0.f;
      if (a.out_q) a.out_q[r] = 0.f;
      if (a.out_kept) a.out_kept[r] = 0;
      if (a.out_cdf) a.out_cdf[2 * r] = 0.f, a.out_cdf[2 * r + 1] = 0.f;
    }
    return;
  }
  SampleRow c;
  c.row = a.logits + (int64_t)r * a.ld;
  c.xs = sp_xs;
  c.inv_t = a.inv_t;
  c.fb = a.fb;
  c.bin0 = 0;
  c.mx = 0.f;
  // 1. stage the row (same image whatever the alignment), log-sum-exp of the WHOLE row
  if (IN_LDS) {
    const bool aligned = ((uintptr_t)c.row & 15) == 0;
    for (int q = t; 4 * q < V; q += SP_THREADS) {
      if (aligned && 4 * q + 3 < V) {
        const float4 f = *(const float4*)(c.row + 4 * q);
        sp_xs[4 * q] = sp_clean(f.x), sp_xs[4 * q + 1] = sp_clean(f.y), sp_xs[4 * q + 2] = sp_clean(f.z), sp_xs[4 * q + 3] = sp_clean(f.w);
      } else {
        for (int e = 4 * q; e < min(4 * q + 4, V); ++e) sp_xs[e] = sp_clean(c.row[e]);
      }
    }
    __syncthreads();
  }
  float mx = -INFINITY;
  for (int i = t; i < V; i += SP_THREADS) mx = fmaxf(mx, sp_raw<IN_LDS>(c, i));
  mx = block_max(mx, sh.red);
  float sm = 0.f;
  if (mx > -INFINITY)
    for (int i = t; i < V; i += SP_THREADS) sm += __expf(sp_raw<IN_LDS>(c, i) - mx);
  sm = block_sum(sm, sh.red);
  const float lse = mx + __logf(sm);
  __syncthreads();
  if (IN_LDS) {
    if (t < a.fb.n && a.fb.ids[t] >= 0 && a.fb.ids[t] < V) sp_xs[a.fb.ids[t]] = -INFINITY;
    __syncthreads();
  }
  // 2. the eligible set: its maximum and its size
  float mxa = -INFINITY;
  unsigned long long na = 0, tot;
  for (int i = t; i < V; i += SP_THREADS) {
    const float x = sp_get<IN_LDS>(c, i);
    mxa = fmaxf(mxa, x);
    na += x > -INFINITY ? 1 : 0;
  }
  mxa = block_max(mxa, sh.red);
  sp_scan(na, sh.wsum, tot);
  const uint32_t n_a = (uint32_t)tot;
  if (n_a == 0) {  // nothing eligible: the row ends here
    if (t == 0) {
      *id_out = a.eos;
      a.out_logp[r] = -INFINITY;
      if (a.out_q) a.out_q[r] = 0.f;
      if (a.out_kept) a.out_kept[r] = 0;
      if (a.out_cdf) a.out_cdf[2 * r] = 0.f, a.out_cdf[2 * r + 1] = 0.f;
      if (a.finished) a.finished[r] = 1;
      if (a.score) a.score[r] += -INFINITY;
    }
    return;
  }
  c.mx = mxa;
  // 3. n0 = min(n_eps, n_k) and the mass of that prefix
  uint32_t n0 = a.top_k == 0 ? n_a : min((uint32_t)a.top_k, n_a);
  unsigned long long m0 = 0;  // the mass of the first n0 (only where the nucleus needs it)
  if (a.epsilon > 0.f || (a.top_p < 1.f && n0 == n_a)) {
    unsigned long long s = 0;
    for (int i = t; i < V; i += SP_THREADS) s += sp_mass(c, sp_get<IN_LDS>(c, i));
    sp_scan(s, sh.wsum, m0);
  }
  if (a.epsilon > 0.f) {
    const unsigned long long thr = (unsigned long long)ceil((double)a.epsilon * (double)m0);
    unsigned long long ne = 0;
    for (int i = t; i < V; i += SP_THREADS) {
      const float x = sp_get<IN_LDS>(c, i);
      ne += (x > -INFINITY && sp_mass(c, x) >= thr) ? 1 : 0;
    }
    sp_scan(ne, sh.wsum, tot);
    n0 = min(n0, max((uint32_t)tot, 1u));
  }
  // the kept set: every id with a key above `key`, and the first `nt` (by id) of those with exactly `key`
  uint32_t key = SP_KEY_NEGINF, nt = 0, kept = n_a;
  if (n0 < n_a) {
    uint32_t ac;
    unsigned long long am;
    sp_select<IN_LDS>(c, sh, V, false, n0, key, nt, ac, am);
    m0 = am + (unsigned long long)nt * sp_mass(c, sp_unkey(key));
    kept = n0;
  }
  if (a.top_p < 1.f) {
    const unsigned long long target = max((unsigned long long)ceil((double)a.top_p * (double)m0), 1ull);
    uint32_t ac;
    unsigned long long am;
    sp_select<IN_LDS>(c, sh, V, true, min(target, m0), key, nt, ac, am);
    kept = ac + nt;
  }
  // 4. the draw: blocked scan in id order over the kept masses
  const int per = (V + SP_THREADS - 1) / SP_THREADS, lo = min(t * per, V), hi = min(lo + per, V);
  unsigned long long tie_base = 0;
  if (nt > 0) {
    unsigned long long n = 0;
    for (int i = lo; i < hi; ++i) n += sp_key(sp_get<IN_LDS>(c, i)) == key ? 1 : 0;
    tie_base = sp_scan(n, sh.wsum, tot) - n;
  }
  unsigned long long lm = 0, ties = tie_base;
  int last = -1;
  for (int i = lo; i < hi; ++i) {
    const float x = sp_get<IN_LDS>(c, i);
    const uint32_t k = sp_key(x);
    const bool in = k > key || (k == key && nt > 0 && ties++ < nt);
    if (in) lm += sp_mass(c, x), last = i;
  }
  if (t == 0) sh.pick = -1, sh.last_kept = -1;
  unsigned long long W;
  const unsigned long long base = sp_scan(lm, sh.wsum, W) - lm;
  float u = a.u[r];
  u = u != u ? 0.f : fminf(fmaxf(u, 0.f), 0.99999994f);
  unsigned long long uw = (unsigned long long)((double)u * (double)W);
  if (W > 0 && uw >= W) uw = W - 1;
  if (last >= 0) atomicMax(&sh.last_kept, last);
  if (base <= uw && uw < base + lm) {
    unsigned long long cs = base;
    ties = tie_base;
    for (int i = lo; i < hi; ++i) {
      const float x = sp_get<IN_LDS>(c, i);
      const uint32_t k = sp_key(x);
      const bool in = k > key || (k == key && nt > 0 && ties++ < nt);
      if (!in) continue;
      const unsigned long long e = sp_mass(c, x);
      cs += e;
      if (cs > uw) {
        sh.pick = i;
        sh.pick_e = e;
        sh.pick_c = cs;
        break;
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    int id = sh.pick;
    unsigned long long e = sh.pick_e, cs = sh.pick_c;
    if (id < 0) {  // no interval holds u * W (not with finite logits): the largest kept id, never a dropped one
      id = sh.last_kept >= 0 ? sh.last_kept : 0;
      e = sp_mass(c, sp_get<IN_LDS>(c, id));
      cs = W;
    }
    const float lp = sp_get<IN_LDS>(c, id) - lse;
    const double w = W > 0 ? (double)W : 1.0;
    *id_out = id;
    a.out_logp[r] = lp;
    if (a.out_q) a.out_q[r] = (float)log((double)e / w);
    if (a.out_kept) a.out_kept[r] = (int32_t)kept;
    if (a.out_cdf) a.out_cdf[2 * r] = (float)((double)(cs - e) / w), a.out_cdf[2 * r + 1] = (float)((double)cs / w);
    if (a.finished && id == a.eos) a.finished[r] = 1;
    if (a.score) a.score[r] += lp;
    if (a.length && id != a.eos) a.length[r] += 1;
  }
}

}  // namespace

extern "C" int js2t_sample_step(const float* logits, int64_t ld, const float* u, uint8_t* finished, int64_t* ids, int64_t ids_ld,
                                int32_t step, float* out_logp, float* out_q, float* score, int32_t* length, int32_t* out_kept,
                                float* out_cdf, int64_t rows, int64_t V, const int32_t* forbid_ids, int32_t n_forbid, float temperature,
                                int32_t top_k, float top_p, float epsilon, int64_t eos, int64_t pad, js2t_stream stream) {
  JS2T_CHECK(rows >= 0 && rows < 0x7fffffff, "sample_step: row count %lld outside 0 .. 2^31 - 1", (long long)rows);
  JS2T_CHECK(V >= 2 && V <= SP_MAX_V, "sample_step: vocabulary %lld outside 2 .. %d", (long long)V, SP_MAX_V);
  JS2T_CHECK(n_forbid >= 0 && n_forbid <= SP_MAX_FORBID && (n_forbid == 0 || forbid_ids), "sample_step: at most %d forbidden ids",
             SP_MAX_FORBID);
  JS2T_CHECK(temperature > 0.f && temperature <= FLT_MAX, "sample_step: temperature %g is not finite and positive", (double)temperature);
  JS2T_CHECK(top_k >= 0, "sample_step: top_k %d below 0", top_k);
  JS2T_CHECK(top_p > 0.f && top_p <= 1.f, "sample_step: top_p %g outside (0, 1]", (double)top_p);
  JS2T_CHECK(epsilon >= 0.f && epsilon < 1.f, "sample_step: epsilon %g outside [0, 1)", (double)epsilon);
  JS2T_CHECK(step >= 0 && step < ids_ld, "sample_step: step %d outside 0 .. ids_ld - 1 = %lld", step, (long long)ids_ld - 1);
  JS2T_CHECK(eos >= 0 && eos < V && pad >= 0 && pad < V, "sample_step: eos %lld / pad %lld outside the vocabulary", (long long)eos,
             (long long)pad);
  JS2T_CHECK(ld >= 0, "sample_step: negative row distance %lld", (long long)ld);
  if (rows == 0) return JS2T_OK;
  JS2T_CHECK(logits && u && ids && out_logp, "sample_step: null pointer");
  SampleArgs a;
  a.logits = logits, a.ld = ld, a.u = u, a.finished = finished, a.ids = ids, a.ids_ld = ids_ld, a.step = step;
  a.out_logp = out_logp, a.out_q = out_q, a.score = score, a.length = length, a.out_kept = out_kept, a.out_cdf = out_cdf;
  a.V = (int32_t)V;
  a.inv_t = fminf(1.f / temperature, FLT_MAX);
  a.top_k = top_k > V ? (int32_t)V : top_k;
  a.top_p = top_p, a.epsilon = epsilon, a.eos = eos, a.pad = pad;
  a.fb.n = n_forbid;
  for (int i = 0; i < SP_MAX_FORBID; ++i) a.fb.ids[i] = i < n_forbid ? forbid_ids[i] : -1;
  if (V <= SP_LDS_V) {
    hipLaunchKernelGGL(sample_step_kernel<true>, dim3((unsigned)rows), dim3(SP_THREADS), (size_t)V * sizeof(float), (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(sample_step_kernel<false>, dim3((unsigned)rows), dim3(SP_THREADS), 0, (hipStream_t)stream, a);
  }
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}
