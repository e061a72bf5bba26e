// CTC prefix beam search (EXTENSION; the reference has no encoder-only n-best decoder): the beam search over the CTC output alone,
// summing over ALL alignments of a labelling (Graves' prefix search restricted to a beam; the recursion is stated in the header).
// One block per utterance, like the loss and the aligner: the search is a chain of T_b dependent steps.  Per frame the block builds
// the <= K + K C proposals (one thread each: K "stay" proposals - the beam's prefixes themselves - and one per (prefix, candidate)
// pair), folds the extensions that ARE a prefix of the beam into that prefix, ranks the rest by counting and writes the K best as
// the next beam.  Two block barriers per frame; every loop that holds one is bounded by T_b, which is block-uniform.
//
// Prefix identity is (64-bit hash of the token sequence, length), not the trie node: a prefix that was pruned and is created again
// gets a new node but the same hash, so an extension of the new node still meets the surviving child of the old one.  With an
// exact identity two extensions can never coincide (equal sequences have equal parents, and the beam's prefixes are distinct), so
// an extension can only coincide with a stay proposal - which is why folding is a scan over the beam and needs no sort.
//
// No atomics, no allocation, no host synchronisation; every trie node has a fixed slot (1 + t K + rank), so nothing is counted and
// nothing read from the workspace that this launch has not written: bit-reproducible, capturable.
//
// LM shallow fusion (js2t_ctc_beam_search_lm) is the same kernel body with LM = true: every prefix carries lm(y), the ascending f32
// sum of ngram.hpp's token values, and the two tokens in front of its last one (the LM's context); the frame's ranking key gains
// lm_weight * lm(y) + length_bonus * |y| while pb / pnb / tot stay pure CTC masses.  An extension's thread computes its own
// ngram_token_logp in phase A - five independent first probes issued together, one memory latency; a probe that meets another key
// walks on as ngram.hpp says, and those walks are most of what the LM costs a frame - and there is no further
// barrier and no other global traffic per frame.  After the last frame one wave adds the EOS term,
// ranks the beam again by counting and the back-trace runs in that order.  With LM = false none of it is compiled: that form is
// what js2t_ctc_beam_search launches.
//
// Contextual biasing (js2t_ctc_beam_search_ctx) is the LM form with CTX = true on top: every prefix carries context.hpp's state
// (node, bank, depth of the node) and the key gains context_weight * m(y), m = bank + depth.  An extension's thread takes its
// context_step in phase A beside its ngram_token_logp - at the root, where most prefixes are, one probe of the edge table; only a
// failing match reads node records - a stay proposal copies its state, and there is no new barrier.  The epilogue adds keep in
// place of depth (ctx(y)) and writes out_ctx in final order.  Like lm(y), the state is a function of the label sequence alone, so
// the identity rule carries over.  With CTX = false none of it is compiled.
//
// The limit on the beam, the fusion rule, the final ranking and the hash's finaliser are nbest.hpp's, shared with rescore.hip and
// ngram.hip, so the list this kernel writes is ranked as they rank it; the checks of the LM arguments are ngram.hpp's ngram_args.
#include "common.hpp"
#include "nbest.hpp"
#include "ngram.hpp"
#include "context.hpp"

namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_MAX_K = NBEST_MAX_N;                       // a beam is an n-best list: one lane per slot in the final ranking
constexpr int CB_MAX_C = 8;                                 // the limit of js2t_beam_pick
constexpr int CB_MAX_E = CB_MAX_K + CB_MAX_K * CB_MAX_C;    // proposals per frame: 288 (a multiple of 4)
constexpr int CB_CHUNK = 64;                                // frames whose candidate rows are staged at a time: 4.25 KB of LDS
constexpr int CB_IGNORED = -2;                              // staged id of a candidate that is ignored (-1 is the root's "last token")
constexpr uint64_t CB_ROOT_HASH = 0x9E3779B97F4A7C15ull;

// h(y + c) = fmix(h(y) ^ (c + 1)), fmix = the finaliser of splitmix64 (a bijection of 64-bit words; h ^ (c + 1) is injective in c,
// so the children of one prefix never collide)
__device__ __forceinline__ uint64_t cb_mix(uint64_t h, int c) { return nbest_fmix(h ^ (uint64_t)(uint32_t)(c + 1)); }

// log(exp a + exp b) on the hardware's exp / log (beam.hip ctc_lae_fast: absolute error ~1e-7 per call); lae(-inf, x) = x, never NaN
__device__ __forceinline__ float cb_lae(float a, float b) {
  const float m = fmaxf(a, b);
  if (!(m > -INFINITY)) return -INFINITY;
  return m + __logf(1.f + __expf(fminf(a, b) - m));
}

// does proposal (kp, ep) come before proposal (k, e)?  Larger score first, then the lower proposal index.  A NaN key (no proposal)
// comes before nothing.
__device__ __forceinline__ int cb_before(float kp, int ep, float k, int e) { return (kp > k || (kp == k && ep < e)) ? 1 : 0; }

template <bool LM, bool CTX>
struct CbBeam {  // one of the two beams; slot = rank of the prefix (key descending)
  float pb[CB_MAX_K], pnb[CB_MAX_K], tot[CB_MAX_K];  // log-mass ending in blank / in non-blank, and their logaddexp
  uint64_t hash[CB_MAX_K], phash[CB_MAX_K];         // of the prefix, and of the prefix without its last token
  int len[CB_MAX_K], last[CB_MAX_K], node[CB_MAX_K];
  float lm[LM ? CB_MAX_K : 1];                      // LM only: lm(y), and the second and third newest tokens of (bos, y), -1 = none
  int t1[LM ? CB_MAX_K : 1], t2[LM ? CB_MAX_K : 1];
  int cnode[CTX ? CB_MAX_K : 1], cbank[CTX ? CB_MAX_K : 1], cdep[CTX ? CB_MAX_K : 1];  // CTX only: context.hpp's state of the prefix
};

struct CbFuse {  // what the LM form takes besides the search's own arguments
  ngram_view lm;
  int bos, eos;
  float lm_weight, length_bonus;
  float *out_ctc, *out_lm;
  context_view ctx;  // what the CTX form takes on top (behind the LM form's: their offsets stay)
  float ctx_weight;
  int32_t* out_ctx;
};

// log p(w | (bos, y)) for the prefix y in slot i of the beam
template <bool LM, bool CTX>
__device__ __forceinline__ float cb_token_logp(const CbFuse& f, const CbBeam<LM, CTX>& g, int i, int w) {
  const int len = g.len[i];
  const int64_t c[NGRAM_MAX_CTX] = {len > 0 ? g.last[i] : f.bos, g.t1[i], g.t2[i]};
  return ngram_token_logp(f.lm, w, c, len + 1 < NGRAM_MAX_CTX ? len + 1 : NGRAM_MAX_CTX);
}

template <typename T, bool LM, bool CTX>
__global__ __launch_bounds__(CB_THREADS) void ctc_beam_kernel(
    const T* __restrict__ x, const float* __restrict__ lse, const int64_t* __restrict__ cand_id, const float* __restrict__ cand_lp,
    const int64_t* __restrict__ in_len, int64_t* __restrict__ out_ids, int32_t* __restrict__ out_len, float* __restrict__ out_score,
    int2* __restrict__ nodes_all, int64_t Tmax, int64_t V, int K, int C, int n_best, int blank, int64_t pad,
    const int32_t* __restrict__ rowoff, const CbFuse fuse) {
  static_assert(LM || !CTX, "the context form is built on the LM form");
  __shared__ CbBeam<LM, CTX> beam[2];
  __shared__ int s_enode[CTX ? CB_MAX_E : 1], s_ebank[CTX ? CB_MAX_E : 1], s_edep[CTX ? CB_MAX_E : 1];  // CTX only: every proposal's state
  __shared__ int s_ctx[CTX ? CB_MAX_K : 1];             // CTX only: ctx(y) per beam slot
  __shared__ float s_elm[LM ? CB_MAX_E : 1];            // LM only: lm(y) of every proposal of the frame
  __shared__ int s_ord[LM ? CB_MAX_K : 1];              // LM only: beam slot of the k-th best by the final score
  __shared__ float s_fin[LM ? CB_MAX_K : 1], s_lmf[LM ? CB_MAX_K : 1];  // final score and lm(y) + p(eos | y) per beam slot
  __shared__ __align__(16) float s_key[CB_MAX_E];       // score of every proposal of the frame, NaN where there is none
  __shared__ float s_epb[CB_MAX_E], s_epnb[CB_MAX_E];   // its two masses
  __shared__ int s_cid[CB_CHUNK][CB_MAX_C];
  __shared__ float s_clp[CB_CHUNK][CB_MAX_C];
  __shared__ float s_lpb[CB_CHUNK];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t Tb = max((int64_t)0, min(in_len[b], Tmax));
  const int64_t r0 = rowoff ? (int64_t)rowoff[b] : (int64_t)b * Tmax;  // first logits / lse / candidate row of the utterance
  int2* nodes = nodes_all + (int64_t)b * (1 + (int64_t)K * Tmax);     // (parent node, token); node 0 = the empty prefix, never read
  const float nan = __int_as_float(0x7fc00000);
  if (tid == 0) {
    CbBeam<LM, CTX>& g = beam[0];
    g.pb[0] = 0.f, g.pnb[0] = -INFINITY, g.tot[0] = 0.f;
    g.hash[0] = CB_ROOT_HASH, g.phash[0] = 0;
    g.len[0] = 0, g.last[0] = -1, g.node[0] = 0;
    if constexpr (LM) g.lm[0] = 0.f, g.t1[0] = -1, g.t2[0] = -1;
    if constexpr (CTX) g.cnode[0] = 0, g.cbank[0] = 0, g.cdep[0] = 0;
  }
  int cur = 0, nbeam = 1;
  __syncthreads();
  for (int64_t c0 = 0; c0 < Tb; c0 += CB_CHUNK) {  // (block-uniform bounds: Tb)
    const int nt = (int)min((int64_t)CB_CHUNK, Tb - c0);
    for (int i = tid; i < nt * C; i += CB_THREADS) {  // stage the candidate rows of this chunk of frames
      const int tt = i / C, s = i - tt * C;
      const int64_t at = (r0 + c0 + tt) * C + s;
      const int64_t id = cand_id[at];
      const float lp = cand_lp[at];
      const bool ok = id >= 0 && id < V && id != (int64_t)blank && lp > -INFINITY;  // (a NaN is ignored too)
      s_cid[tt][s] = ok ? (int)id : CB_IGNORED;
      s_clp[tt][s] = ok ? lp : -INFINITY;
    }
    for (int tt = tid; tt < nt; tt += CB_THREADS) {
      const int64_t r = r0 + c0 + tt;
      s_lpb[tt] = io<T>::ld(x + r * V + blank) - lse[r];
    }
    __syncthreads();
    for (int tt = 0; tt < nt; ++tt) {  // (block-uniform bounds: nt)
      const CbBeam<LM, CTX>& g = beam[cur];
      CbBeam<LM, CTX>& gn = beam[cur ^ 1];
      const int nlive = K + nbeam * C, npad = (nlive + 3) & ~3;  // proposals 0 .. K-1 stay, K + i C + s extends prefix i by slot s
      const float lpb = s_lpb[tt];
      // ---- phase A: the proposals
      for (int q = tid; q < npad; q += CB_THREADS) {
        // LM: the extensions (at most 256) come first, one thread each, so that all their probes are in flight together
        const int e = !LM ? q : q < npad - K ? q + K : q - (npad - K);
        float npb = -INFINITY, npnb = -INFINITY, key = nan, elm = 0.f;
        context_state cs{0, 0, 0};
        if (e < nbeam) {  // prefix e stays: blank, a repeat of its last label, and the extension of its parent that recreates it
          const int last = g.last[e], len = g.len[e];
          npb = g.tot[e] + lpb;
          float lp_rep = -INFINITY;
          for (int s = 0; s < C; ++s)
            if (s_cid[tt][s] == last) lp_rep = s_clp[tt][s];
          npnb = g.pnb[e] + lp_rep;
          if (lp_rep > -INFINITY && len > 0) {
            const uint64_t ph = g.phash[e];
            for (int i = 0; i < nbeam; ++i)
              if (g.len[i] + 1 == len && g.hash[i] == ph) npnb = cb_lae(npnb, (g.last[i] == last ? g.pb[i] : g.tot[i]) + lp_rep);
          }
          key = cb_lae(npb, npnb);
          if constexpr (CTX) {  // a stay proposal copies its state
            elm = g.lm[e], cs = context_state{g.cnode[e], g.cbank[e], g.cdep[e]};
            key = nbest_fuse_ctx(key, elm, cs.bank + cs.depth, len, fuse.lm_weight, fuse.ctx_weight, fuse.length_bonus);
          } else if constexpr (LM) {
            elm = g.lm[e], key = nbest_fuse(key, elm, len, fuse.lm_weight, fuse.length_bonus);
          }
        } else if (e >= K && e < nlive) {
          const int i = (e - K) / C, s = (e - K) - i * C;
          const int c = s_cid[tt][s];
          if (c != CB_IGNORED) {
            const bool rep = c == g.last[i];
            const float base = rep ? g.pb[i] : g.tot[i];
            bool ok = !(rep && !(base > -INFINITY));
            const int len1 = g.len[i] + 1;
            const uint64_t h = g.hash[i];
            for (int j = 0; j < nbeam; ++j)  // the beam holds this very sequence: its stay proposal has taken the mass
              if (g.len[j] == len1 && g.last[j] == c && g.phash[j] == h) ok = false;
            if constexpr (LM) {
              if (ok && fuse.lm_weight != 0.f) {
                elm = g.lm[i] + cb_token_logp(fuse, g, i, c);
                ok = elm > -INFINITY;  // an extension the LM forbids (-inf, or NaN) is not proposed
              }
            }
            if constexpr (CTX) {  // m(y + c): the walk's step, beside the LM's probes; a weight of 0 reads no graph
              if (ok && fuse.ctx_weight != 0.f) cs = context_step(fuse.ctx, context_state{g.cnode[i], g.cbank[i], g.cdep[i]}, c);
            }
            if (ok) {
              npnb = base + s_clp[tt][s];
              key = npnb;
              if constexpr (CTX)
                key = nbest_fuse_ctx(key, elm, cs.bank + cs.depth, len1, fuse.lm_weight, fuse.ctx_weight, fuse.length_bonus);
              else if constexpr (LM)
                key = nbest_fuse(key, elm, len1, fuse.lm_weight, fuse.length_bonus);
            }
          }
        }
        s_key[e] = key, s_epb[e] = npb, s_epnb[e] = npnb;
        if constexpr (LM) s_elm[e] = elm;
        if constexpr (CTX) s_enode[e] = cs.node, s_ebank[e] = cs.bank, s_edep[e] = cs.depth;
      }
      __syncthreads();
      // ---- phase B: rank by counting, the K first become the next beam
      int nv = 0;
      for (int e = tid; e < CB_MAX_E; e += CB_THREADS) {  // every thread runs the first round (it needs nv); wave 0 at most a second
        if (e >= CB_THREADS && e >= nlive) break;
        const float k = e < npad ? s_key[e] : nan;
        int rank = 0;
        nv = 0;
        for (int q = 0; q < npad; q += 4) {
          const float4 v = *(const float4*)&s_key[q];
          rank += cb_before(v.x, q, k, e) + cb_before(v.y, q + 1, k, e) + cb_before(v.z, q + 2, k, e) + cb_before(v.w, q + 3, k, e);
          nv += (v.x == v.x ? 1 : 0) + (v.y == v.y ? 1 : 0) + (v.z == v.z ? 1 : 0) + (v.w == v.w ? 1 : 0);
        }
        if (k == k && rank < K) {
          gn.pb[rank] = s_epb[e], gn.pnb[rank] = s_epnb[e];
          if constexpr (CTX) gn.cnode[rank] = s_enode[e], gn.cbank[rank] = s_ebank[e], gn.cdep[rank] = s_edep[e];
          if constexpr (LM) {  // the key is no longer the CTC total: an extension's is its pnb, a stay's is recomputed
            gn.tot[rank] = e < K ? cb_lae(s_epb[e], s_epnb[e]) : s_epnb[e];
            gn.lm[rank] = s_elm[e];
          } else {
            gn.tot[rank] = k;
          }
          if (e < K) {
            gn.hash[rank] = g.hash[e], gn.phash[rank] = g.phash[e];
            gn.len[rank] = g.len[e], gn.last[rank] = g.last[e], gn.node[rank] = g.node[e];
            if constexpr (LM) gn.t1[rank] = g.t1[e], gn.t2[rank] = g.t2[e];
          } else {
            const int i = (e - K) / C, s = (e - K) - i * C;
            const int c = s_cid[tt][s];
            const int node = 1 + (int)(c0 + tt) * K + rank;  // only survivors get nodes: slot `rank` of this frame's K
            gn.hash[rank] = cb_mix(g.hash[i], c), gn.phash[rank] = g.hash[i];
            gn.len[rank] = g.len[i] + 1, gn.last[rank] = c, gn.node[rank] = node;
            nodes[node] = make_int2(g.node[i], c);
            if constexpr (LM) gn.t1[rank] = g.len[i] > 0 ? g.last[i] : fuse.bos, gn.t2[rank] = g.t1[i];
          }
        }
      }
      __syncthreads();
      cur ^= 1;
      nbeam = min(K, nv);  // (block-uniform: every thread has counted the same keys)
    }
  }
  // the beam is in score order already: its first n_best slots are the result; the barrier that closed the last frame made it, and
  // the nodes (workgroup scope), visible
  const CbBeam<LM, CTX>& g = beam[cur];
  if constexpr (LM) {
    // the EOS term and the final score, lanes < nbeam of the first wave; ranked again by nbest.hpp's rule (equal finals keep the
    // beam's order, a NaN ranks as -inf); the back-trace below runs in that order
    if (tid < 64) {  // (wave-uniform)
      const bool have = tid < nbeam;
      float lmf = 0.f, fin = -INFINITY;
      int ctxv = 0;  // CTX: ctx(y) - keep in place of depth: a partial match that never completed earns nothing
      if (have) {
        if (fuse.lm_weight != 0.f) lmf = g.lm[tid] + cb_token_logp(fuse, g, tid, fuse.eos);
        if constexpr (CTX) {
          if (fuse.ctx_weight != 0.f) ctxv = context_final(fuse.ctx, context_state{g.cnode[tid], g.cbank[tid], g.cdep[tid]});
          fin = nbest_fuse_ctx(g.tot[tid], lmf, ctxv, g.len[tid], fuse.lm_weight, fuse.ctx_weight, fuse.length_bonus);
        } else {
          fin = nbest_fuse(g.tot[tid], lmf, g.len[tid], fuse.lm_weight, fuse.length_bonus);
        }
      }
      const int rank = nbest_rank(fin, tid, nbeam);  // (block-uniform nbeam)
      if (have) s_ord[rank] = tid, s_fin[tid] = fin, s_lmf[tid] = lmf;
      if constexpr (CTX) {
        if (have) s_ctx[tid] = ctxv;
      }
    }
    __syncthreads();
  }
  int64_t* oi = out_ids + (int64_t)b * n_best * Tmax;
  for (int64_t idx = tid; idx < (int64_t)n_best * Tmax; idx += CB_THREADS) {
    const int n = (int)(idx / Tmax);
    if (n >= nbeam || idx - n * Tmax >= g.len[LM ? s_ord[n] : n]) oi[idx] = pad;
  }
  if (tid < n_best) {
    const bool have = tid < nbeam;
    const int from = have && LM ? s_ord[tid] : tid;  // the beam slot returned in output slot tid
    if constexpr (LM) {
      out_score[(int64_t)b * n_best + tid] = have ? s_fin[from] : -INFINITY;
      fuse.out_ctc[(int64_t)b * n_best + tid] = have ? g.tot[from] : -INFINITY;
      fuse.out_lm[(int64_t)b * n_best + tid] = have ? s_lmf[from] : -INFINITY;
      if constexpr (CTX) fuse.out_ctx[(int64_t)b * n_best + tid] = have ? s_ctx[from] : 0;
    } else {
      out_score[(int64_t)b * n_best + tid] = have ? g.tot[tid] : -INFINITY;
    }
    out_len[(int64_t)b * n_best + tid] = have ? g.len[from] : 0;
    if (have) {
      int node = g.node[from];
      for (int p = g.len[from] - 1; p >= 0; --p) {
        const int2 nd = nodes[node];
        oi[(int64_t)tid * Tmax + p] = nd.y;
        node = nd.x;
      }
    }
  }
}

// the checks the two entry points share, and the launch; `who` names the entry point in the messages
template <bool LM, bool CTX>
int cb_launch(const char* who, const void* logits, int dt, const float* lse, const int64_t* cand_id, const float* cand_lp,
              const int64_t* in_len, int64_t* out_ids, int32_t* out_len, float* out_score, void* workspace, int64_t B, int64_t T_, int64_t V,
              int32_t beam, int32_t n_cand, int32_t n_best, int64_t blank, int64_t pad, const int32_t* row_offsets, const CbFuse& fuse,
              js2t_stream stream) {
  JS2T_CHECK(logits && lse && cand_id && cand_lp && in_len && out_ids && out_len && out_score && workspace, "%s: null pointer", who);
  JS2T_CHECK(B > 0 && T_ > 0 && V > 0 && V < 0x7fffffff, "%s: bad shape", who);
  JS2T_CHECK(beam >= 1 && beam <= CB_MAX_K, "%s: beam %d outside 1..%d", who, (int)beam, CB_MAX_K);
  JS2T_CHECK(n_cand >= 1 && n_cand <= CB_MAX_C, "%s: %d candidates outside 1..%d", who, (int)n_cand, CB_MAX_C);
  JS2T_CHECK(n_best >= 1 && n_best <= beam, "%s: n_best %d outside 1..beam (%d)", who, (int)n_best, (int)beam);
  JS2T_CHECK(T_ < (int64_t(1) << 31) / CB_MAX_K, "%s: %lld frames exceed the node index", who, (long long)T_);
  JS2T_CHECK(blank >= 0 && blank < V, "%s: blank %lld outside the vocabulary", who, (long long)blank);
  JS2T_CHECK(dt == JS2T_F32 || dt == JS2T_BF16, "bad dtype %d", dt);
  if (dt == JS2T_F32)
    hipLaunchKernelGGL((ctc_beam_kernel<float, LM, CTX>), dim3((unsigned)B), dim3(CB_THREADS), 0, (hipStream_t)stream, (const float*)logits, lse,
                       cand_id, cand_lp, in_len, out_ids, out_len, out_score, (int2*)workspace, T_, V, (int)beam, (int)n_cand, (int)n_best,
                       (int)blank, pad, row_offsets, fuse);
  else
    hipLaunchKernelGGL((ctc_beam_kernel<uint16_t, LM, CTX>), dim3((unsigned)B), dim3(CB_THREADS), 0, (hipStream_t)stream, (const uint16_t*)logits,
                       lse, cand_id, cand_lp, in_len, out_ids, out_len, out_score, (int2*)workspace, T_, V, (int)beam, (int)n_cand,
                       (int)n_best, (int)blank, pad, row_offsets, fuse);
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}

inline int64_t cb_nodes_per_utt(int64_t T, int64_t K) { return 1 + K * T; }

}  // namespace

extern "C" int64_t js2t_ctc_beam_workspace_bytes(int64_t B, int64_t T, int32_t beam) {
  if (B <= 0 || T <= 0 || beam <= 0) return 0;
  return B * cb_nodes_per_utt(T, beam) * (int64_t)sizeof(int2);
}

extern "C" int js2t_ctc_beam_search(const void* logits, int dt, const float* lse, const int64_t* cand_id, const float* cand_lp,
                                    const int64_t* in_len, int64_t* out_ids, int32_t* out_len, float* out_score, void* workspace,
                                    int64_t B, int64_t T_, int64_t V, int32_t beam, int32_t n_cand, int32_t n_best, int64_t blank,
                                    int64_t pad, const int32_t* row_offsets, js2t_stream stream) {
  if (B == 0) return JS2T_OK;
  return cb_launch<false, false>("ctc_beam_search", logits, dt, lse, cand_id, cand_lp, in_len, out_ids, out_len, out_score, workspace, B, T_, V, beam,
                          n_cand, n_best, blank, pad, row_offsets, CbFuse{}, stream);
}

extern "C" int js2t_ctc_beam_search_lm(const void* logits, int dt, const float* lse, const int64_t* cand_id, const float* cand_lp,
                                       const int64_t* in_len, const float* uni, const void* table, int64_t capacity, int32_t max_probe,
                                       int32_t lm_order, int64_t* out_ids, int32_t* out_len, float* out_score, float* out_ctc, float* out_lm,
                                       void* workspace, int64_t B, int64_t T_, int64_t V, int32_t beam, int32_t n_cand, int32_t n_best,
                                       int64_t blank, int64_t pad, int64_t bos, int64_t eos, float lm_weight, float length_bonus,
                                       const int32_t* row_offsets, js2t_stream stream) {
  if (B == 0) return JS2T_OK;
  const char* who = "ctc_beam_search_lm";
  JS2T_CHECK(out_ctc && out_lm, "%s: null pointer (out_ctc / out_lm)", who);
  CbFuse fuse{};
  if (const int rc = ngram_args(who, uni, table, capacity, max_probe, lm_order, V, bos, eos, lm_weight, length_bonus, &fuse.lm)) return rc;
  fuse.bos = (int)bos, fuse.eos = (int)eos, fuse.lm_weight = lm_weight, fuse.length_bonus = length_bonus;
  fuse.out_ctc = out_ctc, fuse.out_lm = out_lm;
  return cb_launch<true, false>(who, logits, dt, lse, cand_id, cand_lp, in_len, out_ids, out_len, out_score, workspace, B, T_, V, beam, n_cand, n_best,
                         blank, pad, row_offsets, fuse, stream);
}

extern "C" int js2t_ctc_beam_search_ctx(const void* logits, int dt, const float* lse, const int64_t* cand_id, const float* cand_lp,
                                        const int64_t* in_len, const float* uni, const void* table, int64_t capacity, int32_t max_probe,
                                        int32_t lm_order, const void* ctx_nodes, const void* ctx_edges, int64_t ctx_capacity,
                                        int32_t ctx_max_probe, int32_t ctx_n_nodes, int32_t ctx_max_fail, int64_t* out_ids, int32_t* out_len,
                                        float* out_score, float* out_ctc, float* out_lm, int32_t* out_ctx, void* workspace, int64_t B,
                                        int64_t T_, int64_t V, int32_t beam, int32_t n_cand, int32_t n_best, int64_t blank, int64_t pad,
                                        int64_t bos, int64_t eos, float lm_weight, float context_weight, float length_bonus,
                                        const int32_t* row_offsets, js2t_stream stream) {
  if (B == 0) return JS2T_OK;
  const char* who = "ctc_beam_search_ctx";
  JS2T_CHECK(out_ctc && out_lm && out_ctx, "%s: null pointer (out_ctc / out_lm / out_ctx)", who);
  CbFuse fuse{};
  if (const int rc = ngram_args(who, uni, table, capacity, max_probe, lm_order, V, bos, eos, lm_weight, length_bonus, &fuse.lm)) return rc;
  if (const int rc = context_args(who, ctx_nodes, ctx_edges, ctx_capacity, ctx_max_probe, ctx_n_nodes, ctx_max_fail, V, context_weight, &fuse.ctx))
    return rc;
  fuse.bos = (int)bos, fuse.eos = (int)eos, fuse.lm_weight = lm_weight, fuse.length_bonus = length_bonus;
  fuse.out_ctc = out_ctc, fuse.out_lm = out_lm, fuse.ctx_weight = context_weight, fuse.out_ctx = out_ctx;
  return cb_launch<true, true>(who, logits, dt, lse, cand_id, cand_lp, in_len, out_ids, out_len, out_score, workspace, B, T_, V, beam, n_cand,
                               n_best, blank, pad, row_offsets, fuse, stream);
}
