// The CTC prefix beam search's frame recursion, EOS epilogue and back-trace, stated ONCE: ctc_beam.hip (a whole utterance per launch)
// and ctc_stream.hip (a resumable step) instantiate the same functions, so a segment decoded in pieces has the bits of the
// segment decoded at once.  What the recursion is, the prefix identity, the LM and CTX forms: ctc_beam.hip's head comment and
// include/joeys2t_hip.h.
//
// Every function here is called by ALL 256 threads of the block with block-uniform arguments; the barriers inside are stated per
// function.  The LDS of a block is one CbLds.
#pragma once
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
  float *out_ctc, *out_lm;  // (the one-shot entry points' outputs; the functions here write through a CbOut)
  context_view ctx;  // what the CTX form takes on top (behind the LM form's: their offsets stay)
  float ctx_weight;
  int32_t* out_ctx;
};

struct CbOut {  // where one utterance's n-best list goes: ids [n_best, stride], the rest [n_best]
  int64_t* ids;
  int64_t stride;
  int32_t* len;
  float *score, *ctc, *lm;  // ctc / lm: LM forms only
  int32_t* ctx;             // CTX form only
};

template <bool LM, bool CTX>
struct CbLds {  // a block's LDS
  CbBeam<LM, CTX> beam[2];
  int enode[CTX ? CB_MAX_E : 1], ebank[CTX ? CB_MAX_E : 1], edep[CTX ? CB_MAX_E : 1];  // CTX only: every proposal's state
  int ctx[CTX ? CB_MAX_K : 1];             // CTX only: ctx(y) per beam slot
  float elm[LM ? CB_MAX_E : 1];            // LM only: lm(y) of every proposal of the frame
  int ord[LM ? CB_MAX_K : 1];              // LM only: beam slot of the k-th best by the final score
  float fin[LM ? CB_MAX_K : 1], lmf[LM ? CB_MAX_K : 1];  // final score and lm(y) + p(eos | y) per beam slot
  __align__(16) float key[CB_MAX_E];       // score of every proposal of the frame, NaN where there is none
  float epb[CB_MAX_E], epnb[CB_MAX_E];     // its two masses
  int cid[CB_CHUNK][CB_MAX_C];
  float clp[CB_CHUNK][CB_MAX_C];
  float lpb[CB_CHUNK];
};

// log p(w | (bos, y)) for the prefix y in slot i of the beam
template <bool LM, bool CTX>
__device__ __forceinline__ float cb_token_logp(const CbFuse& f, const CbBeam<LM, CTX>& g, int i, int w) {
  const int len = g.len[i];
  const int64_t c[NGRAM_MAX_CTX] = {len > 0 ? g.last[i] : f.bos, g.t1[i], g.t2[i]};
  return ngram_token_logp(f.lm, w, c, len + 1 < NGRAM_MAX_CTX ? len + 1 : NGRAM_MAX_CTX);
}

// the beam of frame 0: the empty prefix in slot 0 (ONE thread calls this; the caller's barrier publishes it)
template <bool LM, bool CTX>
__device__ __forceinline__ void cb_root(CbBeam<LM, CTX>& g) {
  g.pb[0] = 0.f, g.pnb[0] = -INFINITY, g.tot[0] = 0.f;
  g.hash[0] = CB_ROOT_HASH, g.phash[0] = 0;
  g.len[0] = 0, g.last[0] = -1, g.node[0] = 0;
  if constexpr (LM) g.lm[0] = 0.f, g.t1[0] = -1, g.t2[0] = -1;
  if constexpr (CTX) g.cnode[0] = 0, g.cbank[0] = 0, g.cdep[0] = 0;
}

// stage the candidate rows and lp(blank) of the nt (<= CB_CHUNK) frames whose first row is `row`; no barrier: the caller's
template <typename T, bool LM, bool CTX>
__device__ __forceinline__ void cb_stage(CbLds<LM, CTX>& sh, const T* __restrict__ x, const float* __restrict__ lse,
                                         const int64_t* __restrict__ cand_id, const float* __restrict__ cand_lp, int64_t row, int nt,
                                         int64_t V, int C, int blank) {
  const int tid = threadIdx.x;
  for (int i = tid; i < nt * C; i += CB_THREADS) {
    const int tt = i / C, s = i - tt * C;
    const int64_t at = (row + tt) * C + s;
    const int64_t id = cand_id[at];
    const float lp = cand_lp[at];
    const bool ok = id >= 0 && id < V && id != (int64_t)blank && lp > -INFINITY;  // (a NaN is ignored too)
    sh.cid[tt][s] = ok ? (int)id : CB_IGNORED;
    sh.clp[tt][s] = ok ? lp : -INFINITY;
  }
  for (int tt = tid; tt < nt; tt += CB_THREADS) {
    const int64_t r = row + tt;
    sh.lpb[tt] = io<T>::ld(x + r * V + blank) - lse[r];
  }
}

// one frame: staged frame tt, the t-th of its utterance (its survivors get the trie nodes 1 + t K + rank); reads sh.beam[cur] with
// nbeam live slots, writes sh.beam[cur ^ 1] and returns its live slots (block-uniform).  Two barriers, the second behind the last
// write: on return the new beam and the nodes (workgroup scope) are visible.
template <bool LM, bool CTX>
__device__ __forceinline__ int cb_frame(CbLds<LM, CTX>& sh, int cur, int nbeam, int tt, int t, int K, int C, int2* __restrict__ nodes,
                                        const CbFuse& fuse) {
  const int tid = threadIdx.x;
  const float nan = __int_as_float(0x7fc00000);
  const CbBeam<LM, CTX>& g = sh.beam[cur];
  CbBeam<LM, CTX>& gn = sh.beam[cur ^ 1];
  const int nlive = K + nbeam * C, npad = (nlive + 3) & ~3;  // proposals 0 .. K-1 stay, K + i C + s extends prefix i by slot s
  const float lpb = sh.lpb[tt];
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
        if (sh.cid[tt][s] == last) lp_rep = sh.clp[tt][s];
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
      const int c = sh.cid[tt][s];
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
          npnb = base + sh.clp[tt][s];
          key = npnb;
          if constexpr (CTX)
            key = nbest_fuse_ctx(key, elm, cs.bank + cs.depth, len1, fuse.lm_weight, fuse.ctx_weight, fuse.length_bonus);
          else if constexpr (LM)
            key = nbest_fuse(key, elm, len1, fuse.lm_weight, fuse.length_bonus);
        }
      }
    }
    sh.key[e] = key, sh.epb[e] = npb, sh.epnb[e] = npnb;
    if constexpr (LM) sh.elm[e] = elm;
    if constexpr (CTX) sh.enode[e] = cs.node, sh.ebank[e] = cs.bank, sh.edep[e] = cs.depth;
  }
  __syncthreads();
  // ---- phase B: rank by counting, the K first become the next beam
  int nv = 0;
  for (int e = tid; e < CB_MAX_E; e += CB_THREADS) {  // every thread runs the first round (it needs nv); wave 0 at most a second
    if (e >= CB_THREADS && e >= nlive) break;
    const float k = e < npad ? sh.key[e] : nan;
    int rank = 0;
    nv = 0;
    for (int q = 0; q < npad; q += 4) {
      const float4 v = *(const float4*)&sh.key[q];
      rank += cb_before(v.x, q, k, e) + cb_before(v.y, q + 1, k, e) + cb_before(v.z, q + 2, k, e) + cb_before(v.w, q + 3, k, e);
      nv += (v.x == v.x ? 1 : 0) + (v.y == v.y ? 1 : 0) + (v.z == v.z ? 1 : 0) + (v.w == v.w ? 1 : 0);
    }
    if (k == k && rank < K) {
      gn.pb[rank] = sh.epb[e], gn.pnb[rank] = sh.epnb[e];
      if constexpr (CTX) gn.cnode[rank] = sh.enode[e], gn.cbank[rank] = sh.ebank[e], gn.cdep[rank] = sh.edep[e];
      if constexpr (LM) {  // the key is no longer the CTC total: an extension's is its pnb, a stay's is recomputed
        gn.tot[rank] = e < K ? cb_lae(sh.epb[e], sh.epnb[e]) : sh.epnb[e];
        gn.lm[rank] = sh.elm[e];
      } else {
        gn.tot[rank] = k;
      }
      if (e < K) {
        gn.hash[rank] = g.hash[e], gn.phash[rank] = g.phash[e];
        gn.len[rank] = g.len[e], gn.last[rank] = g.last[e], gn.node[rank] = g.node[e];
        if constexpr (LM) gn.t1[rank] = g.t1[e], gn.t2[rank] = g.t2[e];
      } else {
        const int i = (e - K) / C, s = (e - K) - i * C;
        const int c = sh.cid[tt][s];
        const int node = 1 + t * K + rank;  // only survivors get nodes: slot `rank` of this frame's K
        gn.hash[rank] = cb_mix(g.hash[i], c), gn.phash[rank] = g.hash[i];
        gn.len[rank] = g.len[i] + 1, gn.last[rank] = c, gn.node[rank] = node;
        nodes[node] = make_int2(g.node[i], c);
        if constexpr (LM) gn.t1[rank] = g.len[i] > 0 ? g.last[i] : fuse.bos, gn.t2[rank] = g.t1[i];
      }
    }
  }
  __syncthreads();
  return min(K, nv);  // (block-uniform: every thread has counted the same keys)
}

// LM forms, after the last frame: the EOS term and the final score of the beam g (= sh.beam[cur]), lanes < nbeam of the first wave;
// ranked again by nbest.hpp's rule (equal finals keep the beam's order, a NaN ranks as -inf) into sh.ord.  One barrier at the end.
// Without an LM there is nothing to do: the beam is in score order already.
template <bool LM, bool CTX>
__device__ __forceinline__ void cb_finish(CbLds<LM, CTX>& sh, const CbBeam<LM, CTX>& g, int nbeam, const CbFuse& fuse) {
  if constexpr (LM) {
    const int tid = threadIdx.x;
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
      if (have) sh.ord[rank] = tid, sh.fin[tid] = fin, sh.lmf[tid] = lmf;
      if constexpr (CTX) {
        if (have) sh.ctx[tid] = ctxv;
      }
    }
    __syncthreads();
  }
}

// the n_best first of the beam g (behind cb_finish) as one utterance's list: ids pad-filled over o.stride columns, the lengths and
// scores, the labels by the back-trace through `nodes`.  No barrier.
template <bool LM, bool CTX>
__device__ __forceinline__ void cb_emit(const CbLds<LM, CTX>& sh, const CbBeam<LM, CTX>& g, int nbeam, int n_best, int64_t pad, const CbOut& o,
                                        const int2* __restrict__ nodes) {
  const int tid = threadIdx.x;
  const int64_t Tmax = o.stride;
  int64_t* oi = o.ids;
  for (int64_t idx = tid; idx < (int64_t)n_best * Tmax; idx += CB_THREADS) {
    const int n = (int)(idx / Tmax);
    if (n >= nbeam || idx - n * Tmax >= g.len[LM ? sh.ord[n] : n]) oi[idx] = pad;
  }
  if (tid < n_best) {
    const bool have = tid < nbeam;
    const int from = have && LM ? sh.ord[tid] : tid;  // the beam slot returned in output slot tid
    if constexpr (LM) {
      o.score[tid] = have ? sh.fin[from] : -INFINITY;
      o.ctc[tid] = have ? g.tot[from] : -INFINITY;
      o.lm[tid] = have ? sh.lmf[from] : -INFINITY;
      if constexpr (CTX) o.ctx[tid] = have ? sh.ctx[from] : 0;
    } else {
      o.score[tid] = have ? g.tot[tid] : -INFINITY;
    }
    o.len[tid] = have ? g.len[from] : 0;
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

}  // namespace
