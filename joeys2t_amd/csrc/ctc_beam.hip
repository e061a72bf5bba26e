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
//
// The per-frame body (phase A, phase B), the epilogue and the back-trace live in ctc_beam_core.hpp: the resumable step of
// ctc_stream.hip instantiates the same functions, and this kernel is the loop over a whole utterance around them.
#include "ctc_beam_core.hpp"

namespace {

template <typename T, bool LM, bool CTX>
__global__ __launch_bounds__(CB_THREADS) void ctc_beam_kernel(
    const T* __restrict__ x, const float* __restrict__ lse, const int64_t* __restrict__ cand_id, const float* __restrict__ cand_lp,
    const int64_t* __restrict__ in_len, int64_t* __restrict__ out_ids, int32_t* __restrict__ out_len, float* __restrict__ out_score,
    int2* __restrict__ nodes_all, int64_t Tmax, int64_t V, int K, int C, int n_best, int blank, int64_t pad,
    const int32_t* __restrict__ rowoff, const CbFuse fuse) {
  static_assert(LM || !CTX, "the context form is built on the LM form");
  __shared__ CbLds<LM, CTX> sh;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t Tb = max((int64_t)0, min(in_len[b], Tmax));
  const int64_t r0 = rowoff ? (int64_t)rowoff[b] : (int64_t)b * Tmax;  // first logits / lse / candidate row of the utterance
  int2* nodes = nodes_all + (int64_t)b * (1 + (int64_t)K * Tmax);     // (parent node, token); node 0 = the empty prefix, never read
  if (tid == 0) cb_root(sh.beam[0]);
  int cur = 0, nbeam = 1;
  __syncthreads();
  for (int64_t c0 = 0; c0 < Tb; c0 += CB_CHUNK) {  // (block-uniform bounds: Tb)
    const int nt = (int)min((int64_t)CB_CHUNK, Tb - c0);
    cb_stage<T>(sh, x, lse, cand_id, cand_lp, r0 + c0, nt, V, C, blank);  // the candidate rows of this chunk of frames
    __syncthreads();
    for (int tt = 0; tt < nt; ++tt) {  // (block-uniform bounds: nt)
      nbeam = cb_frame(sh, cur, nbeam, tt, (int)(c0 + tt), K, C, nodes, fuse);
      cur ^= 1;
    }
  }
  // the beam is in score order already: its first n_best slots are the result; the barrier that closed the last frame made it, and
  // the nodes (workgroup scope), visible.  LM: the EOS term, the final ranking, and the back-trace in that order
  const CbBeam<LM, CTX>& g = sh.beam[cur];
  cb_finish(sh, g, nbeam, fuse);
  const int64_t at = (int64_t)b * n_best;
  const CbOut o{out_ids + at * Tmax, Tmax, out_len + at, out_score + at, LM ? fuse.out_ctc + at : nullptr, LM ? fuse.out_lm + at : nullptr,
                CTX ? fuse.out_ctx + at : nullptr};
  cb_emit(sh, g, nbeam, n_best, pad, o, nodes);
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
