// Live CTC decoding (EXTENSION; the reference decodes finished utterances): js2t_ctc_stream_step, the prefix beam search of
// ctc_beam.hip as a step that stops and resumes, with the causal endpoint rule of the header beside it.  One block per stream; the
// block loads the stream's state (a 64-byte head and the live beam, 2 KB), walks the call's rows under the rule - IDLE rows cost a
// test of one staged flag, SPEECH rows one cb_frame, the very function the one-shot kernel runs - writes a final record wherever a
// segment ends (cb_finish + cb_emit, again the one-shot kernel's), then the partial result and the state.
//
// Why a resumed search has the one-shot search's bits: a frame's result is a function of the live slots of the beam, the frame's
// staged candidates and lp(blank), and the frame's position in the segment (the node index) - cb_frame reads nothing else.  The
// state carries exactly those between calls; the staging buffer is filled per call, from the call's own rows, with the same
// values wherever a chunk boundary falls.  Slots that are not live are stored as zeros, so the state does not depend on what the
// LDS held either: however the rows are cut into calls, the state ends as the same bytes.
//
// The trie lives in the state and is indexed by the position in the segment, so a segment's nodes are overwritten by the next
// one's; a final record is written before the next segment opens.  Nodes written by an earlier launch are read by the back-trace
// of a later one: ordinary global memory, ordered by the stream.
//
// Everything that steers the walk (phase, n, run, the counts) is read from the state or the staged flags by every thread alike:
// block-uniform, so every barrier is met by all 256 threads.
#include "ctc_beam_core.hpp"

namespace {

using CsBeam = CbBeam<true, true>;
constexpr int CS_IDLE = 0, CS_SPEECH = 1;
constexpr int CS_WHY_ENDPOINT = 1, CS_WHY_FORCED = 2, CS_WHY_FLUSHED = 3;
constexpr int CS_BEAM_WORDS = (int)(sizeof(CsBeam) / 4);

struct CsHead {  // the first 64 bytes of a stream's state; all zero = a fresh stream
  int32_t phase, nbeam, n, run;  // IDLE / SPEECH, live beam slots, frames in the segment, trailing silent frames
  int64_t frames, start;         // frames consumed since the reset, first frame of the open segment
  int64_t unused[4];
};
static_assert(sizeof(CsHead) == 64, "the head of a stream's state is 64 bytes");
static_assert(sizeof(CsBeam) == 2048 && offsetof(CsBeam, hash) == 384 && offsetof(CsBeam, len) == 896, "cs_slot_of_word reads this layout");

// the beam slot a 32-bit word of CsBeam belongs to: 32-entry arrays of 4-byte fields, but for hash / phash (8-byte fields)
__device__ __forceinline__ int cs_slot_of_word(int w) { return w >= 96 && w < 224 ? ((w - 96) >> 1) & 31 : w & 31; }

inline int64_t cs_stride(int64_t K, int64_t max_len) {  // bytes of one stream's state, a multiple of 16
  return (int64_t)sizeof(CsHead) + (int64_t)sizeof(CsBeam) + ((1 + K * max_len) * (int64_t)sizeof(int2) + 15) / 16 * 16;
}

struct CsArgs {
  const float *x, *lse;
  const int64_t* argmax;
  const int64_t* cand_id;
  const float* cand_lp;
  const int32_t *rowoff, *flush;
  char* state;
  int64_t stride;
  int64_t* fin_ids;
  int32_t* fin_len;
  float *fin_score, *fin_ctc, *fin_lm;
  int32_t* fin_ctx;
  int64_t* fin_start;
  int32_t *fin_n, *fin_why, *consumed, *n_final;
  int64_t* part_ids;
  int32_t *part_len, *stable_len;
  int64_t* part_start;
  int64_t rows, V, max_len, pad;
  int K, C, n_best, max_finals, blank, min_silence;
  float log_threshold;
};

__global__ __launch_bounds__(CB_THREADS) void ctc_stream_kernel(const CsArgs a, const CbFuse fuse) {
  __shared__ CbLds<true, true> sh;
  __shared__ int s_sil[CB_CHUNK];  // is the staged frame silent?
  const int b = blockIdx.x, tid = threadIdx.x;
  char* st = a.state + (int64_t)b * a.stride;
  CsHead* hd = (CsHead*)st;
  uint32_t* gbeam = (uint32_t*)(st + sizeof(CsHead));
  int2* nodes = (int2*)(st + sizeof(CsHead) + sizeof(CsBeam));  // node 0 = the empty prefix, never written
  // (the clamps: a state that no step wrote must not lead a loop or a node index outside the LDS or the trie)
  int phase = hd->phase == CS_SPEECH ? CS_SPEECH : CS_IDLE, nbeam = min(max(hd->nbeam, 0), a.K);
  int n = hd->n, run = hd->run;
  if (phase == CS_SPEECH) n = (int)min((int64_t)max(n, 0), a.max_len - 1);  // (an open segment has fewer than max_len frames)
  int64_t frames = hd->frames, start = hd->start;
  int cur = 0;
  for (int w = tid; w < CS_BEAM_WORDS; w += CB_THREADS) ((uint32_t*)&sh.beam[0])[w] = gbeam[w];
  const int64_t r0 = min(max((int64_t)a.rowoff[b], (int64_t)0), a.rows);
  const int64_t r1 = min(max((int64_t)a.rowoff[b + 1], r0), a.rows);
  const int64_t nrows = r1 - r0;
  const int K = a.K, C = a.C;
  int64_t consumed = 0;
  int nfin = 0;
  __syncthreads();

  // a segment ends: the one-shot kernel's epilogue and back-trace into record slot (b, nfin); a barrier behind it, so that the
  // next segment's root does not overtake the readers of this beam
  auto finalize = [&](int why) {
    const CsBeam& g = sh.beam[cur];
    cb_finish(sh, g, nbeam, fuse);
    const int64_t rec = (int64_t)b * a.max_finals + nfin, at = rec * a.n_best;
    const CbOut o{a.fin_ids + at * a.max_len, a.max_len, a.fin_len + at, a.fin_score + at, a.fin_ctc + at, a.fin_lm + at, a.fin_ctx + at};
    cb_emit(sh, g, nbeam, a.n_best, a.pad, o, nodes);
    if (tid == 0) a.fin_start[rec] = start, a.fin_n[rec] = n, a.fin_why[rec] = why;
    phase = CS_IDLE, ++nfin;
    __syncthreads();
  };

  bool full = false;
  for (int64_t c0 = 0; c0 < nrows && !full; c0 += CB_CHUNK) {  // (block-uniform bounds: nrows, full)
    const int nt = (int)min((int64_t)CB_CHUNK, nrows - c0);
    cb_stage<float>(sh, a.x, a.lse, a.cand_id, a.cand_lp, r0 + c0, nt, a.V, C, a.blank);
    for (int tt = tid; tt < nt; tt += CB_THREADS) {  // (the thread that staged lpb[tt] reads it back)
      const int64_t r = r0 + c0 + tt;
      s_sil[tt] = a.argmax[r] == (int64_t)a.blank && sh.lpb[tt] >= a.log_threshold ? 1 : 0;  // a NaN is not silent
    }
    __syncthreads();
    for (int tt = 0; tt < nt; ++tt) {  // (block-uniform bounds and branches)
      if (nfin == a.max_finals) {  // no slot for a further record: the caller sends the rest again
        full = true;
        break;
      }
      const int sil = s_sil[tt];
      ++consumed;
      const int64_t t = frames++;
      if (phase == CS_IDLE) {
        if (sil) continue;
        phase = CS_SPEECH, start = t, n = 0, run = 0, nbeam = 1;
        if (tid == 0) cb_root(sh.beam[cur]);
        __syncthreads();
      }
      nbeam = cb_frame(sh, cur, nbeam, tt, n, K, C, nodes, fuse);
      cur ^= 1;
      ++n;
      run = sil ? run + 1 : 0;
      if (a.min_silence > 0 && run == a.min_silence)
        finalize(CS_WHY_ENDPOINT);
      else if (n == a.max_len)
        finalize(CS_WHY_FORCED);
    }
    __syncthreads();  // the staged rows are read by everyone up to here
  }
  if (consumed == nrows && phase == CS_SPEECH && a.flush && a.flush[b] != 0) finalize(CS_WHY_FLUSHED);

  // ---- the partial result: slot 0's labels, and the longest common prefix of all live slots, by one wave walking the trie.  Lane i
  // first climbs from its slot's node to depth L = the shortest live length, then the lanes climb together and compare tokens.
  const CsBeam& g = sh.beam[cur];
  if (tid < 64) {  // (wave-uniform)
    const bool speech = phase == CS_SPEECH;
    const int live = speech ? nbeam : 0;
    const bool have = tid < live;
    const int most = speech ? n : 0;  // a prefix of n frames has at most n labels, and n <= max_len
    int L = live > 0 ? min(max(g.len[0], 0), most) : 0;
    for (int i = 1; i < live; ++i) L = min(L, max(g.len[i], 0));
    int len = have ? min(g.len[tid], most) : L, node = have ? g.node[tid] : 0;
    int64_t* pi = a.part_ids + (int64_t)b * a.max_len;
    for (int p = len; p > L; --p) {  // (a slot's length is at most n <= max_len: inside part_ids and the trie)
      const int2 nd = nodes[node];
      if (tid == 0) pi[p - 1] = nd.y;
      node = nd.x;
    }
    int stable = L;
    for (int p = L; p >= 1; --p) {  // (wave-uniform bounds)
      int2 nd = make_int2(0, 0);
      if (have) nd = nodes[node];
      const int tok0 = __shfl(nd.y, 0);
      if (!__all(!have || nd.y == tok0)) stable = p - 1;
      if (tid == 0) pi[p - 1] = nd.y;
      node = nd.x;
    }
    if (tid == 0) {
      a.part_len[b] = live > 0 ? min(max(g.len[0], 0), most) : 0;
      a.stable_len[b] = stable;
      a.part_start[b] = speech ? start : -1;
      a.consumed[b] = (int32_t)consumed, a.n_final[b] = nfin;
      hd->phase = phase, hd->nbeam = nbeam, hd->n = n, hd->run = run;
      hd->frames = frames, hd->start = start;
    }
  }
  // ---- the state: the beam as it stands (after a final: that segment's last beam), slots that are not live as zeros
  for (int w = tid; w < CS_BEAM_WORDS; w += CB_THREADS) gbeam[w] = cs_slot_of_word(w) < nbeam ? ((const uint32_t*)&g)[w] : 0u;
}

}  // namespace

extern "C" int64_t js2t_ctc_stream_state_bytes(int64_t B, int32_t beam, int64_t max_len) {
  if (B <= 0 || beam <= 0 || beam > CB_MAX_K || max_len <= 0 || max_len >= (int64_t(1) << 31) / CB_MAX_K) return 0;
  return B * cs_stride(beam, max_len);
}

extern "C" int js2t_ctc_stream_step(const float* logits, const float* lse, const int64_t* argmax, const int64_t* cand_id,
                                    const float* cand_lp, const int32_t* row_offsets, const int32_t* flush, const float* uni,
                                    const void* table, int64_t capacity, int32_t max_probe, int32_t lm_order, const void* ctx_nodes,
                                    const void* ctx_edges, int64_t ctx_capacity, int32_t ctx_max_probe, int32_t ctx_n_nodes,
                                    int32_t ctx_max_fail, void* state, int64_t* fin_ids, int32_t* fin_len, float* fin_score, float* fin_ctc,
                                    float* fin_lm, int32_t* fin_ctx, int64_t* fin_start, int32_t* fin_n, int32_t* fin_why, int32_t* consumed,
                                    int32_t* n_final, int64_t* part_ids, int32_t* part_len, int32_t* stable_len, int64_t* part_start,
                                    int64_t B, int64_t rows, int64_t V, int32_t beam, int32_t n_cand, int32_t n_best, int32_t max_finals,
                                    int64_t max_len, int64_t blank, int64_t pad, int64_t bos, int64_t eos, float lm_weight,
                                    float context_weight, float length_bonus, float log_threshold, int32_t min_silence,
                                    js2t_stream stream) {
  if (B == 0) return JS2T_OK;
  const char* who = "ctc_stream_step";
  JS2T_CHECK(B > 0 && B < (int64_t(1) << 31) && rows >= 0 && rows < (int64_t(1) << 31) && V > 0, "%s: bad shape", who);
  JS2T_CHECK(rows == 0 || (logits && lse && argmax && cand_id && cand_lp), "%s: null pointer (rows)", who);
  JS2T_CHECK(row_offsets && state, "%s: null pointer (row_offsets / state)", who);
  JS2T_CHECK(fin_ids && fin_len && fin_score && fin_ctc && fin_lm && fin_ctx && fin_start && fin_n && fin_why && consumed && n_final,
             "%s: null pointer (final records)", who);
  JS2T_CHECK(part_ids && part_len && stable_len && part_start, "%s: null pointer (partial result)", who);
  JS2T_CHECK(((uintptr_t)state & 15) == 0, "%s: state not 16-byte aligned", who);
  JS2T_CHECK(beam >= 1 && beam <= CB_MAX_K, "%s: beam %d outside 1..%d", who, (int)beam, CB_MAX_K);
  JS2T_CHECK(n_cand >= 1 && n_cand <= CB_MAX_C, "%s: %d candidates outside 1..%d", who, (int)n_cand, CB_MAX_C);
  JS2T_CHECK(n_best >= 1 && n_best <= beam, "%s: n_best %d outside 1..beam (%d)", who, (int)n_best, (int)beam);
  JS2T_CHECK(max_len >= 1 && max_len < (int64_t(1) << 31) / CB_MAX_K, "%s: max_len %lld outside 1..: the node index", who, (long long)max_len);
  JS2T_CHECK(max_finals >= 1, "%s: max_finals %d below 1", who, (int)max_finals);
  JS2T_CHECK(min_silence >= 0, "%s: min_silence %d below 0", who, (int)min_silence);
  JS2T_CHECK(log_threshold == log_threshold, "%s: log_threshold is NaN", who);
  JS2T_CHECK(blank >= 0 && blank < V, "%s: blank %lld outside the vocabulary", who, (long long)blank);
  CbFuse fuse{};
  if (const int rc = ngram_args(who, uni, table, capacity, max_probe, lm_order, V, bos, eos, lm_weight, length_bonus, &fuse.lm)) return rc;
  if (const int rc = context_args(who, ctx_nodes, ctx_edges, ctx_capacity, ctx_max_probe, ctx_n_nodes, ctx_max_fail, V, context_weight, &fuse.ctx))
    return rc;
  fuse.bos = (int)bos, fuse.eos = (int)eos, fuse.lm_weight = lm_weight, fuse.length_bonus = length_bonus, fuse.ctx_weight = context_weight;
  CsArgs a{};
  a.x = logits, a.lse = lse, a.argmax = argmax, a.cand_id = cand_id, a.cand_lp = cand_lp, a.rowoff = row_offsets, a.flush = flush;
  a.state = (char*)state, a.stride = cs_stride(beam, max_len);
  a.fin_ids = fin_ids, a.fin_len = fin_len, a.fin_score = fin_score, a.fin_ctc = fin_ctc, a.fin_lm = fin_lm, a.fin_ctx = fin_ctx;
  a.fin_start = fin_start, a.fin_n = fin_n, a.fin_why = fin_why, a.consumed = consumed, a.n_final = n_final;
  a.part_ids = part_ids, a.part_len = part_len, a.stable_len = stable_len, a.part_start = part_start;
  a.rows = rows, a.V = V, a.max_len = max_len, a.pad = pad;
  a.K = (int)beam, a.C = (int)n_cand, a.n_best = (int)n_best, a.max_finals = (int)max_finals, a.blank = (int)blank;
  a.min_silence = (int)min_silence, a.log_threshold = log_threshold;
  hipLaunchKernelGGL(ctc_stream_kernel, dim3((unsigned)B), dim3(CB_THREADS), 0, (hipStream_t)stream, a, fuse);
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}
