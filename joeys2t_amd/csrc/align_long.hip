// CTC forced alignment of a whole RECORDING (EXTENSION): js2t_ctc_align's recursion, emission rule and tie rule (align.hip) for a
// state count that one block's LDS does not bound, and optionally free ends.  Three kinds of launch on ONE stream, nothing else
// orders them - no block ever waits for another block:
//   1. forward, one launch per anti-diagonal of (time tile of ALL_TT frames, block column of ALL_SB states).  A lane owns ALL_KL
//      consecutive states in registers; its left neighbour's last two values come by a DPP wave shift.  The four waves of a block
//      are skewed in time: in phase p wave j works on sub-tile p - j (ALL_F frames) and reads the two edge values of every frame
//      of it that wave j - 1 left in LDS in phase p - 1 - one __syncthreads() per phase, none per frame.  One level up the same:
//      block (k, c) reads the edge column that block (k, c - 1) wrote to the workspace one launch earlier, and the state row
//      that block (k - 1, c) left there.  Emissions of the next ALL_G frames are in flight while a group is computed.
//   2. back-trace, one block: chunks of ALL_BT frames; the path moves at most 2 states per frame, so a chunk needs a window of
//      2 ALL_BT + 1 states of the bit matrix - staged in LDS by all threads, walked there by thread 0 (align.hip's opening
//      comment: a dependent GLOBAL read per frame is what this avoids).
//   3. outputs, parallel over t: frame_logp and the spans from the path.
// Back-pointers (2 bits, align.hip's codes) as dword [t >> 4][s >> 2][(t >> 2) & 3]: byte t & 3, bits 2 (s & 3) of it - the lane
// that owns states 4 q .. 4 q + 3 stores the four dwords of sixteen frames as one 16-byte store.  Every dword the back-trace can
// read is written whole by the forward launches, and nothing in the workspace is read before this call wrote it.
#include "common.hpp"

namespace {

constexpr int ALL_THREADS = 256;
constexpr int ALL_WAVES = ALL_THREADS / 64;
constexpr int ALL_KL = 4;                    // states per lane
constexpr int ALL_WS = 64 * ALL_KL;          // states per wave
constexpr int ALL_SB = ALL_WAVES * ALL_WS;   // states per block column
constexpr int ALL_G = 8;                     // frames per prefetch group
constexpr int ALL_F = 32;                    // frames per sub-tile: what a wave does between two block barriers
constexpr int ALL_TT = 512;                  // frames per launch tile
constexpr int ALL_BT = 256;                  // frames per back-trace chunk
constexpr int ALL_BQ = 2 * ALL_BT / 4 + 4;   // quads of states in the staged window (2 states per frame, rounding at both ends)
constexpr int64_t ALL_MAX_L = (int64_t(1) << 20) - 1;
static_assert(ALL_F % 16 == 0 && ALL_TT % ALL_F == 0 && ALL_BT % 16 == 0 && ALL_KL == 4, "back-pointer dwords: 16 frames x 4 states per lane");

struct AllPlan {  // host: where things lie in the workspace (bytes), for (T, L)
  int64_t ncol, ntile, spad, rows_off, edge_off, bits_off, bytes;
};
inline AllPlan all_plan(int64_t T, int64_t L) {
  AllPlan p;
  p.ncol = (2 * L + 1 + ALL_SB - 1) / ALL_SB;
  p.ntile = (T + ALL_TT - 1) / ALL_TT;
  p.spad = p.ncol * ALL_SB;
  p.rows_off = 0;                                                    // f32 [ncol][ALL_SB]: v at the end of the column's last tile
  p.edge_off = p.rows_off + p.spad * 4;                              // float2 [ncol][2][ALL_TT]: edge columns, by time-tile parity
  p.bits_off = p.edge_off + p.ncol * 2 * ALL_TT * 8;                 // u32 [(T + 15) >> 4][spad / 4][4]
  p.bytes = p.bits_off + ((T + 15) >> 4) * p.spad * 4;
  return p;
}

// v of the lane to the left (wave shift right by one lane); lane 0 takes `edge`
__device__ __forceinline__ float all_from_left(float v, float edge) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138, 0xf, 0xf, false));  // wave_shr:1
}

struct AllGroup {  // what ALL_G frames need from memory: the two gathered logits, lse, the blank's logit, the edge from the left column
  float g1[ALL_G], g3[ALL_G], lse[ALL_G], bl[ALL_G], ex[ALL_G], ey[ALL_G];
};

template <typename T>
__global__ __launch_bounds__(ALL_THREADS) void ctc_align_long_fwd_kernel(
    const T* __restrict__ x, const float* __restrict__ lse, const int64_t* __restrict__ targets, float* __restrict__ rows,
    float2* __restrict__ edges, uint4* __restrict__ bits, int64_t Tn, int64_t V, int S, int64_t blank, int free_start, int free_end,
    int diag, int col_lo, int64_t spad4) {
  __shared__ float2 edge_lds[ALL_WAVES][2][ALL_F];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = col_lo + (int)blockIdx.x, k = diag - c;
  const int64_t t0 = (int64_t)k * ALL_TT;
  const int nfr = (int)min((int64_t)ALL_TT, Tn - t0);  // frames of this tile, >= 1
  const int ngroups = (nfr + ALL_G - 1) / ALL_G, nsub = (nfr + ALL_F - 1) / ALL_F;
  const int s0 = c * ALL_SB + w * ALL_WS + lane * ALL_KL;  // the lane's states s0 .. s0 + 3; s0 is even: s0 + 1, s0 + 3 are labels

  // emissions: even states share lp_t(blank) unless past S (-inf) or freed (0); odd ones gather their label's column
  const bool blank_ok = blank >= 0 && blank < V;
  const int64_t bcol = blank_ok ? blank : 0;
  const int64_t l1 = s0 + 1 < S ? targets[(s0 + 1) >> 1] : -1, l3 = s0 + 3 < S ? targets[(s0 + 3) >> 1] : -1;
  const bool v1 = l1 >= 0 && l1 < V, v3 = l3 >= 0 && l3 < V;
  const int64_t col1 = v1 ? l1 : 0, col3 = v3 ? l3 : 0;
  auto even_const = [&](int s, bool& is_const) {
    is_const = s >= S || (s == 0 && free_start) || (s == S - 1 && free_end);
    return s >= S ? -INFINITY : 0.f;
  };
  bool m0, m2;
  const float c0 = even_const(s0, m0), c2 = even_const(s0 + 2, m2);
  // the skip over a blank: label states only (ctc_recursion_body's condition); the label two states back may be another lane's
  bool sk1 = false, sk3 = false;
  if (s0 + 1 < S && s0 + 1 >= 2) sk1 = l1 != blank && l1 != targets[(s0 - 1) >> 1];
  if (s0 + 3 < S) sk3 = l3 != blank && l3 != l1;

  // v of the frame before this tile: the column's row in the workspace, or (first tile) -0.0f in state 0 and -inf elsewhere -
  // -0.0f + e = e for every e, so frame 0 comes out as v_0(s) = lp_0(s) for s < 2 without a branch of its own
  float a0, a1, a2, a3;
  if (k == 0) {
    a0 = s0 == 0 ? -0.f : -INFINITY;
    a1 = a2 = a3 = -INFINITY;
  } else {
    const float4 r = *(const float4*)(rows + s0);
    a0 = r.x, a1 = r.y, a2 = r.z, a3 = r.w;
  }
  const float2* gedge_in = (w == 0 && c > 0) ? edges + ((int64_t)(c - 1) * 2 + (k & 1)) * ALL_TT : nullptr;
  float2* gedge_out = (w == ALL_WAVES - 1 && (c + 1) * ALL_SB < S) ? edges + ((int64_t)c * 2 + (k & 1)) * ALL_TT : nullptr;

  auto load_group = [&](int gi) {
    AllGroup g;
#pragma unroll
    for (int i = 0; i < ALL_G; ++i) {
      const int tt = gi * ALL_G + i;                       // < ALL_TT
      const int64_t t = t0 + min(tt, nfr - 1);             // (frames behind the tile's end: loaded in bounds, never used)
      const T* row = x + t * V;
      g.g1[i] = io<T>::ld(row + col1);
      g.g3[i] = io<T>::ld(row + col3);
      g.bl[i] = io<T>::ld(row + bcol);
      g.lse[i] = lse[t];
      float2 e = make_float2(-INFINITY, -INFINITY);
      if (gedge_in) e = gedge_in[tt];
      g.ex[i] = e.x, g.ey[i] = e.y;
    }
    return g;
  };

  uint32_t bw[4] = {0u, 0u, 0u, 0u};
  AllGroup cur = load_group(0);
  const int nphase = nsub + ALL_WAVES - 1;
  for (int p = 0; p < nphase; ++p) {
    const int q = p - w;  // (wave-uniform)
    if (q >= 0 && q < nsub) {
      const float2* ledge_in = w > 0 ? edge_lds[w - 1][(p - 1) & 1] : nullptr;
      float2* ledge_out = w < ALL_WAVES - 1 ? edge_lds[w][p & 1] : nullptr;
#pragma unroll 1
      for (int m = 0; m < ALL_F / 16; ++m) {
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          const int gi = q * (ALL_F / ALL_G) + m * 2 + hh;
          if (gi < ngroups) {
            AllGroup nxt = cur;
            if (gi + 1 < ngroups) nxt = load_group(gi + 1);
            if (ledge_in) {
#pragma unroll
              for (int i = 0; i < ALL_G; ++i) {
                const float2 e = ledge_in[(m * 2 + hh) * ALL_G + i];
                cur.ex[i] = e.x, cur.ey[i] = e.y;
              }
            }
#pragma unroll
            for (int i = 0; i < ALL_G; ++i) {
              const int tt = gi * ALL_G + i;
              if (tt < nfr) {
                if (lane == 63) {  // the next wave's / column's view of this frame: v_{t-1} of this lane's last two states
                  if (ledge_out) ledge_out[(m * 2 + hh) * ALL_G + i] = make_float2(a2, a3);
                  if (gedge_out) gedge_out[tt] = make_float2(a2, a3);
                }
                const float p1 = all_from_left(a2, cur.ex[i]), p2 = all_from_left(a3, cur.ey[i]);  // states s0 - 2, s0 - 1
                const float eb = blank_ok ? cur.bl[i] - cur.lse[i] : -INFINITY;
                const float e0 = m0 ? c0 : eb, e2 = m2 ? c2 : eb;
                const float e1 = v1 ? cur.g1[i] - cur.lse[i] : -INFINITY, e3 = v3 ? cur.g3[i] - cur.lse[i] : -INFINITY;
                // a predecessor replaces the best so far only if STRICTLY greater, in the order stay, s-1, s-2
                float b0 = a0, b1 = a1, b2 = a2, b3 = a3;
                uint32_t k0 = 0u, k1 = 0u, k2 = 0u, k3 = 0u;
                if (p2 > b0) { b0 = p2; k0 = 1u; }
                if (a0 > b1) { b1 = a0; k1 = 1u << 2; }
                if (sk1 && p2 > b1) { b1 = p2; k1 = 2u << 2; }
                if (a1 > b2) { b2 = a1; k2 = 1u << 4; }
                if (a2 > b3) { b3 = a2; k3 = 1u << 6; }
                if (sk3 && a1 > b3) { b3 = a1; k3 = 2u << 6; }
                a0 = b0 + e0, a1 = b1 + e1, a2 = b2 + e2, a3 = b3 + e3;
                bw[hh * 2 + (i >> 2)] |= (k0 | k1 | k2 | k3) << (8 * (i & 3));
              }
            }
            if (hh == 1 || gi == ngroups - 1) {
              const int64_t g16 = (t0 + (int64_t)gi * ALL_G) >> 4;
              bits[g16 * spad4 + (s0 >> 2)] = make_uint4(bw[0], bw[1], bw[2], bw[3]);
              bw[0] = bw[1] = bw[2] = bw[3] = 0u;
            }
            cur = nxt;
          }
        }
      }
    }
    __syncthreads();
  }
  *(float4*)(rows + s0) = make_float4(a0, a1, a2, a3);
}

// one block: final state by the tie rule, then the walk, a chunk of ALL_BT frames at a time through LDS
__global__ __launch_bounds__(ALL_THREADS) void ctc_align_long_back_kernel(const float* __restrict__ rows, const uint4* __restrict__ bits,
                                                                          int32_t* __restrict__ path, float* __restrict__ score, int64_t Tn,
                                                                          int S, int64_t spad4) {
  __shared__ uint4 win[ALL_BT / 16][ALL_BQ];
  __shared__ int s_cur;
  const int tid = threadIdx.x;
  if (tid == 0) {
    int s = -1;
    float sc = -INFINITY;
    if (Tn > 0) {
      s = S - 1;
      if (S > 1 && rows[S - 2] > rows[S - 1]) s = S - 2;
      sc = rows[s];
    }
    const bool ok = sc > -INFINITY;  // (not NaN either)
    score[0] = ok ? sc : -INFINITY;
    s_cur = ok ? s : -1;
  }
  __syncthreads();
  if (s_cur < 0) return;  // (block-uniform) no path: the outputs launch fills path / spans / frame_logp
  const int64_t nchunk = (Tn + ALL_BT - 1) / ALL_BT;
  for (int64_t ch = nchunk - 1; ch >= 0; --ch) {
    const int64_t tlo = ch * ALL_BT, thi = min(Tn, tlo + ALL_BT) - 1;
    const int s_hi = s_cur;
    // the states the walk can be in at frames thi .. tlo - 1 (it leaves the chunk in the last of them): q_hi - q_lo + 1 <= ALL_BQ
    const int q_hi = s_hi >> 2, q_lo = max(0, (s_hi - 2 * (int)(thi - tlo + 1)) >> 2);
    const int nq = q_hi - q_lo + 1, ng = (int)((thi >> 4) - (tlo >> 4)) + 1;
    const int64_t g0 = tlo >> 4;
    for (int i = tid; i < ng * nq; i += ALL_THREADS) {
      const int g = i / nq, qq = i - g * nq;
      win[g][qq] = bits[(g0 + g) * spad4 + q_lo + qq];
    }
    __syncthreads();
    if (tid == 0) {
      const uint32_t* wd = (const uint32_t*)win;
      int s = s_hi;
      for (int64_t t = thi; t >= tlo; --t) {
        path[t] = s;
        if (t > 0) {
          const uint32_t word = wd[(((int)(t >> 4) - (int)g0) * ALL_BQ + ((s >> 2) - q_lo)) * 4 + (int)((t >> 2) & 3)];
          s = max(s - (int)((word >> (8 * (int)(t & 3) + 2 * (s & 3))) & 3u), q_lo * 4);
        }
      }
      s_cur = s;
    }
    __syncthreads();
  }
}

// parallel over t and l: frame log-probabilities and spans from the path; the fill values where there is no path
template <typename T>
__global__ __launch_bounds__(ALL_THREADS) void ctc_align_long_out_kernel(const T* __restrict__ x, const float* __restrict__ lse,
                                                                         const int64_t* __restrict__ targets, int32_t* __restrict__ path,
                                                                         int32_t* __restrict__ ts, int32_t* __restrict__ te,
                                                                         float* __restrict__ fl, const float* __restrict__ score, int64_t Tn,
                                                                         int64_t V, int64_t L, int64_t blank, int free_start, int free_end) {
  const int64_t t = (int64_t)blockIdx.x * ALL_THREADS + threadIdx.x;
  const bool ok = score[0] > -INFINITY;
  const int S = (int)(2 * L + 1);
  if (t < Tn) {
    if (ok) {
      const int s = path[t];
      const int64_t lab = (s & 1) ? targets[s >> 1] : blank;
      const bool freed = (s == 0 && free_start) || (s == S - 1 && free_end);
      fl[t] = freed ? 0.f : ((lab >= 0 && lab < V) ? io<T>::ld(x + t * V + lab) - lse[t] : -INFINITY);
      if (s & 1) {  // a label state: every one is visited, in one run of frames
        if (t == 0 || path[t - 1] != s) ts[s >> 1] = (int32_t)t;
        if (t == Tn - 1 || path[t + 1] != s) te[s >> 1] = (int32_t)t + 1;
      }
    } else {
      path[t] = -1;
      fl[t] = 0.f;
    }
  }
  if (!ok && t < L) { ts[t] = -1; te[t] = -1; }
}

template <typename T>
int all_launch(hipStream_t st, const AllPlan& p, const void* logits, const float* lse, const int64_t* targets, int32_t* path,
               int32_t* tok_start, int32_t* tok_end, float* frame_logp, float* score, char* ws, int64_t Tn, int64_t V, int64_t L,
               int64_t blank, int free_start, int free_end) {
  float* rows = (float*)(ws + p.rows_off);
  float2* edges = (float2*)(ws + p.edge_off);
  uint4* bits = (uint4*)(ws + p.bits_off);
  const int S = (int)(2 * L + 1);
  for (int64_t d = 0; Tn > 0 && d < p.ntile + p.ncol - 1; ++d) {  // anti-diagonals: block (k, c), k + c = d
    const int64_t c_lo = d - p.ntile + 1 > 0 ? d - p.ntile + 1 : 0, c_hi = d < p.ncol - 1 ? d : p.ncol - 1;
    hipLaunchKernelGGL(ctc_align_long_fwd_kernel<T>, dim3((unsigned)(c_hi - c_lo + 1)), dim3(ALL_THREADS), 0, st, (const T*)logits, lse,
                       targets, rows, edges, bits, Tn, V, S, blank, free_start, free_end, (int)d, (int)c_lo, p.spad / 4);
    JS2T_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ctc_align_long_back_kernel, dim3(1), dim3(ALL_THREADS), 0, st, rows, bits, path, score, Tn, S, p.spad / 4);
  JS2T_LAUNCH_CHECK();
  const int64_t n = Tn > L ? Tn : L;
  if (n > 0) {
    hipLaunchKernelGGL(ctc_align_long_out_kernel<T>, dim3((unsigned)((n + ALL_THREADS - 1) / ALL_THREADS)), dim3(ALL_THREADS), 0, st,
                       (const T*)logits, lse, targets, path, tok_start, tok_end, frame_logp, score, Tn, V, L, blank, free_start, free_end);
    JS2T_LAUNCH_CHECK();
  }
  return JS2T_OK;
}

}  // namespace

extern "C" int64_t js2t_ctc_align_long_workspace_bytes(int64_t T, int64_t L) {
  if (T <= 0 || L < 0 || L > ALL_MAX_L) return 0;
  return all_plan(T, L).bytes;
}

extern "C" void js2t_ctc_align_long_tiles(int32_t* out) {
  out[0] = ALL_KL, out[1] = ALL_WS, out[2] = ALL_SB, out[3] = ALL_TT;
}

extern "C" int js2t_ctc_align_long(const void* logits, int dt, const float* lse, const int64_t* targets, int32_t* path, int32_t* tok_start,
                                   int32_t* tok_end, float* frame_logp, float* score, void* workspace, int64_t T_, int64_t V, int64_t L,
                                   int64_t blank, int free_start, int free_end, js2t_stream stream) {
  JS2T_CHECK(T_ >= 0 && T_ < (int64_t(1) << 31) && V >= 1 && L >= 0, "ctc_align_long: bad shape (T %lld, V %lld, L %lld)", (long long)T_,
             (long long)V, (long long)L);
  JS2T_CHECK(L <= ALL_MAX_L, "ctc_align_long: target length %lld exceeds %lld", (long long)L, (long long)ALL_MAX_L);
  JS2T_CHECK(dt == JS2T_F32 || dt == JS2T_BF16, "bad dtype %d", dt);
  JS2T_CHECK(score && (T_ == 0 || (logits && lse && path && frame_logp)) && (L == 0 || (targets && tok_start && tok_end)),
             "ctc_align_long: null pointer");
  const AllPlan p = all_plan(T_, L);
  JS2T_CHECK(T_ == 0 || workspace, "ctc_align_long: workspace needed (%lld bytes)", (long long)p.bytes);
  JS2T_CHECK(((uintptr_t)workspace & 15) == 0, "ctc_align_long: the workspace must be 16-byte aligned");
  if (dt == JS2T_F32)
    return all_launch<float>((hipStream_t)stream, p, logits, lse, targets, path, tok_start, tok_end, frame_logp, score, (char*)workspace, T_, V,
                             L, blank, free_start != 0, free_end != 0);
  return all_launch<uint16_t>((hipStream_t)stream, p, logits, lse, targets, path, tok_start, tok_end, frame_logp, score, (char*)workspace, T_,
                              V, L, blank, free_start != 0, free_end != 0);
}
