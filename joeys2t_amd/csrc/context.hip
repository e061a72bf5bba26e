// Contextual-biasing count of an n-best list (EXTENSION; the reference has no hot words): R = B * N hypotheses -> ctx(y) of every
// hypothesis under the phrase automaton, its combination with the last stage's score and the rank of every slot within its
// utterance.  The semantics are stated in the header; the tables and the walk are context.hpp's, the ones the beam kernel uses.
//
// One launch, one wave per utterance: lane k < N walks hypothesis k - the walk is sequential in the labels, a step is a probe or
// two - and the same wave ranks the N slots by nbest.hpp's rule.  A dead slot, and every slot when context_weight is 0, reads
// neither ids nor the graph.
//
// js2t_context_walk_host runs the same walk on the host over host tables: the statement the kernels share, checkable without a
// device.
//
// No atomics, no allocation, no workspace, no host synchronisation: bit-reproducible, capturable.
#include "common.hpp"
#include "nbest.hpp"
#include "context.hpp"

namespace {

__global__ __launch_bounds__(64) void context_rescore_kernel(const int64_t* __restrict__ ids, int64_t ids_stride, const int32_t* __restrict__ n,
                                                             const float* __restrict__ base_score, const context_view g,
                                                             int32_t* __restrict__ ctx, float* __restrict__ score, int32_t* __restrict__ order,
                                                             int N, int64_t Lp, float context_weight) {
  const int k = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * N + k;
  float sc = -INFINITY;
  if (k < N) {
    const int nr = n[r];
    const float bs = base_score[r];
    int count = 0;
    if (!nbest_dead(bs, nr, Lp)) {
      if (context_weight != 0.f) {
        const int64_t* idr = ids + r * ids_stride;
        context_state s{0, 0, 0};
        for (int l = 0; l < nr; ++l) s = context_step(g, s, idr[l]);  // (nr <= Lp - 1: a host-checked bound)
        count = context_final(g, s);
      }
      sc = nbest_fuse_ctx(bs, 0.f, count, 0, 0.f, context_weight, 0.f);
    }
    ctx[r] = count;
    score[r] = sc;
  }
  const int rank = nbest_rank(sc, k, N);  // (every lane of the wave; N is uniform)
  if (k < N) order[(int64_t)blockIdx.x * N + rank] = k;
}

}  // namespace

extern "C" int js2t_context_rescore(const int64_t* ids, int64_t ids_stride, const int32_t* n, const float* base_score, const void* ctx_nodes,
                                    const void* ctx_edges, int64_t ctx_capacity, int32_t ctx_max_probe, int32_t ctx_n_nodes,
                                    int32_t ctx_max_fail, int32_t* ctx, float* score, int32_t* order, int64_t B, int32_t N, int64_t Lp,
                                    int64_t V, float context_weight, js2t_stream stream) {
  if (B == 0) return JS2T_OK;
  JS2T_CHECK(n && base_score && ctx && score && order, "context_rescore: null pointer");
  if (const int rc = nbest_list_args("context_rescore", B, N, Lp, ids_stride, NBEST_SLOTS)) return rc;  // (one wave per utterance: no B * N * Lp grid)
  context_view g;
  if (const int rc = context_args("context_rescore", ctx_nodes, ctx_edges, ctx_capacity, ctx_max_probe, ctx_n_nodes, ctx_max_fail, V,
                                  context_weight, &g))
    return rc;
  JS2T_CHECK(ids || context_weight == 0.f, "context_rescore: null pointer (ids, with context_weight %g)", (double)context_weight);
  hipLaunchKernelGGL(context_rescore_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, ids, ids_stride, n, base_score, g, ctx, score,
                     order, (int)N, Lp, context_weight);
  JS2T_LAUNCH_CHECK();
  return JS2T_OK;
}

extern "C" int js2t_context_walk_host(const int64_t* ids, int64_t n, const void* ctx_nodes, const void* ctx_edges, int64_t ctx_capacity,
                                      int32_t ctx_max_probe, int32_t ctx_n_nodes, int32_t ctx_max_fail, int64_t V, int32_t* out_node,
                                      int32_t* out_bank, int32_t* out_m, int32_t* out_ctx) {
  JS2T_CHECK(n >= 0 && (n == 0 || (ids && out_node && out_bank && out_m && out_ctx)), "context_walk_host: null pointer or n %lld below 0",
             (long long)n);
  context_view g;
  if (const int rc = context_args("context_walk_host", ctx_nodes, ctx_edges, ctx_capacity, ctx_max_probe, ctx_n_nodes, ctx_max_fail, V, 1.f, &g))
    return rc;
  context_state s{0, 0, 0};
  for (int64_t l = 0; l < n; ++l) {
    s = context_step(g, s, ids[l]);
    out_node[l] = s.node, out_bank[l] = s.bank, out_m[l] = s.bank + s.depth, out_ctx[l] = context_final(g, s);
  }
  return JS2T_OK;
}
