"""js2t_ctc_beam_search_ctx at the LS100 shape of tools/ctc_beam_bench.py (B = 32, T' = 375, V = 5000 f32 logits with a planted
labelling, beam 10, 8 candidates) with a graph of about 1000 phrases of 2 to 6 tokens - half of them cut from the planted labellings,
so that matches, failing matches and fail links all occur - and the synthetic order-4 LM of tools/ctc_beam_lm_bench.py: in one
process, on the same logits and candidate tables, the biased launch with and without the LM and with context_weight 0, against
js2t_ctc_beam_search and js2t_ctc_beam_search_lm; and js2t_context_rescore of the 320 hypotheses of the list.  C entry points with
pre-allocated outputs (no allocator in the timed window), alternating rounds, device events; prints the median of the rounds for
each and the cost per frame (the time over the T' frames of the longest utterance).
Two rows take the context step apart (their RESULTS are those of another graph): ctx_max_probe 1 with ctx_max_fail 1 stops every
walk at its first probe, and a graph of one phrase that never occurs leaves the first probe of every extension and nothing else.
The biased result is checked against js2t_context_rescore of its own labellings with base = out_ctc.
usage: python tools/ctc_beam_ctx_bench.py [--beam K] [--cand C] [--rounds N] [--reps N] [--ngrams N] [--phrases N]"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from joeys2t_amd import ops  # noqa: E402
from joeys2t_amd._lib import check, lib  # noqa: E402
from joeys2t_amd.biasing import ContextGraph  # noqa: E402
from joeys2t_amd.lm import NGramLM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--beam", type=int, default=10)
ap.add_argument("--cand", type=int, default=8)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--ngrams", type=int, default=2_000_000)
ap.add_argument("--phrases", type=int, default=1000)
args = ap.parse_args()

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(7)
rs = np.random.RandomState(11)
B, T, V, blank, pad, bos, eos = 32, 375, 5000, 2, 1, 2, 3
K, NC = args.beam, args.cand
LMW, BONUS, CW = 0.5, 0.2, 1.0
in_len = torch.cat([torch.tensor([T]), torch.randint(250, T + 1, (B - 1, ), generator=g)])
planted = torch.full((B, T), blank, dtype=torch.int64)
planted[:, ::4] = torch.randint(4, V, (B, (T + 3) // 4), generator=g)
logits = torch.randn(B, T, V, generator=g)
logits.scatter_add_(2, planted.unsqueeze(-1), torch.full((B, T, 1), 14.0))
rows = B * T
labels = [planted[b, :int(in_len[b])][planted[b, :int(in_len[b])] != blank].numpy() for b in range(B)]

# ------------------------------------------------------------------ the LM (tools/ctc_beam_lm_bench.py's) and the graph
uni = np.stack([-rs.uniform(2.0, 9.0, size=V), -rs.uniform(0.0, 1.0, size=V)], axis=1).astype(np.float32)
share = {2: 0.5, 3: 0.35, 4: 0.15}
grams = {}
for k in (2, 3, 4):
    own = np.concatenate([np.lib.stride_tricks.sliding_window_view(np.concatenate([[bos], y, [eos]]), k) for y in labels])
    own = own[rs.uniform(size=len(own)) < 0.7]
    gk = np.unique(np.concatenate([own, rs.randint(0, V, size=(int(args.ngrams * share[k]), k))]), axis=0)
    grams[k] = (gk, -rs.uniform(0.5, 6.0, size=len(gk)), -rs.uniform(0.0, 1.0, size=len(gk)))
lm = NGramLM.from_arrays(uni, grams, max_load=0.5).to(dev)
phrases = []
for i in range(args.phrases):
    L = int(rs.randint(2, 7))
    if i % 2 == 0:  # cut from a planted labelling: it occurs
        y = labels[rs.randint(B)]
        s = int(rs.randint(0, len(y) - L + 1))
        phrases.append(tuple(int(v) for v in y[s:s + L]))
    else:           # random, with the first token of a planted label half of the time: a match that starts and fails
        y = labels[rs.randint(B)]
        head = [int(y[rs.randint(len(y))])] if rs.rand() < 0.5 else []
        phrases.append(tuple(head + [int(v) for v in rs.randint(4, V, size=L - len(head))]))
graph = ContextGraph.from_phrases(phrases, V, device=dev)
never = ContextGraph.from_phrases([(0, 1)], V, device=dev)  # ids below 4 are never planted: the first probe of every extension misses
print(f"LM: order {lm.order}, {lm.n_entries} n-grams, capacity {lm.capacity} = {lm.capacity * 16 / 2**20:.0f} MiB, max_probe {lm.max_probe}; graph: "
      f"{graph.n_phrases} phrases, {graph.n_nodes} nodes, capacity {graph.capacity} = {graph.capacity * 16 / 2**10:.0f} KiB, max_probe "
      f"{graph.max_probe}, max_fail {graph.max_fail}", flush=True)
logits, in_len = logits.to(dev), in_len.to(dev)

# ------------------------------------------------------------------ the routes
p, st, i64, i32, f32 = ops._p, ops._stream, C.c_int64, C.c_int32, C.c_float
zeros = torch.zeros((rows, ), device=dev)
cand_lp, cand_id = torch.empty((rows, NC), device=dev), torch.empty((rows, NC), dtype=torch.int64, device=dev)
lse = torch.empty((rows, ), device=dev)
forbid = (C.c_int32 * 1)(blank)
ws = torch.empty((ops.ctc_beam_workspace_bytes(B, T, K), ), dtype=torch.uint8, device=dev)
o_ids, o_n = torch.empty((B, K, T), dtype=torch.int64, device=dev), torch.empty((B, K), dtype=torch.int32, device=dev)
o_score, o_ctc, o_lm = (torch.empty((B, K), device=dev) for _ in range(3))
o_ctx = torch.empty((B, K), dtype=torch.int32, device=dev)
r_ctx, r_score, r_order = torch.empty((B * K, ), dtype=torch.int32, device=dev), torch.empty((B * K, ), device=dev), torch.empty((B, K), dtype=torch.int32, device=dev)
check(lib().js2t_beam_pick(p(logits), p(zeros), p(cand_lp), p(cand_id), p(lse), i64(rows), i32(NC), i64(V), forbid, 1, st()), "js2t_beam_pick")


def biased(lmw=LMW, bonus=BONUS, cw=CW, gr=graph, max_probe=None, max_fail=None):
    check(lib().js2t_ctc_beam_search_ctx(p(logits), 0, p(lse), p(cand_id), p(cand_lp), p(in_len), p(lm.uni_dev), p(lm.table_dev), i64(lm.capacity),
                                         i32(lm.max_probe), i32(lm.order), p(gr.nodes_dev), p(gr.edges_dev), i64(gr.capacity),
                                         i32(max_probe or gr.max_probe), i32(gr.n_nodes), i32(max_fail or gr.max_fail), p(o_ids), p(o_n),
                                         p(o_score), p(o_ctc), p(o_lm), p(o_ctx), p(ws), i64(B), i64(T), i64(V), i32(K), i32(NC), i32(K),
                                         i64(blank), i64(pad), i64(bos), i64(eos), f32(lmw), f32(cw), f32(bonus), None, st()),
          "js2t_ctc_beam_search_ctx")


def with_lm(lmw=LMW, bonus=BONUS):
    check(lib().js2t_ctc_beam_search_lm(p(logits), 0, p(lse), p(cand_id), p(cand_lp), p(in_len), p(lm.uni_dev), p(lm.table_dev), i64(lm.capacity),
                                        i32(lm.max_probe), i32(lm.order), p(o_ids), p(o_n), p(o_score), p(o_ctc), p(o_lm), p(ws), i64(B), i64(T),
                                        i64(V), i32(K), i32(NC), i32(K), i64(blank), i64(pad), i64(bos), i64(eos), f32(lmw), f32(bonus), None, st()),
          "js2t_ctc_beam_search_lm")


def plain():
    check(lib().js2t_ctc_beam_search(p(logits), 0, p(lse), p(cand_id), p(cand_lp), p(in_len), p(o_ids), p(o_n), p(o_score), p(ws), i64(B), i64(T),
                                     i64(V), i32(K), i32(NC), i32(K), i64(blank), i64(pad), None, st()), "js2t_ctc_beam_search")


def rescore():
    check(lib().js2t_context_rescore(p(o_ids), i64(T), p(o_n), p(o_ctc), p(graph.nodes_dev), p(graph.edges_dev), i64(graph.capacity),
                                     i32(graph.max_probe), i32(graph.n_nodes), i32(graph.max_fail), p(r_ctx), p(r_score), p(r_order), i64(B), i32(K),
                                     i64(T + 1), i64(V), f32(CW), st()), "js2t_context_rescore")


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


# the biased result is what js2t_context_rescore gives its own labellings with base = out_ctc (no LM: the same two roundings, bit for bit)
biased(0.0, 0.0)
rescore()
torch.cuda.synchronize()
live = torch.isfinite(o_score.view(-1))
assert torch.equal(o_ctx.view(-1), r_ctx) and torch.equal(o_score.view(-1)[live], r_score[live]) and bool(live.view(B, K)[:, 0].all())
matched = float(o_ctx[:, 0].float().mean())
kept = [o_ids[b, 0, :int(o_n[b, 0])].tolist() for b in range(B)]
plain()
torch.cuda.synchronize()
other = sum(kept[b] != o_ids[b, 0, :int(o_n[b, 0])].tolist() for b in range(B))
print(f"B {B} T' {T} (lengths {int(in_len.min())}..{T}) V {V} f32, beam {K}, {NC} candidates, n_best {K}, context_weight {CW}, lm_weight {LMW}, bonus "
      f"{BONUS}; the best hypothesis holds {matched:.1f} matched tokens on average and differs from the unbiased one on {other} of {B} utterances")
biased(0.0, 0.0)  # the list js2t_context_rescore is timed on

work = [("js2t_ctc_beam_search_ctx (LM + graph)", biased), ("  first probes only (ctx max_probe 1, max_fail 1)", lambda: biased(max_probe=1, max_fail=1)),
        ("  a graph of one phrase that never occurs", lambda: biased(gr=never)), ("  context_weight 0 (LM alone)", lambda: biased(cw=0.0)),
        ("js2t_ctc_beam_search_lm", with_lm), ("js2t_ctc_beam_search_ctx, graph alone (LM weights 0)", lambda: biased(0.0, 0.0)),
        ("  graph alone, first probes only", lambda: biased(0.0, 0.0, max_probe=1, max_fail=1)),
        ("js2t_ctc_beam_search_ctx, all weights 0", lambda: biased(0.0, 0.0, 0.0)), ("js2t_ctc_beam_search_lm, both weights 0", lambda: with_lm(0.0, 0.0)),
        ("js2t_ctc_beam_search", plain)]
for _, fn in work:
    timed(fn, 3)
times = {name: [] for name, _ in work}
for _ in range(args.rounds):
    for name, fn in work:
        times[name].append(timed(fn, args.reps))
biased(0.0, 0.0)
torch.cuda.synchronize()
rs_times = [timed(rescore, args.reps * 5) for _ in range(args.rounds)]
for name, _ in work:
    v = times[name]
    med = statistics.median(v)
    print(f"{name:54s} {med:9.1f} us = {med / T:6.2f} us per frame  (min {min(v):.1f}, max {max(v):.1f} over {args.rounds} rounds of {args.reps})")
print(f"{'js2t_context_rescore, ' + str(B * K) + ' hypotheses':54s} {statistics.median(rs_times):9.1f} us  (min {min(rs_times):.1f}, max {max(rs_times):.1f})")
