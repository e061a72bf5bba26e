"""js2t_ctc_beam_search_lm at the LS100 shape of tools/ctc_beam_bench.py (B = 32, T' = 375, V = 5000 f32 logits with a planted
labelling, beam 10, 8 candidates) with the synthetic order-4 LM of tools/ngram_bench.py (about 2 M n-grams, a table of 64 MiB): in one
process, on the same logits and candidate tables, the fused launch, the LM-less launch (js2t_ctc_beam_search) and the LM-less launch
followed by js2t_ngram_rescore of its n-best list - the route the fused search replaces.  C entry points with pre-allocated outputs
(no allocator in the timed window), alternating rounds, device events; prints the median of the rounds for each and the cost per
frame (the time over the T' frames of the longest utterance: one block per utterance, the launch lasts as long as its longest chain).
The LM holds the 2-, 3- and 4-grams of the planted labellings (each kept with probability 0.7) plus random n-grams up to the size.
The fused result is checked against js2t_ngram_rescore of its own labellings with base = out_ctc.
usage: python tools/ctc_beam_lm_bench.py [--beam K] [--cand C] [--rounds N] [--reps N] [--ngrams N]"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from joeys2t_amd import ops  # noqa: E402
from joeys2t_amd._lib import check, lib  # noqa: E402
from joeys2t_amd.lm import NGramLM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--beam", type=int, default=10)
ap.add_argument("--cand", type=int, default=8)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--ngrams", type=int, default=2_000_000)
args = ap.parse_args()

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(7)
rs = np.random.RandomState(11)
B, T, V, blank, pad, bos, eos = 32, 375, 5000, 2, 1, 2, 3
K, NC = args.beam, args.cand
LMW, BONUS = 0.5, 0.2
in_len = torch.cat([torch.tensor([T]), torch.randint(250, T + 1, (B - 1, ), generator=g)])
planted = torch.full((B, T), blank, dtype=torch.int64)
planted[:, ::4] = torch.randint(4, V, (B, (T + 3) // 4), generator=g)
logits = torch.randn(B, T, V, generator=g)
logits.scatter_add_(2, planted.unsqueeze(-1), torch.full((B, T, 1), 14.0))
rows = B * T

# ------------------------------------------------------------------ the LM
uni = np.stack([-rs.uniform(2.0, 9.0, size=V), -rs.uniform(0.0, 1.0, size=V)], axis=1).astype(np.float32)
share = {2: 0.5, 3: 0.35, 4: 0.15}
grams = {}
for k in (2, 3, 4):
    own = []
    for b in range(B):
        labels = planted[b, :int(in_len[b])]
        h = np.concatenate([[bos], labels[labels != blank].numpy(), [eos]])
        own.append(np.lib.stride_tricks.sliding_window_view(h, k))
    own = np.concatenate(own)
    own = own[rs.uniform(size=len(own)) < 0.7]
    fill = rs.randint(0, V, size=(int(args.ngrams * share[k]), k))
    gk = np.unique(np.concatenate([own, fill]), axis=0)
    grams[k] = (gk, -rs.uniform(0.5, 6.0, size=len(gk)), -rs.uniform(0.0, 1.0, size=len(gk)))
t0 = time.perf_counter()
lm = NGramLM.from_arrays(uni, grams, max_load=0.5)
print(f"LM: order {lm.order}, V {V}, {lm.n_entries} n-grams in the table, capacity {lm.capacity} = {lm.capacity * 16 / 2**20:.0f} MiB, max_probe "
      f"{lm.max_probe}; built in {time.perf_counter() - t0:.2f} s", flush=True)
lm.to(dev)
logits, in_len = logits.to(dev), in_len.to(dev)

# ------------------------------------------------------------------ the three routes
p, st, i64, i32, f32 = ops._p, ops._stream, C.c_int64, C.c_int32, C.c_float
zeros = torch.zeros((rows, ), device=dev)
cand_lp, cand_id = torch.empty((rows, NC), device=dev), torch.empty((rows, NC), dtype=torch.int64, device=dev)
lse = torch.empty((rows, ), device=dev)
forbid = (C.c_int32 * 1)(blank)
ws = torch.empty((ops.ctc_beam_workspace_bytes(B, T, K), ), dtype=torch.uint8, device=dev)


def outputs(n):
    return (torch.empty((B, K, T), dtype=torch.int64, device=dev), torch.empty((B, K), dtype=torch.int32, device=dev)) + \
        tuple(torch.empty((B, K), device=dev) for _ in range(n))


f_ids, f_n, f_score, f_ctc, f_lm = outputs(3)
c_ids, c_n, c_score = outputs(1)
r_lm, r_score, r_order = torch.empty((B * K, ), device=dev), torch.empty((B * K, ), device=dev), torch.empty((B, K), dtype=torch.int32, device=dev)
check(lib().js2t_beam_pick(p(logits), p(zeros), p(cand_lp), p(cand_id), p(lse), i64(rows), i32(NC), i64(V), forbid, 1, st()), "js2t_beam_pick")


def fused(lmw=LMW, bonus=BONUS, max_probe=None, order=None):
    check(lib().js2t_ctc_beam_search_lm(p(logits), 0, p(lse), p(cand_id), p(cand_lp), p(in_len), p(lm.uni_dev), p(lm.table_dev), i64(lm.capacity),
                                        i32(max_probe or lm.max_probe), i32(order or lm.order), p(f_ids), p(f_n), p(f_score), p(f_ctc), p(f_lm),
                                        p(ws), i64(B), i64(T), i64(V), i32(K), i32(NC), i32(K), i64(blank), i64(pad), i64(bos), i64(eos), f32(lmw),
                                        f32(bonus), None, st()), "js2t_ctc_beam_search_lm")


def plain():
    check(lib().js2t_ctc_beam_search(p(logits), 0, p(lse), p(cand_id), p(cand_lp), p(in_len), p(c_ids), p(c_n), p(c_score), p(ws), i64(B), i64(T),
                                     i64(V), i32(K), i32(NC), i32(K), i64(blank), i64(pad), None, st()), "js2t_ctc_beam_search")


def rescore(ids, n, base):
    check(lib().js2t_ngram_rescore(p(ids), i64(T), p(n), p(base), p(lm.uni_dev), p(lm.table_dev), i64(lm.capacity), i32(lm.max_probe),
                                   i32(lm.order), None, p(r_lm), p(r_score), p(r_order), i64(B), i32(K), i64(T + 1), i64(V), i64(bos), i64(eos),
                                   f32(LMW), f32(BONUS), st()), "js2t_ngram_rescore")


def plain_then_rescore():
    plain()
    rescore(c_ids, c_n, c_score)


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


# two rows that take the LM's cost apart (their RESULTS are those of another model): max_probe 1 stops every lookup at its first probe -
# the one memory latency a frame cannot avoid - and order 1 reads the unigrams alone
work = [("js2t_ctc_beam_search_lm (fused)", fused), ("  first probes only (max_probe 1)", lambda: fused(max_probe=1)),
        ("  unigrams only (order 1)", lambda: fused(order=1)), ("js2t_ctc_beam_search_lm, both weights 0", lambda: fused(0.0, 0.0)),
        ("js2t_ctc_beam_search (no LM)", plain), ("js2t_ctc_beam_search + js2t_ngram_rescore", plain_then_rescore)]
for _, fn in work:
    timed(fn, 3)
times = {name: [] for name, _ in work}
for _ in range(args.rounds):
    for name, fn in work:
        times[name].append(timed(fn, args.reps))

# the fused scores are what js2t_ngram_rescore gives the same labellings with base = out_ctc, and the lists are sorted
fused()
rescore(f_ids, f_n, f_ctc)
torch.cuda.synchronize()
live = torch.isfinite(f_score.view(-1))
err = float(((f_score.view(-1) - r_score).abs() / r_score.abs().clamp(min=1.0))[live].max())
err_lm = float(((f_lm.view(-1) - r_lm).abs() / r_lm.abs().clamp(min=1.0))[live].max())
assert err <= 1e-4 and err_lm <= 1e-4, f"the fused scores and js2t_ngram_rescore of the same labellings disagree: {err}, {err_lm}"
assert bool(live.view(B, K)[:, 0].all()) and bool((f_score[:, :-1] >= f_score[:, 1:]).all())
plain_then_rescore()
torch.cuda.synchronize()
best = r_order[:, 0].to(torch.int64)
route_best = r_score.view(B, K)[torch.arange(B, device=dev), best]
other = sum(f_ids[b, 0, :int(f_n[b, 0])].tolist() != c_ids[b, int(best[b]), :int(c_n[b, int(best[b])])].tolist() for b in range(B))
print(f"B {B} T' {T} (lengths {int(in_len.min())}..{T}) V {V} f32, beam {K}, {NC} candidates, n_best {K}, lm_weight {LMW}, bonus {BONUS}; worst "
      f"relative difference to js2t_ngram_rescore of the fused labellings {err:.2e} (lm {err_lm:.2e}); best hypothesis differs from the rescore "
      f"route's on {other} of {B} utterances, fused best >= route best on {int((f_score[:, 0] >= route_best - 1e-3).sum())}")
for name, _ in work:
    v = times[name]
    med = statistics.median(v)
    print(f"{name:44s} {med:9.1f} us = {med / T:6.2f} us per frame  (min {min(v):.1f}, max {max(v):.1f} over {args.rounds} rounds of {args.reps})")
