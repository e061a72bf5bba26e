"""js2t_ctc_beam_search at the LS100 shape (B = 32, T' = 375, V = 5000 f32 logits with a planted labelling, beam 10, 8 candidates,
n_best 1 and 10): the candidate selection (js2t_beam_pick) and the beam kernel timed separately, with js2t_ctc_align (on the beam's
best hypotheses) and the greedy path (js2t_row_lse with arg-max + js2t_ctc_collapse) as yardsticks in the same process on the same
logits.  C entry points with pre-allocated outputs (no allocator in the timed window), alternating rounds, device events; prints the
median of the rounds for each.  usage: python tools/ctc_beam_bench.py [--beam K] [--cand C] [--rounds N] [--reps N]"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from joeys2t_amd import ops  # noqa: E402
from joeys2t_amd._lib import check, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--beam", type=int, default=10)
ap.add_argument("--cand", type=int, default=8)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(7)
B, T, V, blank, pad = 32, 375, 5000, 2, 1
K, NC = args.beam, args.cand
in_len = torch.cat([torch.tensor([T]), torch.randint(250, T + 1, (B - 1, ), generator=g)])
# a planted frame labelling: a label every fourth frame, blanks between - what a trained CTC head's posteriors look like
planted = torch.full((B, T), blank, dtype=torch.int64)
planted[:, ::4] = torch.randint(4, V, (B, (T + 3) // 4), generator=g)
logits = torch.randn(B, T, V, generator=g)
logits.scatter_add_(2, planted.unsqueeze(-1), torch.full((B, T, 1), 14.0))
logits, in_len = logits.to(dev), in_len.to(dev)
rows = B * T

p, st, i64, i32 = ops._p, ops._stream, C.c_int64, C.c_int32
zeros = torch.zeros((rows, ), device=dev)
cand_lp, cand_id = torch.empty((rows, NC), device=dev), torch.empty((rows, NC), dtype=torch.int64, device=dev)
lse = torch.empty((rows, ), device=dev)
forbid = (C.c_int32 * 1)(blank)
ws = torch.empty((ops.ctc_beam_workspace_bytes(B, T, K), ), dtype=torch.uint8, device=dev)
out = {n: (torch.empty((B, n, T), dtype=torch.int64, device=dev), torch.empty((B, n), dtype=torch.int32, device=dev),
           torch.empty((B, n), device=dev)) for n in sorted({1, K})}
best = torch.empty((rows, ), dtype=torch.int64, device=dev)
lse2 = torch.empty((rows, ), device=dev)
greedy_ids, greedy_n = torch.empty((B, T), dtype=torch.int64, device=dev), torch.empty((B, ), dtype=torch.int64, device=dev)


def pick():
    check(lib().js2t_beam_pick(p(logits), p(zeros), p(cand_lp), p(cand_id), p(lse), i64(rows), i32(NC), i64(V), forbid, 1, st()), "js2t_beam_pick")


def beam(n_best):
    ids, n, score = out[n_best]
    check(lib().js2t_ctc_beam_search(p(logits), 0, p(lse), p(cand_id), p(cand_lp), p(in_len), p(ids), p(n), p(score), p(ws), i64(B), i64(T),
                                     i64(V), i32(K), i32(NC), i32(n_best), i64(blank), i64(pad), None, st()), "js2t_ctc_beam_search")


def greedy():
    check(lib().js2t_row_lse(p(logits), p(lse2), p(best), i64(rows), i64(V), 0, st()), "js2t_row_lse")
    check(lib().js2t_ctc_collapse(p(best), p(in_len), p(greedy_ids), p(greedy_n), i64(B), i64(T), i64(blank), i64(pad), st()), "js2t_ctc_collapse")


pick()
beam(1)
torch.cuda.synchronize()
hyp_n = out[1][1][:, 0].to(torch.int64).contiguous()
Lmax = max(int(hyp_n.max()), 1)
hyp = out[1][0][:, 0, :Lmax].contiguous()
path = torch.empty((B, T), dtype=torch.int32, device=dev)
tok_start, tok_end = torch.empty((B, Lmax), dtype=torch.int32, device=dev), torch.empty((B, Lmax), dtype=torch.int32, device=dev)
frame_logp, al_score = torch.empty((B, T), device=dev), torch.empty((B, ), device=dev)
al_ws = torch.empty((max(ops.ctc_align_workspace_bytes(B, T, Lmax), 1), ), dtype=torch.uint8, device=dev)


def align():
    check(lib().js2t_ctc_align(p(logits), 0, p(lse), p(hyp), p(in_len), p(hyp_n), p(path), p(tok_start), p(tok_end), p(frame_logp), p(al_score),
                               p(al_ws), i64(B), i64(T), i64(V), i64(Lmax), i64(blank), None, st()), "js2t_ctc_align")


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


work = [("js2t_beam_pick (candidates)", pick)] + [(f"js2t_ctc_beam_search n_best {n}", (lambda n=n: beam(n))) for n in sorted(out)] + \
    [("js2t_ctc_align (yardstick)", align), ("row_lse + ctc_collapse (greedy)", greedy)]
for _, fn in work:
    timed(fn, 3)
times = {name: [] for name, _ in work}
for _ in range(args.rounds):
    for name, fn in work:
        times[name].append(timed(fn, args.reps))
# the search found the planted labelling, and the greedy path agrees with it on this input
greedy()
torch.cuda.synchronize()
want = [[int(v) for v in planted[b, :int(in_len[b])].tolist() if v != blank] for b in range(B)]
got = [out[1][0][b, 0, :int(hyp_n[b])].tolist() for b in range(B)]
assert got == want, "the beam's best hypothesis is not the planted labelling"
assert bool(torch.isfinite(out[1][2]).all()) and bool((out[K][2][:, :-1] >= out[K][2][:, 1:]).all())
print(f"B {B} T' {T} (lengths {int(in_len.min())}..{T}) V {V} f32, beam {K}, {NC} candidates, hypotheses of {int(hyp_n.min())}..{Lmax} labels")
for name, _ in work:
    v = times[name]
    print(f"{name:34s} {statistics.median(v):9.1f} us  (min {min(v):.1f}, max {max(v):.1f} over {args.rounds} rounds of {args.reps})")
