"""Long-form CTC at the LS100 shape: a synthetic 10-minute recording - 15000 encoder frames of 40 ms, V = 5000 - as 55 overlapping
windows of 375 frames (15 s, 50 frames kept back on either side), speech stretches of planted labels between pauses.  Timed in one
process on the same data, C entry points with pre-allocated outputs, alternating rounds, device events, medians:
  js2t_ctc_stitch (f32 and bf16 windows) against the torch-op equivalent - index_select of the kept rows, ops.row_lse with arg-max,
  gather of the blank column - with the bytes each moves over its time;
  js2t_ctc_segment;
  js2t_beam_pick over the stream's rows, then js2t_ctc_beam_search over the segments as packed rows against the SAME kernel over the
  same stream as ONE utterance.
The encoder is not part of it: the windows' logits are cut from one planted stream, so the stitch has to give that stream back.
usage: python tools/long_form_bench.py [--rounds N] [--reps N] [--beam K]"""
import argparse
import ctypes as C
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from joeys2t_amd import ops  # noqa: E402
from joeys2t_amd._lib import check, lib  # noqa: E402
from joeys2t_amd.long_form import plan_windows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--beam", type=int, default=10)
args = ap.parse_args()

dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(7)
V, blank, pad, K, NC, sub = 5000, 2, 1, args.beam, 8, 4
plan = plan_windows(60000, 1500, 200, sub)  # 10 min of 10 ms feature frames; windows of 15 s, 2 s of context on either side
T, W, S = plan.rows, len(plan.start), 375
# the stream: stretches of 2 .. 12 s with a label every fourth frame, pauses of 0.4 .. 2 s of confident blanks
planted = torch.full((T, ), blank, dtype=torch.int64)
gen_h = torch.Generator().manual_seed(7)
t = 0
while t < T:
    n = int(torch.randint(50, 301, (1, ), generator=gen_h))
    planted[t:t + n:4] = torch.randint(4, V, (len(range(t, min(t + n, T), 4)), ), generator=gen_h)
    t += n + int(torch.randint(10, 51, (1, ), generator=gen_h))
stream = torch.randn((T, V), generator=g, device=dev)
stream.scatter_add_(1, planted.to(dev).unsqueeze(1), torch.full((T, 1), 14.0, device=dev))
logits = torch.zeros((W, S, V), device=dev)
for w, st0 in enumerate(plan.start):
    n = -(-plan.length[w] // sub)
    logits[w, :n] = stream[st0 // sub:st0 // sub + n]
logits16 = logits.to(torch.bfloat16)
lo, hi, row = (torch.tensor(v, dtype=torch.int32, device=dev) for v in (plan.keep_lo, plan.keep_hi, plan.out_row))
index = torch.cat([torch.arange(w * S + plan.keep_lo[w], w * S + plan.keep_hi[w]) for w in range(W)]).to(dev)

p, st, i64, i32 = ops._p, ops._stream, C.c_int64, C.c_int32
out, lse, am, blp = (torch.empty((T, V), device=dev), torch.empty((T, ), device=dev), torch.empty((T, ), dtype=torch.int64, device=dev),
                     torch.empty((T, ), device=dev))
t_out = torch.empty((T, V), device=dev)


def stitch(x):
    check(lib().js2t_ctc_stitch(p(x), ops.dt_code(x), p(lo), p(hi), p(row), p(out), p(lse), p(am), p(blp), W, S, V, T, blank, st()), "js2t_ctc_stitch")


def torch_route(x):
    if x.dtype == torch.float32:
        torch.index_select(x.view(W * S, V), 0, index, out=t_out)
    else:
        t_out.copy_(x.view(W * S, V).index_select(0, index))
    t_lse, t_am = ops.row_lse(t_out, want_argmax=True)
    return t_lse, t_am, t_out[:, blank] - t_lse


stitch(logits)
torch.cuda.synchronize()
t_lse, t_am, t_blp = torch_route(logits)
assert torch.equal(out, stream) and torch.equal(out, t_out) and torch.equal(lse.view(torch.int32), t_lse.view(torch.int32)) and torch.equal(am, t_am)
assert torch.equal(blp.view(torch.int32), t_blp.view(torch.int32))

# segments
MIN_SIL, MARGIN, MAX_LEN, THR = 8, 3, 375, math.log(0.9)
most = T // MIN_SIL + T // (MAX_LEN // 2 + 1) + 2
n_seg, seg_off, seg_len = torch.empty((1, ), dtype=torch.int32, device=dev), torch.empty((most + 1, ), dtype=torch.int32, device=dev), \
    torch.empty((most, ), dtype=torch.int64, device=dev)
seg_ws = torch.empty((lib().js2t_ctc_segment_workspace_bytes(T), ), dtype=torch.uint8, device=dev)


def segment():
    check(lib().js2t_ctc_segment(p(blp), p(am), T, blank, THR, MIN_SIL, MARGIN, MAX_LEN, most, p(n_seg), p(seg_off), p(seg_len), p(seg_ws), st()),
          "js2t_ctc_segment")


segment()
B = int(n_seg.item())
assert B > 0
seg, in_len = seg_off[:B + 1].contiguous(), seg_len[:B].contiguous()
Tmax = int(in_len.max())

# the beam: candidates once for the stream's rows, then packed segments against one utterance
zeros = torch.zeros((T, ), device=dev)
cand_lp, cand_id, pick_lse = torch.empty((T, NC), device=dev), torch.empty((T, NC), dtype=torch.int64, device=dev), torch.empty((T, ), device=dev)
forbid = (C.c_int32 * 1)(blank)
ws_p = torch.empty((max(ops.ctc_beam_workspace_bytes(B, Tmax, K), 8), ), dtype=torch.uint8, device=dev)
ws_1 = torch.empty((max(ops.ctc_beam_workspace_bytes(1, T, K), 8), ), dtype=torch.uint8, device=dev)
res_p = (torch.empty((B, 1, Tmax), dtype=torch.int64, device=dev), torch.empty((B, 1), dtype=torch.int32, device=dev), torch.empty((B, 1), device=dev))
res_1 = (torch.empty((1, 1, T), dtype=torch.int64, device=dev), torch.empty((1, 1), dtype=torch.int32, device=dev), torch.empty((1, 1), device=dev))
len_1 = torch.tensor([T], dtype=torch.int64, device=dev)


def pick():
    check(lib().js2t_beam_pick(p(out), p(zeros), p(cand_lp), p(cand_id), p(pick_lse), i64(T), i32(NC), i64(V), forbid, 1, st()), "js2t_beam_pick")


def beam(packed):
    (ids, n, score), ws = (res_p, ws_p) if packed else (res_1, ws_1)
    check(lib().js2t_ctc_beam_search(p(out), 0, p(pick_lse), p(cand_id), p(cand_lp), p(in_len if packed else len_1), p(ids), p(n), p(score), p(ws),
                                     i64(B if packed else 1), i64(Tmax if packed else T), i64(V), i32(K), i32(NC), i32(1), i64(blank), i64(pad),
                                     p(seg) if packed else None, st()), "js2t_ctc_beam_search")


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


work = [("js2t_ctc_stitch f32", lambda: stitch(logits)), ("index_select + row_lse + gather f32", lambda: torch_route(logits)),
        ("js2t_ctc_stitch bf16", lambda: stitch(logits16)), ("index_select + row_lse + gather bf16", lambda: torch_route(logits16)),
        ("js2t_ctc_segment", segment), ("js2t_beam_pick (candidates)", pick),
        (f"js2t_ctc_beam_search {B} packed segments", lambda: beam(True)), ("js2t_ctc_beam_search one utterance", lambda: beam(False))]
pick()
for _, fn in work:
    timed(fn, 1)
stitch(logits)  # (the bf16 rounds leave the rounded stream behind: the beam is timed and checked on the f32 one)
pick()
times = {name: [] for name, _ in work[4:]}
for _ in range(args.rounds):
    for name, fn in work[4:]:
        times[name].append(timed(fn, args.reps))
beam(True), beam(False)
torch.cuda.synchronize()
# both routes find the planted labelling: the segments' hypotheses, back to back, are the one utterance's
want = [int(v) for v in planted.tolist() if v != blank]
got_p = [v for b in range(B) for v in res_p[0][b, 0, :int(res_p[1][b, 0])].tolist()]
got_1 = res_1[0][0, 0, :int(res_1[1][0, 0])].tolist()
assert got_p == want and got_1 == want, "a route did not find the planted labelling"
for _ in range(args.rounds):
    for name, fn in work[:4]:
        times.setdefault(name, []).append(timed(fn, args.reps))

HBM = 8.0  # TB/s, the data-sheet rate DESIGN.md measures against
moved = {"f32": T * V * 8 + T * 16, "bf16": T * V * 6 + T * 16}  # one read of the kept rows, one f32 write, the three statistics
print(f"T {T} encoder frames (10 min), V {V}, {W} windows of {S}; {B} segments of {int(in_len.min())}..{Tmax} frames "
      f"({int(in_len.sum())} frames kept), {len(want)} labels; beam {K}, {NC} candidates")
for name, _ in work:
    v = times[name]
    med = statistics.median(v)
    extra = ""
    if name.startswith("js2t_ctc_stitch"):
        nbytes = moved[name.split()[-1]]
        extra = f"  {nbytes / 1e6:.1f} MB moved: {nbytes / med / 1e6:.2f} TB/s = {nbytes / med / 1e6 / HBM:.2f} of {HBM:.0f} TB/s"
    print(f"{name:44s} {med:10.1f} us  (min {min(v):.1f}, max {max(v):.1f} over {args.rounds} rounds of {args.reps}){extra}")
