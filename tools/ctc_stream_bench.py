"""js2t_ctc_stream_step, us per call, beside the one-shot kernel (js2t_ctc_beam_search_ctx, all weights 0) on the same rows in the same
run: 1 stream x 10 frames and 32 streams x 25 frames of V = 5000 f32 logits with a planted labelling (a label every fourth frame),
beam 10, 8 candidates, n_best 1.  The streams stay inside one open segment (min_silence 0, max_len 1500): a call is the state's
load and store, the frames' recursion and the partial back-trace, whose length is the segment's label count - so every shape is
timed from two places, a fresh segment and 250 frames into one.  A round restores the saved state (outside the timed window) and
times `reps` consecutive calls; rounds of the stream step and of the one-shot launch alternate; device events; the median over the
rounds.  C entry points with pre-allocated outputs: no allocator and no host read in the timed window.
usage: python tools/ctc_stream_bench.py [--rounds N] [--reps N] [--time-limit SECONDS]"""
import argparse
import ctypes as C
import json
import signal
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from joeys2t_amd import ops  # noqa: E402
from joeys2t_amd._lib import check, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--time-limit", type=int, default=240)
args = ap.parse_args()
signal.alarm(args.time_limit)  # the tool's own time limit: SIGALRM ends the process

dev = torch.device("cuda:0")
V, K, NC, NB, blank, pad, bos, eos, MAX_LEN, AHEAD = 5000, 10, 8, 1, 2, 1, 2, 3, 1500, 250
p, st, i64, i32, f32 = ops._p, ops._stream, C.c_int64, C.c_int32, C.c_float


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


results = []
for B, T in ((1, 10), (32, 25)):
    g = torch.Generator().manual_seed(7 + B)
    planted = torch.full((B, T), blank, dtype=torch.int64)
    planted[:, ::4] = torch.randint(4, V, (B, (T + 3) // 4), generator=g)
    logits = torch.randn(B, T, V, generator=g)
    logits.scatter_add_(2, planted.unsqueeze(-1), torch.full((B, T, 1), 14.0))
    logits = logits.to(dev).view(B * T, V)
    cand_id, cand_lp, lse = ops.ctc_beam_candidates(logits, NC, blank)
    _, argmax = ops.row_lse(logits, want_argmax=True)
    off = torch.arange(B + 1, dtype=torch.int32, device=dev) * T
    in_len = torch.full((B, ), T, dtype=torch.int64, device=dev)
    state = ops.ctc_stream_state(B, K, MAX_LEN, dev)
    out = ops.ctc_stream_outputs(dev, B, NB, 1, MAX_LEN)
    ws = torch.empty((ops.ctc_beam_workspace_bytes(B, T, K), ), dtype=torch.uint8, device=dev)
    o_ids, o_n = torch.empty((B, NB, T), dtype=torch.int64, device=dev), torch.empty((B, NB), dtype=torch.int32, device=dev)
    o_score, o_ctc, o_lm = (torch.empty((B, NB), device=dev) for _ in range(3))
    o_ctx = torch.empty((B, NB), dtype=torch.int32, device=dev)

    def step():
        check(lib().js2t_ctc_stream_step(p(logits), p(lse), p(argmax), p(cand_id), p(cand_lp), p(off), None, None, None, i64(0), i32(1), i32(1), None,
                                         None, i64(0), i32(1), i32(0), i32(0), p(state), p(out["fin_ids"]), p(out["fin_len"]), p(out["fin_score"]),
                                         p(out["fin_ctc"]), p(out["fin_lm"]), p(out["fin_ctx"]), p(out["fin_start"]), p(out["fin_n"]),
                                         p(out["fin_why"]), p(out["consumed"]), p(out["n_final"]), p(out["part_ids"]), p(out["part_len"]),
                                         p(out["stable_len"]), p(out["part_start"]), i64(B), i64(B * T), i64(V), i32(K), i32(NC), i32(NB), i32(1),
                                         i64(MAX_LEN), i64(blank), i64(pad), i64(bos), i64(eos), f32(0.0), f32(0.0), f32(0.0), f32(-0.1), i32(0),
                                         st()), "js2t_ctc_stream_step")

    def one_shot():
        check(lib().js2t_ctc_beam_search_ctx(p(logits), 0, p(lse), p(cand_id), p(cand_lp), p(in_len), None, None, i64(0), i32(1), i32(1), None, None,
                                             i64(0), i32(1), i32(0), i32(0), p(o_ids), p(o_n), p(o_score), p(o_ctc), p(o_lm), p(o_ctx), p(ws), i64(B),
                                             i64(T), i64(V), i32(K), i32(NC), i32(NB), i64(blank), i64(pad), i64(bos), i64(eos), f32(0.0), f32(0.0),
                                             f32(0.0), None, st()), "js2t_ctc_beam_search_ctx")

    # the first call of a fresh stream is the one-shot search of its rows: the same labels, the same score
    step()
    one_shot()
    torch.cuda.synchronize()
    n = int(out["part_len"][0])
    assert int(out["consumed"][0]) == T and int(out["part_start"][0]) == 0 and n == int(o_n[0, 0]) > 0
    assert torch.equal(out["part_ids"][0, :n], o_ids[0, 0, :n])
    for ahead in (0, AHEAD):
        state.zero_()
        for _ in range(ahead // T):
            step()
        torch.cuda.synchronize()
        saved = state.clone()
        assert (ahead + (args.reps + 3) * T) < MAX_LEN  # the segment stays open through a round
        timed(step, 3)
        timed(one_shot, 3)
        t_step, t_one = [], []
        for _ in range(args.rounds):
            state.copy_(saved)
            t_step.append(timed(step, args.reps))
            t_one.append(timed(one_shot, args.reps))
        labels = int(out["part_len"][0])
        r = dict(streams=B, frames=T, frames_into_segment=ahead, labels_at_the_end_of_a_round=labels, stream_step_us=statistics.median(t_step),
                 one_shot_us=statistics.median(t_one), stream_step_min_max=[min(t_step), max(t_step)], one_shot_min_max=[min(t_one), max(t_one)],
                 state_bytes_per_stream=state.shape[1])
        results.append(r)
        print(f"{B:2d} streams x {T} frames, {ahead:3d} frames into the segment ({labels} labels at the end of a round): stream step "
              f"{r['stream_step_us']:7.1f} us (min {min(t_step):.1f}, max {max(t_step):.1f}), one-shot {r['one_shot_us']:7.1f} us (min {min(t_one):.1f}, "
              f"max {max(t_one):.1f}) over {args.rounds} rounds of {args.reps}", flush=True)
print(json.dumps(dict(V=V, beam=K, candidates=NC, n_best=NB, results=results)))
