"""js2t_ctc_align at the LS100 shape (B = 32, T' = 375, V = 5000, random targets of 40 to 90 labels) against the shipped
js2t_ctc_alpha without beta, in one process on the same inputs: both C entry points are called with pre-allocated outputs (no
allocator in the timed window), in alternating rounds, timed with device events; prints the median of the rounds for each and their
ratio.  usage: python tools/align_bench.py [--dtype f32|bf16] [--rounds N]"""
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
ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(7)
B, T, V, blank = 32, 375, 5000, 2
tgt_len = torch.randint(40, 91, (B,), generator=g)
Lmax = int(tgt_len.max())
targets = torch.randint(4, V, (B, Lmax), generator=g).to(dev)
in_len = torch.cat([torch.tensor([T]), torch.randint(250, T + 1, (B - 1,), generator=g)]).to(dev)
tgt_len = tgt_len.to(dev)
logits = (torch.randn(B, T, V, generator=g) * 2.0).to(torch.float32 if args.dtype == "f32" else torch.bfloat16).to(dev)
lse, _ = ops.row_lse(logits.view(B * T, V))

p, st, i64 = ops._p, ops._stream, C.c_int64
path = torch.empty((B, T), dtype=torch.int32, device=dev)
tok_start, tok_end = torch.empty((B, Lmax), dtype=torch.int32, device=dev), torch.empty((B, Lmax), dtype=torch.int32, device=dev)
frame_logp, score = torch.empty((B, T), device=dev), torch.empty((B,), device=dev)
ws = torch.empty((max(ops.ctc_align_workspace_bytes(B, T, Lmax), 1),), dtype=torch.uint8, device=dev)
alpha = torch.empty((B, T, 2 * Lmax + 1), device=dev)
nll, loss_rows = torch.empty((B,), device=dev), torch.empty((B,), device=dev)
dt = ops.dt_code(logits)


def align():
    check(lib().js2t_ctc_align(p(logits), dt, p(lse), p(targets), p(in_len), p(tgt_len), p(path), p(tok_start), p(tok_end), p(frame_logp),
                               p(score), p(ws), i64(B), i64(T), i64(V), i64(Lmax), i64(blank), None, st()), "js2t_ctc_align")


def alpha_only():
    check(lib().js2t_ctc_alpha(p(logits), dt, p(lse), p(targets), p(in_len), p(tgt_len), p(alpha), None, p(nll), p(loss_rows), i64(B),
                               i64(T), i64(V), i64(Lmax), i64(blank), 0, None, st()), "js2t_ctc_alpha")


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


for fn in (align, alpha_only):
    timed(fn, 10)
t_align, t_alpha = [], []
for _ in range(args.rounds):
    t_align.append(timed(align, args.reps))
    t_alpha.append(timed(alpha_only, args.reps))
assert bool((score <= -nll + 1e-4 * nll.abs().clamp(min=1.0)).all()) and bool(torch.isfinite(score).all())
a, b = statistics.median(t_align), statistics.median(t_alpha)
print(f"B {B} T' {T} V {V} labels {int(tgt_len.min())}..{Lmax} (2 Lmax + 1 = {2 * Lmax + 1}) {args.dtype}")
print(f"js2t_ctc_align            {a:8.1f} us  (min {min(t_align):.1f}, max {max(t_align):.1f} over {args.rounds} rounds of {args.reps})")
print(f"js2t_ctc_alpha, no beta   {b:8.1f} us  (min {min(t_alpha):.1f}, max {max(t_alpha):.1f}; includes its loss_rows launch)")
print(f"ratio align / alpha       {a / b:8.2f}")
