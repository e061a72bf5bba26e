"""js2t_ctc_align_long at the LS100 shape: a synthetic 10-minute recording - T = 15000 encoder frames of 40 ms, V = 5000 - and its
transcript of L = 3000 labels, planted one every fifth frame behind a head and in front of a tail the text lacks.  Timed in one
process, the C entry point with pre-allocated outputs and workspace, alternating rounds, device events, medians:
  the whole call (every forward launch, the back-trace, the outputs) at ten minutes, free ends on;
  the same call and js2t_ctc_align on the largest shape both run (L = 511, i.e. S = 1023; T = 2500), with the per-frame time of each;
  the float32 NumPy reference of the tests on the host for the same inputs (once), whose path and score bits the kernel must give.
The call is not taken apart: forward launches and back-trace are enqueued inside one entry point, so the tool reports their sum.
usage: python tools/align_long_bench.py [--rounds N] [--reps N]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import ctc_align_long_reference as RL  # noqa: E402
from joeys2t_amd import ops  # noqa: E402
from joeys2t_amd._lib import check, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

dev = torch.device("cuda:0")
V, blank = 5000, 2
p, st = ops._p, ops._stream


def recording(T, L, seed):
    """(logits f32 [T, V] on the device, lse, targets i64 [L]): the labels planted every (T - 2 head) / L frames, blanks elsewhere"""
    gen_h = torch.Generator().manual_seed(seed)
    head = T // 30
    step = (T - 2 * head) // L
    targets = torch.randint(4, V, (L, ), generator=gen_h)
    planted = torch.full((T, ), blank, dtype=torch.int64)
    planted[head:head + L * step:step] = targets
    planted[:head] = planted[T - head:] = 3  # an id the text lacks
    x = torch.randn((T, V), generator=torch.Generator(device=dev).manual_seed(seed), device=dev)
    x.scatter_add_(1, planted.to(dev).unsqueeze(1), torch.full((T, 1), 14.0, device=dev))
    return x, ops.row_lse(x)[0], targets.to(dev)


def outputs(T, L):
    return (torch.empty((T, ), dtype=torch.int32, device=dev), torch.empty((L, ), dtype=torch.int32, device=dev),
            torch.empty((L, ), dtype=torch.int32, device=dev), torch.empty((T, ), device=dev), torch.empty((1, ), device=dev))


def long_call(x, lse, tg, out, ws, free):
    T, L = x.shape[0], tg.shape[0]
    check(lib().js2t_ctc_align_long(p(x), 0, p(lse), p(tg), *(p(o) for o in out), p(ws), T, V, L, blank, free, free, st()), "js2t_ctc_align_long")


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def host_reference(x, lse, tg, free):
    lp = (x - lse[:, None]).cpu().numpy()
    t0 = time.perf_counter()
    ref = RL.align_free(lp, tg.cpu().numpy(), blank, free, free, dtype=np.float32)
    return ref, time.perf_counter() - t0


def same(out, ref):
    return (np.array_equal(out[0].cpu().numpy(), ref["path"]) and
            np.array_equal(out[4].cpu().numpy().view(np.int32), np.float32([ref["score"]]).view(np.int32)))


tiles = ops.ctc_align_long_tiles()
# ten minutes
T10, L10 = 15000, 3000
x10, lse10, tg10 = recording(T10, L10, 7)
ws10 = torch.empty((ops.ctc_align_long_workspace_bytes(T10, L10), ), dtype=torch.uint8, device=dev)
out10 = outputs(T10, L10)
# the shape js2t_ctc_align also runs
Ts, Ls = 2500, 511
xs, lses, tgs = recording(Ts, Ls, 8)
wss = torch.empty((ops.ctc_align_long_workspace_bytes(Ts, Ls), ), dtype=torch.uint8, device=dev)
outs = outputs(Ts, Ls)
old_ws = torch.empty((ops.ctc_align_workspace_bytes(1, Ts, Ls), ), dtype=torch.uint8, device=dev)
old_out = outputs(Ts, Ls)
in_len, tgt_len = torch.tensor([Ts], device=dev), torch.tensor([Ls], device=dev)


def old_call():
    check(lib().js2t_ctc_align(p(xs), 0, p(lses), p(tgs), p(in_len), p(tgt_len), *(p(o) for o in old_out), p(old_ws), 1, Ts, V, Ls, blank, None,
                               st()), "js2t_ctc_align")


work = [(f"js2t_ctc_align_long T {T10} L {L10} free ends", lambda: long_call(x10, lse10, tg10, out10, ws10, 1), T10),
        (f"js2t_ctc_align_long T {Ts} L {Ls}", lambda: long_call(xs, lses, tgs, outs, wss, 0), Ts),
        (f"js2t_ctc_align      T {Ts} L {Ls}", old_call, Ts)]
for _, fn, _ in work:
    timed(fn, 1)
assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs, old_out)), "the two kernels differ at the shared shape"
times = {name: [] for name, _, _ in work}
for _ in range(args.rounds):
    for name, fn, _ in work:
        times[name].append(timed(fn, args.reps))
ref10, host10 = host_reference(x10, lse10, tg10, True)
refs, hosts = host_reference(xs, lses, tgs, False)
assert same(out10, ref10) and same(outs, refs), "the kernel's path or score bits differ from the float32 reference"
ntile, ncol = -(-T10 // tiles[3]), -(-(2 * L10 + 1) // tiles[2])
print(f"V {V}; tiles (states per lane, wave, block column; frames per launch tile) {tiles}; ten minutes: {ncol} block columns x {ntile} "
      f"time tiles = {ntile + ncol - 1} forward launches + 2, workspace {ws10.numel()} bytes; score {float(out10[4]):.3f}")
for name, _, T in work:
    v = times[name]
    med = statistics.median(v)
    print(f"{name:48s} {med:10.1f} us = {med / T * 1e3:7.1f} ns per frame  (min {min(v):.1f}, max {max(v):.1f} over {args.rounds} rounds of {args.reps})")
print(f"float32 NumPy reference on the host: T {T10} L {L10} {host10 * 1e3:.0f} ms, T {Ts} L {Ls} {hosts * 1e3:.0f} ms; same path and score bits")
