"""js2t_ctc_spot at the LS100 shape: a synthetic 10-minute recording - T = 15000 encoder frames of 40 ms, V = 5000 - searched for
K in {1, 64, 1024} phrases of L = 4 and of L = 32 labels; phrase 0 is planted every 500 frames, the others are random ids.  Timed in
one process, the C entry point with pre-allocated outputs, alternating rounds, device events, medians; with and without the dense
frame_score / frame_start outputs at K = 64.  At K = 1 - one wavefront, sequential in T - the float32 NumPy reference of the tests
runs on the host for the same inputs (once per L), and the kernel must give its frame_score bits, frame_start and hits.
The kernel's only memory traffic are the gathers of one logit per (frame, state): bytes = T * (2 L - 1) * 4 per phrase, reported as
a rate for what it is - a latency-bound gather, not a share of the HBM peak.
usage: python tools/spot_bench.py [--rounds N] [--reps N]"""
import argparse
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import ctc_spot_reference as RS  # noqa: E402
from joeys2t_amd import ops  # noqa: E402
from joeys2t_amd._lib import check, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

dev = torch.device("cuda:0")
T, V, blank, ROOM = 15000, 5000, 2, 64
thr = math.log(0.5)
p, st = ops._p, ops._stream


def case(K, L, seed):
    """(logits f32 [T, V] on the device, norm = the row maximum, tokens i64 [K, L], lengths): phrase 0 planted every 500 frames, one
    frame per label, +14 on the planted id"""
    gen = torch.Generator().manual_seed(seed)
    tokens = torch.randint(4, V, (K, L), generator=gen)
    tokens[0] = torch.randperm(V - 4, generator=gen)[:L] + 4  # (no repeats: no blank frame needed)
    x = torch.randn((T, V), generator=torch.Generator(device=dev).manual_seed(seed), device=dev)
    at = torch.arange(250, T - L, 500)
    rows = (at[:, None] + torch.arange(L)[None, :]).reshape(-1)
    x[rows.to(dev), tokens[0].repeat(at.numel()).to(dev)] += 14.0
    return x, x.max(dim=1).values.contiguous(), tokens.to(dev), torch.full((K, ), L, dtype=torch.int32, device=dev), at.numel()


def outputs(K, dense):
    return (torch.empty((K, ), dtype=torch.int32, device=dev), torch.empty((K, ROOM), dtype=torch.int32, device=dev),
            torch.empty((K, ROOM), dtype=torch.int32, device=dev), torch.empty((K, ROOM), device=dev),
            torch.empty((K, T), device=dev) if dense else None, torch.empty((K, T), dtype=torch.int32, device=dev) if dense else None)


def spot_call(x, norm, tok, length, out):
    K, L = tok.shape
    check(lib().js2t_ctc_spot(p(x), 0, p(norm), p(tok), p(length), K, L, p(out[0]), p(out[1]), p(out[2]), p(out[3]), ROOM, p(out[4]), p(out[5]),
                              T, V, blank, thr, st()), "js2t_ctc_spot")


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


work, checks = [], []
for L in (4, 32):
    inputs = {K: case(K, L, 10 * L + i) for i, K in enumerate((1, 64, 1024))}
    for K, (x, norm, tok, length, planted) in inputs.items():
        for dense in ((False, True) if K == 64 else (False, )):
            out = outputs(K, dense)
            work.append((f"K {K:5d} L {L:2d}{' + dense outputs' if dense else ''}", (lambda a=(x, norm, tok, length, out): spot_call(*a)), K, L))
        if K == 1:
            checks.append((L, x, norm, tok, length, planted))
for _, fn, _, _ in work:
    timed(fn, 1)
times = {name: [] for name, _, _, _ in work}
for _ in range(args.rounds):
    for name, fn, _, _ in work:
        times[name].append(timed(fn, args.reps))

print(f"T {T} V {V}; tiles (most labels per phrase, phrases per block, frames per prefetch group) {ops.ctc_spot_tiles()}; threshold 0.5")
for name, _, K, L in work:
    v = times[name]
    med = statistics.median(v)
    gathered = K * T * (2 * L - 1) * 4
    print(f"js2t_ctc_spot {name:28s} {med:10.1f} us = {med / T * 1e3:7.1f} ns per frame, {med / K:9.2f} us per phrase, "
          f"{gathered / med * 1e-3:7.2f} GB/s gathered  (min {min(v):.1f}, max {max(v):.1f} over {args.rounds} rounds of {args.reps})")
for L, x, norm, tok, length, planted in checks:
    out = outputs(1, True)
    spot_call(x, norm, tok, length, out)
    torch.cuda.synchronize()
    xh, nh, phrase = x.cpu().numpy(), norm.cpu().numpy(), tok[0].cpu().tolist()
    t0 = time.perf_counter()
    h, s = RS.spot(xh, nh, phrase, blank, np.float32)
    hits = RS.pick(h, s, np.float32(thr))
    host = time.perf_counter() - t0
    n = int(out[0].item())
    got = list(zip(out[1][0, :n].tolist(), out[2][0, :n].tolist(), out[3][0, :n].tolist()))
    assert n == len(hits) == planted and got == [(a, e, float(sc)) for a, e, sc in hits], "the kernel's hits differ from the float32 reference"
    assert np.array_equal(out[4][0].cpu().numpy().view(np.int32), h.view(np.int32)) and np.array_equal(out[5][0].cpu().numpy(), s), \
        "the kernel's frame_score bits or frame_start differ from the float32 reference"
    print(f"float32 NumPy reference on the host: K 1 L {L:2d} {host * 1e3:.0f} ms; same frame_score bits, frame_start and {n} hits")
