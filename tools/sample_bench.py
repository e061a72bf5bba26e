"""The sampling step of the attention decoder, at the sizes the decoder runs it.

Part 1, the selection: js2t_sample_step against js2t_beam_step at beam 1 - the selection the greedy loop already pays - on the same
logits (5 * randn, f32), same process: rows {32, 256, 512} x V {5000, 10000}; filters off / top_k = 50 / top_p = 0.9 / epsilon,
top-k and nucleus together.  C entry points, pre-allocated outputs, alternating rounds, device events, medians; bytes (the logits
once) over time against the 6.29 TB/s a float4 copy reaches.
Part 2, the step graph: one replayed `IncrementalDecoder` step of bench.py's decode model (bf16) at rows = 32 * N, N = 8 and 16.
Part 3, the whole decode of 32 x 15 s: `sample_search` at N = 8 and 16, with and without decision="mbr", against
`search(beam_size=5)`; same batch, same process, front end and encoder included.
usage: python tools/sample_bench.py [--rounds N] [--reps N] [--decode-rounds N]   (--decode-rounds 0: part 1 alone)"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import bench  # noqa: E402
from joeys2t_amd import ops  # noqa: E402
from joeys2t_amd._lib import check, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--decode-rounds", type=int, default=5)
args = ap.parse_args()

dev = torch.device("cuda:0")
COPY_RATE = 6.29e12
p, st, i64, i32, f32 = ops._p, ops._stream, C.c_int64, C.c_int32, C.c_float
FORBID = (C.c_int32 * 3)(0, 2, 4)
FILTERS = [("off", dict(k=0, p=1.0, eps=0.0)), ("top_k 50", dict(k=50, p=1.0, eps=0.0)), ("top_p 0.9", dict(k=0, p=0.9, eps=0.0)),
           ("eps 0.005 + top_k 50 + top_p 0.9", dict(k=50, p=0.9, eps=0.005))]


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


# ------------------------------------------------------------------ part 1: the selection step
print("js2t_sample_step against js2t_beam_step (beam 1), logits 5 * randn f32, 3 forbidden ids", flush=True)
selection = {}
for rows in (32, 256, 512):
    for V in (5000, 10000):
        gen = torch.Generator(device=dev).manual_seed(rows + V)
        logits = 5.0 * torch.randn((rows, V), generator=gen, device=dev)
        u = torch.rand((rows, ), generator=gen, device=dev)
        ids = torch.zeros((rows, 4), dtype=torch.int64, device=dev)
        logp, q, score = (torch.zeros((rows, ), device=dev) for _ in range(3))
        kept, length = (torch.zeros((rows, ), dtype=torch.int32, device=dev) for _ in range(2))
        cdf = torch.zeros((rows, 2), device=dev)
        fin = torch.zeros((rows, ), dtype=torch.uint8, device=dev)
        zero, b_scores, b_lse = (torch.zeros((rows, ), device=dev) for _ in range(3))
        b_ids = torch.zeros((rows, ), dtype=torch.int64, device=dev)

        def sample(f):
            fin.zero_()  # (a row that drew EOS would be skipped by the next launch)
            check(lib().js2t_sample_step(p(logits), i64(V), p(u), p(fin), p(ids), i64(4), i32(1), p(logp), p(q), p(score), p(length), p(kept),
                                         p(cdf), i64(rows), i64(V), FORBID, i32(3), f32(1.0), i32(f["k"]), f32(f["p"]), f32(f["eps"]), i64(3),
                                         i64(1), st()), "js2t_sample_step")

        def greedy():
            fin.zero_()  # (the same extra launch in both timed windows)
            check(lib().js2t_beam_step(p(logits), p(zero), p(b_scores), p(b_ids), p(b_lse), i64(rows), i32(1), i64(V), FORBID, i32(3), f32(0.0),
                                       st()), "js2t_beam_step")

        def clear():
            fin.zero_()

        runs = [("beam_step", greedy), ("clear", clear)] + [(name, (lambda f=f: sample(f))) for name, f in FILTERS]
        for _, fn in runs:
            timed(fn, 3)
        times = {name: [] for name, _ in runs}
        for _ in range(args.rounds):
            for name, fn in runs:
                times[name].append(timed(fn, args.reps))
        base = statistics.median(times["clear"])
        g = statistics.median(times["beam_step"]) - base
        line = f"rows {rows:3d} V {V:5d}: beam_step {g:7.2f} us ({rows * V * 4 / (g * 1e-6) / COPY_RATE:.2f} of the copy rate)"
        for name, _ in FILTERS:
            t = statistics.median(times[name]) - base
            selection[(rows, V, name)] = t
            line += f"; {name} {t:7.2f} us = {t / g:.2f} x ({rows * V * 4 / (t * 1e-6) / COPY_RATE:.3f})"
        print(line + f"   [flag clear {base:.2f} us taken off each; medians of {args.rounds} rounds of {args.reps}]", flush=True)
if args.decode_rounds < 1:
    sys.exit(0)

# ------------------------------------------------------------------ parts 2 and 3: the step graph and the whole decode
import copy  # noqa: E402

from joeys2t_amd.batch import Batch  # noqa: E402
from joeys2t_amd.incremental import IncrementalDecoder  # noqa: E402
from joeys2t_amd.model import build_model  # noqa: E402
from joeys2t_amd.search import sample_search, search  # noqa: E402
from joeys2t_amd.tokenizers import SpeechProcessor  # noqa: E402
from joeys2t_amd.vocabulary import Vocabulary  # noqa: E402

torch.manual_seed(42)
dtype = torch.bfloat16
B, V = bench.BATCH, bench.VOCAB
model = build_model(copy.deepcopy(bench.MUSTC_MODEL), None, Vocabulary.synthetic(V))
model.finalize(dev, dtype).eval()
proc = SpeechProcessor(num_freq=80, min_length=10, max_length=5000, cmvn=dict(norm_means=True, norm_vars=True, before=True))
wave = bench.synth_waveforms(B, bench.SAMPLES).to(dev)
MAX_LEN = 100


def batch():
    feats, lengths = proc.batch_from_waveforms(wave, [bench.SAMPLES] * B, is_train=False, out_dtype=dtype)
    b = Batch(src=feats, src_length=torch.tensor(lengths, device=dev), src_prompt_mask=None, trg=None, trg_length=None, trg_prompt_mask=None,
              indices=torch.arange(B), device=dev, pad_index=1, eos_index=3, is_train=False, task="S2T", n_gpu=1)
    b.sort_by_src_length()
    return b


with torch.no_grad():
    b0 = batch()
    enc, _, mask, _ = model(return_type="encode", **vars(b0))
for N in (8, 16):
    rows = B * N
    inc = IncrementalDecoder(model, enc, mask, N, MAX_LEN)
    last = torch.full((rows, ), 5, dtype=torch.int64, device=dev)
    inc.step(last)  # captures
    steps = []
    for _ in range(3):
        steps.append(timed(lambda: inc.step(last), 30))
    t = statistics.median(steps)
    worst = selection.get((rows, 5000, FILTERS[-1][0]))
    print(f"one replayed decoder step at rows {rows} (N = {N}): {t:8.1f} us (3 runs of 30 positions: {min(steps):.1f} .. {max(steps):.1f}); "
          f"js2t_sample_step with all filters at V 5000: {worst:.1f} us = {worst / t:.3f} of the step", flush=True)
    del inc

decodes = [("search beam 5", lambda: search(model, batch(), max_output_length=MAX_LEN, beam_size=5, beam_alpha=1.0))]
for N in (8, 16):
    kw = dict(n_samples=N, max_output_length=MAX_LEN, epsilon=0.02)
    decodes.append((f"sample_search N {N} epsilon 0.02", lambda kw=kw: sample_search(model, batch(), **kw)))
    decodes.append((f"sample_search N {N} epsilon 0.02, decision mbr", lambda kw=kw: sample_search(model, batch(), decision="mbr", **kw)))
for _, fn in decodes:
    wall(fn)
dtimes = {name: [] for name, _ in decodes}
for _ in range(args.decode_rounds):
    for name, fn in decodes:
        dtimes[name].append(wall(fn))
print(f"decode of {B} x {bench.SAMPLES / 16000:.0f} s, bf16, {MAX_LEN} positions at most, front end and encoder included")
for name, _ in decodes:
    v = dtimes[name]
    print(f"{name:48s} {statistics.median(v):9.2f} ms  (min {min(v):.2f}, max {max(v):.2f} over {args.decode_rounds} rounds)")
