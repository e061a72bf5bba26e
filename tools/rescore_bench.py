"""Attention rescoring at the LS100 shape (32 utterances x 375 frames, V = 5000, beam 10, n_rescore 10, hypotheses of about 40 labels).

Part 1, the kernel: js2t_rescore on random f32 logits [320, Lp, 5000] (pre-allocated outputs, no allocator in the timed window)
against the three-pass route on the same logits - ops.log_softmax over all rows, then a gather and a masked sum in torch - and
against itself with every slot dead (no logits are read: what the two launches cost without the stream).  The achieved share of the
HBM rate counts the live rows' bytes once over the time of the whole call (launch 2 included: a lower bound for launch 1).
Part 2, the decode: search.ctc_attention_rescore (front end, encoder, CTC n-best, one teacher-forced decoder pass, rescoring)
against search(beam_size=5) and search(beam_size=5, ctc_weight=0.3) on the same batch in the same process, bench.py's decode model
and waveforms (random init, bf16).  A random-init CTC head labels nearly every frame, so the tool adds a planted labelling (a label
every ninth frame, blanks between: about 41 labels) to the CTC logits the model computes - one small launch inside the timed window.
Alternating rounds; device events for part 1, a host clock around synchronised work for part 2; medians.
usage: python tools/rescore_bench.py [--rounds N] [--reps N] [--decode-rounds N]   (--decode-rounds 0: part 1 alone, for a kernel trace)"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from joeys2t_amd import alignment, ops  # noqa: E402
from joeys2t_amd._lib import check, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--decode-rounds", type=int, default=5)
args = ap.parse_args()

HBM_TBS = 8.0  # HBM3E, data-sheet rate
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(11)
B, N, V, eos = bench.BATCH, 10, bench.VOCAB, 3
R = B * N

# ------------------------------------------------------------------ part 1: the kernel
n = torch.randint(34, 47, (R, ), generator=g, dtype=torch.int32)
Lp = int(n.max()) + 1
T = 375
logits = (torch.randn(R, Lp, V, generator=g) * 4.0).to(dev)
ids = torch.randint(0, V, (B, N, T), generator=g).to(dev)
n = n.to(dev)
ctc = -(torch.rand(R, generator=g) + 0.5).to(dev) * (n.float() + 1) * 16.0
dead_ctc = torch.full_like(ctc, float("-inf"))
out = (torch.empty((R, Lp), device=dev), torch.empty((R, ), device=dev), torch.empty((R, ), device=dev),
       torch.empty((B, N), dtype=torch.int32, device=dev))
p, st, i64, i32 = ops._p, ops._stream, C.c_int64, C.c_int32


def rescore(scores=ctc):
    check(lib().js2t_rescore(p(logits), 0, p(ids), i64(T), p(n), p(scores), p(out[0]), p(out[1]), p(out[2]), p(out[3]), i64(B), i32(N), i64(Lp),
                             i64(V), i64(eos), C.c_float(0.3), st()), "js2t_rescore")


pos = torch.arange(Lp, device=dev)[None, :]
gold = torch.cat([ids.view(R, T)[:, :Lp - 1], torch.full((R, 1), eos, dtype=torch.int64, device=dev)], dim=1)
gold = torch.where(pos == n.view(R, 1), torch.full_like(gold, eos), gold)
live = pos <= n.view(R, 1)


def three_pass():
    lp = ops.log_softmax(logits.view(R * Lp, V)).view(R, Lp, V)
    tok = lp.gather(2, gold.unsqueeze(-1)).squeeze(-1)
    return torch.where(live, tok, torch.zeros_like(tok)).sum(dim=1)


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


work = [("js2t_rescore", rescore), ("js2t_rescore, every slot dead", lambda: rescore(dead_ctc)),
        ("ops.log_softmax + gather + sum (three passes)", three_pass)]
for _, fn in work:
    timed(fn, 3)
times = {name: [] for name, _ in work}
for _ in range(args.rounds):
    for name, fn in work:
        times[name].append(timed(fn, args.reps))
rescore()
want = three_pass()
torch.cuda.synchronize()
err = float(((out[1] - want).abs() / want.abs().clamp(min=1.0)).max())
assert err <= 1e-4, f"js2t_rescore and the three-pass route disagree: {err}"
live_bytes = int(live.sum()) * V * 4
print(f"R {R} (B {B} x N {N}) Lp {Lp} V {V} f32, hypotheses of {int(n.min())}..{int(n.max())} labels: {int(live.sum())} live rows, "
      f"{live_bytes / 1e6:.1f} MB (all rows: {R * Lp * V * 4 / 1e6:.1f} MB); worst relative difference of the sums {err:.2e}")
for name, _ in work:
    v = times[name]
    print(f"{name:48s} {statistics.median(v):9.1f} us  (min {min(v):.1f}, max {max(v):.1f} over {args.rounds} rounds of {args.reps})")
us = statistics.median(times["js2t_rescore"])
print(f"js2t_rescore: {live_bytes / us / 1e6:.2f} TB/s over the live rows = {live_bytes / us / 1e6 / HBM_TBS:.2f} of the {HBM_TBS} TB/s HBM rate; "
      f"{statistics.median(times['ops.log_softmax + gather + sum (three passes)']) / us:.1f} x the three-pass route", flush=True)
del logits, want, gold, live
if args.decode_rounds < 1:  # part 1 alone, e.g. under a kernel trace: --decode-rounds 0
    sys.exit(0)

# ------------------------------------------------------------------ part 2: the whole decode
import copy  # noqa: E402

from joeys2t_amd.batch import Batch  # noqa: E402
from joeys2t_amd.model import build_model  # noqa: E402
from joeys2t_amd.search import ctc_attention_rescore, search  # noqa: E402
from joeys2t_amd.tokenizers import SpeechProcessor  # noqa: E402
from joeys2t_amd.vocabulary import Vocabulary  # noqa: E402

torch.manual_seed(42)
dtype = torch.bfloat16
model = build_model(copy.deepcopy(bench.MUSTC_MODEL), None, Vocabulary.synthetic(V))
model.finalize(dev, dtype).eval()
proc = SpeechProcessor(num_freq=80, min_length=10, max_length=5000, cmvn=dict(norm_means=True, norm_vars=True, before=True))
wave = bench.synth_waveforms(B, bench.SAMPLES).to(dev)
planted = {}
ctc_frames = alignment._ctc_frames


def planted_ctc_frames(model, batch, **kw):
    res = ctc_frames(model, batch, **kw)
    ctc_out = res[0]
    Bq, Tq, Vq = ctc_out.shape
    if (Bq, Tq) not in planted:
        path = torch.full((Bq, Tq), model.bos_index, dtype=torch.int64)
        path[:, ::9] = torch.randint(4, Vq, (Bq, (Tq + 8) // 9), generator=g)
        planted[(Bq, Tq)] = (path.unsqueeze(-1).to(dev), torch.full((Bq, Tq, 1), 30.0, dtype=ctc_out.dtype, device=dev))
    ctc_out.scatter_add_(2, *planted[(Bq, Tq)])
    return res


alignment._ctc_frames = planted_ctc_frames


def batch():
    feats, lengths = proc.batch_from_waveforms(wave, [bench.SAMPLES] * B, is_train=False, out_dtype=dtype)
    b = Batch(src=feats, src_length=torch.tensor(lengths, device=dev), src_prompt_mask=None, trg=None, trg_length=None, trg_prompt_mask=None,
              indices=torch.arange(B), device=dev, pad_index=1, eos_index=3, is_train=False, task="S2T", n_gpu=1)
    b.sort_by_src_length()
    return b


lengths = {}


def two_pass():
    _, _, hyp_n = ctc_attention_rescore(model, batch(), beam_size=N, n_best=1, n_rescore=N, ctc_weight=0.3)
    lengths["two-pass"] = (int(hyp_n.min()), int(hyp_n.max()))


def beam5(**extra):
    search(model, batch(), max_output_length=100, beam_size=5, beam_alpha=1.0, n_best=1, **extra)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


decodes = [("ctc_attention_rescore beam 10, n_rescore 10", two_pass), ("search beam 5", beam5),
           ("search beam 5, ctc_weight 0.3", lambda: beam5(ctc_weight=0.3, ctc_candidates=8))]
for _, fn in decodes:
    wall(fn)
dtimes = {name: [] for name, _ in decodes}
for _ in range(args.decode_rounds):
    for name, fn in decodes:
        dtimes[name].append(wall(fn))
print(f"decode of {B} x {bench.SAMPLES / 16000:.0f} s, bf16, front end and encoder included; two-pass hypotheses of {lengths['two-pass'][0]}.."
      f"{lengths['two-pass'][1]} labels")
for name, _ in decodes:
    v = dtimes[name]
    print(f"{name:48s} {statistics.median(v):9.2f} ms  (min {min(v):.2f}, max {max(v):.2f} over {args.decode_rounds} rounds)")
