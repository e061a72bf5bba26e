"""N-gram LM rescoring at the LS100 shape (32 utterances, n_rescore 10: 320 hypotheses of 34 - 46 labels, V = 5000) with a synthetic
order-4 LM of about 2 M n-grams - a table of 64 MiB, well beyond the 4 MiB L2 of an XCD.

The LM: the 2-, 3- and 4-grams of the bench hypotheses themselves (each kept with probability 0.7, so that hits, back-offs and
misses all occur) plus random n-grams up to the size; random values.  The builder's time for it is printed.
Part 1, the kernel: js2t_ngram_rescore alone (pre-allocated outputs, no allocator in the timed window) with and without lm_tok,
against the host route a user has without it: ids and lengths copied to the host, scored there by the NumPy reference of the tests
(tests/ngram_reference.py, a dict look-up per level), scores copied back.  The two routes' scores are compared.
Part 2, the decode: search.ctc_beam_search and search.ctc_attention_rescore of the bench batch with and without the LM, same batch,
same process (bench.py's decode model and waveforms, random init, bf16, a planted labelling as in tools/rescore_bench.py).
Alternating rounds; device events for the kernel, a host clock around synchronised work for everything else; medians.
usage: python tools/ngram_bench.py [--rounds N] [--reps N] [--decode-rounds N]   (--decode-rounds 0: part 1 alone)"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import bench  # noqa: E402
import ngram_reference as G  # noqa: E402
from joeys2t_amd import alignment, ops  # noqa: E402
from joeys2t_amd._lib import check, lib  # noqa: E402
from joeys2t_amd.lm import NGramLM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--decode-rounds", type=int, default=5)
ap.add_argument("--ngrams", type=int, default=2_000_000)
args = ap.parse_args()

dev = torch.device("cuda:0")
rs = np.random.RandomState(11)
B, N, V, bos, eos = bench.BATCH, 10, bench.VOCAB, 2, 3
R, T = B * N, 375
LMW, BONUS = 0.5, 0.2

# ------------------------------------------------------------------ the hypotheses and the LM
n_np = rs.randint(34, 47, size=R).astype(np.int32)
Lp = int(n_np.max()) + 1
ids_np = rs.randint(0, V, size=(R, T)).astype(np.int64)
uni = np.stack([-rs.uniform(2.0, 9.0, size=V), -rs.uniform(0.0, 1.0, size=V)], axis=1).astype(np.float32)
share = {2: 0.5, 3: 0.35, 4: 0.15}
grams = {}
for k in (2, 3, 4):
    own = []
    for r in range(R):
        h = np.concatenate([[bos], ids_np[r, :n_np[r]], [eos]])
        own.append(np.lib.stride_tricks.sliding_window_view(h, k))
    own = np.concatenate(own)
    own = own[rs.uniform(size=len(own)) < 0.7]
    fill = rs.randint(0, V, size=(int(args.ngrams * share[k]), k))
    g = np.unique(np.concatenate([own, fill]), axis=0)
    grams[k] = (g, -rs.uniform(0.5, 6.0, size=len(g)), -rs.uniform(0.0, 1.0, size=len(g)))
t0 = time.perf_counter()
lm = NGramLM.from_arrays(uni, grams, max_load=0.5)
t_build = time.perf_counter() - t0
print(f"LM: order {lm.order}, V {V}, {lm.n_entries} n-grams in the table ({', '.join(f'{len(grams[k][0])} {k}-grams' for k in grams)}), capacity "
      f"{lm.capacity} = {lm.capacity * 16 / 2**20:.0f} MiB, max_probe {lm.max_probe}; built in {t_build:.2f} s", flush=True)
lm.to(dev)

# ------------------------------------------------------------------ part 1: the kernel against the host route
ids = torch.from_numpy(ids_np).view(B, N, T).to(dev)
n = torch.from_numpy(n_np).to(dev)
base = (-(torch.rand(R) + 0.5) * (torch.from_numpy(n_np).float() + 1) * 4.0).to(dev)
out = (torch.empty((R, Lp), device=dev), torch.empty((R, ), device=dev), torch.empty((R, ), device=dev),
       torch.empty((B, N), dtype=torch.int32, device=dev))
p, st, i64, i32, f32 = ops._p, ops._stream, C.c_int64, C.c_int32, C.c_float


def kernel(tok=True):
    check(lib().js2t_ngram_rescore(p(ids), i64(T), p(n), p(base), p(lm.uni_dev), p(lm.table_dev), i64(lm.capacity), i32(lm.max_probe),
                                   i32(lm.order), p(out[0]) if tok else None, p(out[1]), p(out[2]), p(out[3]), i64(B), i32(N), i64(Lp), i64(V),
                                   i64(bos), i64(eos), f32(LMW), f32(BONUS), st()), "js2t_ngram_rescore")


t0 = time.perf_counter()
lm_dict = {(w, ): (float(uni[w, 0]), float(uni[w, 1])) for w in range(V)}
for k, (g, lp, bo) in grams.items():
    lm_dict.update(zip(map(tuple, g.tolist()), zip(lp.astype(np.float32).astype(np.float64).tolist(), bo.astype(np.float32).astype(np.float64).tolist())))
print(f"host route: the LM as a Python dict of {len(lm_dict)} entries, made in {time.perf_counter() - t0:.1f} s (not timed below)", flush=True)
host = {}


def host_route():
    h_ids, h_n, h_base = ids.cpu().numpy(), n.cpu().numpy(), base.cpu().numpy()
    _, _, score, order = G.rescore(h_ids, h_n, h_base, N, Lp, lm_dict, V, lm.order, bos, eos, LMW, BONUS)
    host["score"], host["order"] = score, order
    return torch.from_numpy(score.astype(np.float32)).to(dev), torch.from_numpy(order.astype(np.int32)).to(dev)


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


work = [("js2t_ngram_rescore with lm_tok", kernel), ("js2t_ngram_rescore, lm_tok NULL", lambda: kernel(False))]
for _, fn in work:
    timed(fn, 3)
times = {name: [] for name, _ in work}
htimes = []
for rnd in range(args.rounds):
    for name, fn in work:
        times[name].append(timed(fn, args.reps))
    if rnd < 3:
        htimes.append(wall(host_route))
kernel()
torch.cuda.synchronize()
got = out[2].cpu().numpy().astype(np.float64)
err = float(np.max(np.abs(got - host["score"]) / np.maximum(1.0, np.abs(host["score"]))))
assert err <= 1e-4, f"js2t_ngram_rescore and the host route disagree: {err}"
same_order = int((out[3].cpu().numpy() == host["order"]).all(axis=1).sum())
positions = int(n_np.sum()) + R
print(f"R {R} (B {B} x N {N}) Lp {Lp}, hypotheses of {int(n_np.min())}..{int(n_np.max())} labels: {positions} positions; worst relative "
      f"difference of the scores {err:.2e}; {same_order} of {B} rankings equal")
for name, _ in work:
    v = times[name]
    print(f"{name:48s} {statistics.median(v):9.1f} us  (min {min(v):.1f}, max {max(v):.1f} over {args.rounds} rounds of {args.reps})")
print(f"{'host route: copy, NumPy reference, copy back':48s} {statistics.median(htimes) * 1e3:9.1f} us  (min {min(htimes) * 1e3:.1f}, max "
      f"{max(htimes) * 1e3:.1f} over {len(htimes)} runs) = {statistics.median(htimes) * 1e3 / statistics.median(times[work[0][0]]):.0f} x the kernel",
      flush=True)
del lm_dict
if args.decode_rounds < 1:
    sys.exit(0)

# ------------------------------------------------------------------ part 2: the whole decode
import copy  # noqa: E402

from joeys2t_amd.batch import Batch  # noqa: E402
from joeys2t_amd.model import build_model  # noqa: E402
from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search  # noqa: E402
from joeys2t_amd.tokenizers import SpeechProcessor  # noqa: E402
from joeys2t_amd.vocabulary import Vocabulary  # noqa: E402

torch.manual_seed(42)
g = torch.Generator().manual_seed(11)
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


with_lm = dict(lm=lm, lm_weight=LMW, length_bonus=BONUS)
decodes = [("ctc_beam_search beam 10", lambda: ctc_beam_search(model, batch(), beam_size=N, n_best=1)),
           ("ctc_beam_search beam 10 + LM", lambda: ctc_beam_search(model, batch(), beam_size=N, n_best=1, **with_lm)),
           ("ctc_attention_rescore beam 10", lambda: ctc_attention_rescore(model, batch(), beam_size=N, n_best=1, ctc_weight=0.3)),
           ("ctc_attention_rescore beam 10 + LM", lambda: ctc_attention_rescore(model, batch(), beam_size=N, n_best=1, ctc_weight=0.3, **with_lm))]
for _, fn in decodes:
    wall(fn)
dtimes = {name: [] for name, _ in decodes}
for _ in range(args.decode_rounds):
    for name, fn in decodes:
        dtimes[name].append(wall(fn))
print(f"decode of {B} x {bench.SAMPLES / 16000:.0f} s, bf16, front end and encoder included")
for name, _ in decodes:
    v = dtimes[name]
    print(f"{name:48s} {statistics.median(v):9.2f} ms  (min {min(v):.2f}, max {max(v):.2f} over {args.decode_rounds} rounds)")
