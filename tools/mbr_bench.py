"""Minimum-Bayes-risk ranking at the LS100 shape: 32 utterances, N = 10 and 32 hypotheses of 34 - 46 labels each.

The lists: variants of one planted labelling per utterance (a few substitutions, insertions and deletions each - how the lists of a
beam search look: most labels shared), and, as the worst case, unrelated random rows at the same lengths, of which nothing is
trimmed and every pair walks its whole table.
Part 1, the kernel: js2t_mbr_rescore alone (pre-allocated outputs, no allocator in the timed window) on both kinds of list, against
the host route a user has without it: ids, lengths and scores copied to the host, ranked there by the reference of the tests
(tests/mbr_reference.py), the order copied back.  The two routes' distances and risks are compared.
Part 2, the decode: search.ctc_beam_search and search.ctc_attention_rescore of the bench batch with decision="map" and "mbr", same
batch, same process (bench.py's decode model and waveforms, random init, bf16, a planted labelling as in tools/ngram_bench.py).
Alternating rounds; device events for the kernel, a host clock around synchronised work for everything else; medians.
usage: python tools/mbr_bench.py [--rounds N] [--reps N] [--decode-rounds N]   (--decode-rounds 0: part 1 alone)"""
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
import mbr_reference as M  # noqa: E402
from joeys2t_amd import alignment, ops  # noqa: E402
from joeys2t_amd._lib import check, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--decode-rounds", type=int, default=5)
args = ap.parse_args()

dev = torch.device("cuda:0")
B, V, T = bench.BATCH, bench.VOCAB, 375
SCALE = 1.0
p, st, i64, i32, f32 = ops._p, ops._stream, C.c_int64, C.c_int32, C.c_float


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


def lists(N, related, rs):
    """(ids i64 [B, N, T], n i32 [B, N], score f32 [B, N]): hypotheses of 34 - 46 labels"""
    ids = rs.randint(4, V, size=(B, N, T)).astype(np.int64)
    n = rs.randint(34, 47, size=(B, N)).astype(np.int32)
    if related:
        for b in range(B):
            base = rs.randint(4, V, size=40).tolist()
            for k in range(N):
                row = base
                while not 34 <= len(row) <= 46 or (k and row == base):
                    row = M.variant(rs, base, int(rs.randint(1, 6)))
                ids[b, k, :len(row)], n[b, k] = row, len(row)
    score = (-40.0 - np.sort(rs.uniform(0.0, 6.0, size=(B, N)), axis=1)).astype(np.float32)
    return ids, n, score


# ------------------------------------------------------------------ part 1: the kernel against the host route
print(f"js2t_mbr_rescore, B {B}, hypotheses of 34..46 labels, scale {SCALE}; JS2T_EDIT_MAX_LEN {ops.edit_max_len()}", flush=True)
for N in (10, 32):
    rs = np.random.RandomState(11 + N)
    data = {kind: lists(N, kind == "variants", rs) for kind in ("variants", "unrelated")}
    on_dev = {kind: tuple(torch.from_numpy(x).to(dev) for x in v) for kind, v in data.items()}
    Lp = 47
    out = (torch.empty((B, N, N), dtype=torch.int32, device=dev), torch.empty((B * N, ), device=dev), torch.empty((B * N, ), device=dev),
           torch.empty((B, N), dtype=torch.int32, device=dev))

    def kernel(kind):
        ids, n, score = on_dev[kind]
        check(lib().js2t_mbr_rescore(p(ids), i64(T), p(n), p(score), p(out[0]), p(out[1]), p(out[2]), p(out[3]), i64(B), i32(N), i64(Lp),
                                     f32(SCALE), st()), "js2t_mbr_rescore")

    host = {}

    def host_route(kind):
        ids, n, score = on_dev[kind]
        h_ids, h_n, h_score = ids.cpu().numpy(), n.cpu().numpy(), score.cpu().numpy()
        host[kind] = M.mbr(h_ids, h_n, h_score, N, Lp, SCALE)
        return torch.from_numpy(host[kind][3].astype(np.int32)).to(dev)

    kinds = ("variants", "unrelated")
    for kind in kinds:
        timed(lambda: kernel(kind), 3)
    times = {kind: [] for kind in kinds}
    htimes = {kind: [] for kind in kinds}
    for rnd in range(args.rounds):
        for kind in kinds:
            times[kind].append(timed(lambda: kernel(kind), args.reps))
            if rnd < (2 if N <= 10 else 1):  # (the host route of N = 32 takes seconds)
                htimes[kind].append(wall(lambda: host_route(kind)))
    pairs = B * N * (N - 1) // 2
    for kind in kinds:
        kernel(kind)
        torch.cuda.synchronize()
        rdist, _, rrisk, rorder = host[kind]
        assert np.array_equal(out[0].cpu().numpy(), rdist), f"js2t_mbr_rescore and the host route disagree on the distances ({kind})"
        err = float(np.max(np.abs(out[2].cpu().numpy().astype(np.float64) - rrisk) / np.maximum(1.0, np.abs(rrisk))))
        assert err <= 1e-4, f"js2t_mbr_rescore and the host route disagree: {err}"
        same = int((out[3].cpu().numpy() == rorder).all(axis=1).sum())
        off = rdist[:, np.triu_indices(N, 1)[0], np.triu_indices(N, 1)[1]]
        changed = int((rorder[:, 0] != 0).sum())
        k, h = statistics.median(times[kind]), statistics.median(htimes[kind]) * 1e3
        print(f"N {N:2d} {kind:9s}: {pairs} pairs, mean distance {off.mean():5.1f}; kernel {k:8.1f} us (min {min(times[kind]):.1f}, max "
              f"{max(times[kind]):.1f} over {args.rounds} rounds of {args.reps}); host route {h / 1e3:9.1f} ms (min {min(htimes[kind]):.1f}, max "
              f"{max(htimes[kind]):.1f} over {len(htimes[kind])} runs) = {h / k:.0f} x the kernel; worst relative difference of the risks {err:.1e}; "
              f"{same} of {B} rankings equal; MBR top is not slot 0 in {changed} of {B}", flush=True)
    v, u = statistics.median(times["variants"]), statistics.median(times["unrelated"])
    print(f"N {N:2d}: the list of variants takes {v / u:.2f} x the time of the unrelated rows (prefix / suffix trimming and what it leaves)", flush=True)
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
N = 10
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


mbr = dict(decision="mbr")
decodes = [("ctc_beam_search beam 10", lambda: ctc_beam_search(model, batch(), beam_size=N, n_best=1)),
           ("ctc_beam_search beam 10, decision mbr", lambda: ctc_beam_search(model, batch(), beam_size=N, n_best=1, **mbr)),
           ("ctc_attention_rescore beam 10", lambda: ctc_attention_rescore(model, batch(), beam_size=N, n_best=1, ctc_weight=0.3)),
           ("ctc_attention_rescore beam 10, decision mbr", lambda: ctc_attention_rescore(model, batch(), beam_size=N, n_best=1, ctc_weight=0.3, **mbr))]
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
