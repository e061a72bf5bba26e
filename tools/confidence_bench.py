"""Token confidence from the n-best list at the LS100 shape: 32 utterances, hypotheses of 34 - 46 labels each, on the two kinds of
list tools/mbr_bench.py ranks (variants of one planted labelling per utterance; unrelated rows at the same lengths, of which no
suffix is trimmed and every pair walks its whole table), the same generator and seeds.

Part 1, the kernel: js2t_nbest_confidence alone (pre-allocated outputs and workspace, no allocator in the timed window) at N = 10 with
P = 1 and P = 10 pivots and at N = 32 with P = 32, against
  - the host route a user has without it: ids, lengths and scores copied to the host, voted there by the reference of the tests
    (tests/confidence_reference.py), the confidences copied back; the two routes' votes must be equal;
  - js2t_mbr_rescore on the same input in the same process, alternating rounds: it pays for the forward DP of N (N - 1) / 2 pairs
    and no back-trace, js2t_nbest_confidence for P (N - 1) pairs with the direction codes and the back-trace.
Part 2, the decode: search.ctc_beam_search and search.ctc_attention_rescore of the bench batch with and without confidence=True, same
batch, same process (bench.py's decode model and waveforms, random init, bf16, a planted labelling as in tools/mbr_bench.py).
Alternating rounds; device events for the kernels, a host clock around synchronised work for everything else; medians.
The split between the forward pass and the back-trace is timed with a build variant, not a trace: a library built with
JS2T_HIPCC_EXTRA=-DJS2T_ALIGN_SKIP_TRACE returns before the back-trace; run it with JS2T_LIB=<that library> and --timing-only.
usage: python tools/confidence_bench.py [--rounds N] [--reps N] [--decode-rounds N] [--timing-only]   (--decode-rounds 0: part 1 alone)"""
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
import confidence_reference as CR  # noqa: E402
import mbr_reference as M  # noqa: E402
from joeys2t_amd import alignment, ops  # noqa: E402
from joeys2t_amd._lib import check, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--decode-rounds", type=int, default=5)
ap.add_argument("--timing-only", action="store_true", help="no host route and no comparison: for a library built with "
                "JS2T_HIPCC_EXTRA=-DJS2T_ALIGN_SKIP_TRACE (JS2T_LIB names it), whose votes are wrong by construction")
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
    """(ids i64 [B, N, T], n i32 [B, N], score f32 [B, N]): hypotheses of 34 - 46 labels (tools/mbr_bench.py's generator)"""
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


# ------------------------------------------------------------------ part 1: the kernel against the host route and the MBR kernel
print(f"js2t_nbest_confidence, B {B}, hypotheses of 34..46 labels, scale {SCALE}", flush=True)
Lp = 47
kinds = ("variants", "unrelated")
for N, P in ((10, 1), (10, 10), (32, 32)):
    rs = np.random.RandomState(11 + N)  # (tools/mbr_bench.py's seed: the same two lists)
    data = {kind: lists(N, kind == "variants", rs) for kind in kinds}
    on_dev = {kind: tuple(torch.from_numpy(x).to(dev) for x in v) for kind, v in data.items()}
    pivot = torch.arange(P, dtype=torch.int32, device=dev).expand(B, P).contiguous()  # the P best-scored slots
    need = lib().js2t_nbest_confidence_workspace(B, P, N, Lp)
    ws = torch.empty((need, ), dtype=torch.uint8, device=dev)
    out = (torch.empty((B * N, ), device=dev), torch.empty((B, P, Lp - 1), device=dev), torch.empty((B, P), device=dev),
           torch.empty((B, P, N, Lp - 1), dtype=torch.uint8, device=dev))
    mout = (torch.empty((B, N, N), dtype=torch.int32, device=dev), torch.empty((B * N, ), device=dev), torch.empty((B * N, ), device=dev),
            torch.empty((B, N), dtype=torch.int32, device=dev))

    def kernel(kind, match=True):
        ids, n, score = on_dev[kind]
        check(lib().js2t_nbest_confidence(p(ids), i64(T), p(n), p(score), p(pivot), p(out[0]), p(out[1]), p(out[2]), p(out[3]) if match else None,
                                          p(ws), i64(need), i64(B), i32(N), i32(P), i64(Lp), f32(SCALE), st()), "js2t_nbest_confidence")

    def mbr_kernel(kind):
        ids, n, score = on_dev[kind]
        check(lib().js2t_mbr_rescore(p(ids), i64(T), p(n), p(score), p(mout[0]), p(mout[1]), p(mout[2]), p(mout[3]), i64(B), i32(N), i64(Lp),
                                     f32(SCALE), st()), "js2t_mbr_rescore")

    host = {}

    def host_route(kind):
        ids, n, score = on_dev[kind]
        h_ids, h_n, h_score = ids.cpu().numpy(), n.cpu().numpy(), score.cpu().numpy()
        host[kind] = CR.confidence(h_ids, h_n, h_score, N, pivot.cpu().numpy(), Lp, SCALE)
        return torch.from_numpy(host[kind][1].astype(np.float32)).to(dev), torch.from_numpy(host[kind][2].astype(np.float32)).to(dev)

    for kind in kinds:
        timed(lambda: kernel(kind), 3)
        timed(lambda: mbr_kernel(kind), 3)
    times, ntimes, mtimes, htimes = ({kind: [] for kind in kinds} for _ in range(4))
    for rnd in range(args.rounds):
        for kind in kinds:
            times[kind].append(timed(lambda: kernel(kind), args.reps))
            mtimes[kind].append(timed(lambda: mbr_kernel(kind), args.reps))
            ntimes[kind].append(timed(lambda: kernel(kind, match=False), args.reps))
            if not args.timing_only and rnd < (2 if P * N <= 100 else 1):  # (the host route of 32 x 32 pairs takes a minute)
                htimes[kind].append(wall(lambda: host_route(kind)))
    for kind in kinds if not args.timing_only else ():
        kernel(kind)
        torch.cuda.synchronize()
        rpost, rconf, rhyp, rmatch = host[kind]
        assert np.array_equal(out[3].cpu().numpy(), rmatch), f"js2t_nbest_confidence and the host route disagree on the votes ({kind})"
        err = float(np.max(np.abs(out[1].cpu().numpy().astype(np.float64) - rconf)))
        assert err <= 1e-4, f"js2t_nbest_confidence and the host route disagree: {err}"
        k, k0, m, h = (statistics.median(t[kind]) for t in (times, ntimes, mtimes, htimes))
        print(f"N {N:2d} P {P:2d} {kind:9s}: {B * P * (N - 1)} aligned pairs, workspace {need / 2**20:.1f} MiB; kernel {k:8.1f} us (min {min(times[kind]):.1f}, "
              f"max {max(times[kind]):.1f} over {args.rounds} rounds of {args.reps}), without `match` {k0:8.1f} us; js2t_mbr_rescore "
              f"({B * N * (N - 1) // 2} pairs) {m:8.1f} us (min {min(mtimes[kind]):.1f}, max {max(mtimes[kind]):.1f}); host route {h:9.1f} ms over "
              f"{len(htimes[kind])} runs = {h * 1e3 / k:.0f} x the kernel; votes equal, worst difference of conf {err:.1e}; mean conf of the "
              f"top pivot {float(rconf[:, 0][rmatch[:, 0].max(axis=1) > 0].mean()):.3f}", flush=True)
    for kind in kinds if args.timing_only else ():
        k, k0, m = (statistics.median(t[kind]) for t in (times, ntimes, mtimes))
        print(f"N {N:2d} P {P:2d} {kind:9s}: kernel {k:8.1f} us (min {min(times[kind]):.1f}, max {max(times[kind]):.1f}), without `match` {k0:8.1f} us; "
              f"js2t_mbr_rescore {m:8.1f} us", flush=True)
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


conf = dict(confidence=True, n_rescore=N)
decodes = [("ctc_beam_search beam 10", lambda: ctc_beam_search(model, batch(), beam_size=N, n_best=1)),
           ("ctc_beam_search beam 10, confidence", lambda: ctc_beam_search(model, batch(), beam_size=N, n_best=1, **conf)),
           ("ctc_attention_rescore beam 10", lambda: ctc_attention_rescore(model, batch(), beam_size=N, n_best=1, ctc_weight=0.3)),
           ("ctc_attention_rescore beam 10, confidence", lambda: ctc_attention_rescore(model, batch(), beam_size=N, n_best=1, ctc_weight=0.3, **conf))]
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
