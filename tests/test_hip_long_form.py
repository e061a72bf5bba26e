"""GPU: long-form CTC - js2t_ctc_stitch and js2t_ctc_segment against tests/long_form_reference.py (pinned on the CPU by
test_long_form_cpu.py), the packed route of joeys2t_amd.long_form against hand-built calls of the kernels it chains, the
concatenation property on a stream with exact pauses, and transcribe_long on a golden toy model.

Tolerances.  Copies, arg-max and every integer: exact.  lse: the BITS of ops.row_lse on the same f32 row (one reduction in one
order, csrc/row_lse.hpp), and within 1e-5 * max(1, |ref|) of the float64 value - hardware exp / log carry a relative error of about
1e-7 each, the sum of at most 1030 terms in f32 a relative 1030 * 6e-8 / 2 in the worst case, so 1e-5 has a factor of a few in hand.
blank_lp: one more f32 subtraction of values of magnitude <= ~20, the same bound.  Scores: bit equality between routes that
run the same kernels; 1e-4 * max(1, |score|), the project's budget for accumulated log-likelihoods, where two decodings differ."""
import functools
import math
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ctc_beam_reference as R
import long_form_reference as L
from test_long_form_cpu import SEGMENT_CASES, stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------- stitch
KEEP_LO, KEEP_HI, OUT_ROW, ROWS = [2, 3, 0], [5, 3, 7], [1, 4, 4], 12  # a centre range, an empty one, a full one; rows 0 and 11 free


def stitch_input(V, seed):
    """f32 [3, 7, V]: NaN outside the kept frames, a planted tie for the maximum in every kept frame"""
    rs = np.random.RandomState(seed)
    x = np.full((3, 7, V), np.nan, dtype=np.float32)
    for w in range(3):
        for j in range(KEEP_LO[w], KEEP_HI[w]):
            row = (rs.randn(V) * 3).astype(np.float32)
            a, b = sorted(rs.choice(V, 2, replace=False).tolist())
            row[a] = row[b] = np.float32(row.max() + 1.5)  # the first of the two is the arg-max
            x[w, j] = row
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [5, 64, 70, 257, 1030])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned_base", "shifted_base"])
def test_stitch_matches_reference(device, V, dtype, shift):
    from joeys2t_amd import ops
    x = torch.from_numpy(stitch_input(V, 11 * V + shift)).to(dtype)
    flat = torch.empty(x.numel() + 8, dtype=dtype, device=device)
    src = flat[shift:shift + x.numel()].view(3, 7, V)  # shift 1: no row of the source starts on a 16-byte boundary by design
    src.copy_(x)
    blank = V - 1 if shift else 0
    out_flat = torch.full((ROWS * V + 8, ), 7.0, dtype=torch.float32, device=device)
    out = (out_flat[3 * shift:3 * shift + ROWS * V].view(ROWS, V), torch.full((ROWS, ), 7.0, device=device),
           torch.full((ROWS, ), 7, dtype=torch.int64, device=device), torch.full((ROWS, ), 7.0, device=device))
    lo, hi, row = (torch.tensor(v, dtype=torch.int32, device=device) for v in (KEEP_LO, KEEP_HI, OUT_ROW))
    st, lse, am, blp = ops.ctc_stitch(src, lo, hi, row, blank, out=out)
    want_lse, _ = ops.row_lse(st[1:11].contiguous())
    torch.cuda.synchronize()
    ref_out, ref_lse, ref_am, ref_blp, written = L.stitch(x.float().numpy(), KEEP_LO, KEEP_HI, OUT_ROW, ROWS, blank)
    assert written.tolist() == [False] + [True] * 10 + [False]
    st, lse, am, blp = st.cpu().numpy(), lse.cpu().numpy(), am.cpu().numpy(), blp.cpu().numpy()
    for t in (st, lse, blp):
        assert not np.isnan(t).any()
    assert np.array_equal(bits(st[written]), bits(ref_out[written].astype(np.float32)))  # copies bit-exact (bf16 widened)
    for free in (0, 11):  # rows no window writes keep their contents
        assert (st[free] == 7.0).all() and lse[free] == 7.0 and am[free] == 7 and blp[free] == 7.0
    assert np.array_equal(am[written], ref_am[written])
    assert np.array_equal(bits(lse[written]), bits(want_lse.cpu().numpy()))
    err_lse = np.abs(lse[written] - ref_lse[written]) / np.maximum(1.0, np.abs(ref_lse[written]))
    err_blp = np.abs(blp[written] - ref_blp[written]) / np.maximum(1.0, np.abs(ref_blp[written]))
    print(f"V {V} {dtype} shift {shift}: lse err / 1e-5 {err_lse.max() / 1e-5:.4f}, blank_lp err / 1e-5 {err_blp.max() / 1e-5:.4f}")
    assert err_lse.max() <= 1e-5 and err_blp.max() <= 1e-5
    assert np.array_equal(bits(blp[written]), bits((st[written, blank] - lse[written]).astype(np.float32)))


def test_stitch_alone_and_in_a_batch_give_the_same_bits(device):
    from joeys2t_amd import ops
    for V in (70, 1030):
        x = torch.from_numpy(stitch_input(V, 5)).to(device)
        lo, hi, row = (torch.tensor(v, dtype=torch.int32, device=device) for v in (KEEP_LO, KEEP_HI, OUT_ROW))
        both = ops.ctc_stitch(x, lo, hi, row, 0, rows=ROWS)
        alone = ops.ctc_stitch(x[2:3].contiguous(), lo[2:3].contiguous(), hi[2:3].contiguous(), row[2:3].contiguous(), 0, rows=ROWS)
        for a, b in zip(both, alone):
            assert np.array_equal(bits(a[4:11].cpu().numpy()), bits(b[4:11].cpu().numpy()))


def test_stitch_refusals(device):
    from joeys2t_amd import ops
    x = torch.zeros((1, 2, 8), device=device)
    one = torch.zeros((1, ), dtype=torch.int32, device=device)
    with pytest.raises(ops.Js2tError, match="blank"):
        ops.ctc_stitch(x, one, one, one, 8, rows=2)
    with pytest.raises(ops.Js2tError, match="12000"):
        ops.ctc_stitch(torch.zeros((1, 1, 12001), device=device), one, one, one, 0, rows=1)
    with pytest.raises(ops.Js2tError, match="int32"):
        ops.ctc_stitch(x, one.long(), one, one, 0, rows=2)
    with pytest.raises(ops.Js2tError, match="CPU tensor"):
        ops.ctc_stitch(x.cpu(), one, one, one, 0, rows=2)
    # a range beyond the window and a destination beyond the stream are clamped / skipped, not written out of bounds
    lo, hi, row = (torch.tensor([v], dtype=torch.int32, device=device) for v in (-3, 9, 1))
    st, lse, am, blp = ops.ctc_stitch(x, lo, hi, row, 0, out=(torch.full((2, 8), 7.0, device=device), torch.full((2, ), 7.0, device=device),
                                                               torch.full((2, ), 7, dtype=torch.int64, device=device),
                                                               torch.full((2, ), 7.0, device=device)))
    assert st[0].eq(7.0).all() and st[1].eq(0.0).all() and am.tolist() == [7, 0] and abs(lse[1].item() - math.log(8.0)) < 1e-6


# ---------------------------------------------------------------- segment
def run_segment(device, lp, am, thr, max_segments=None, **params):
    """[(start, end)] as the kernel gives them, or -1; checks seg_off's last entry on the way"""
    from joeys2t_amd import ops
    T = len(lp)
    if max_segments is None:
        max_segments = T // min(params["min_silence"], T + 1) + T // (min(params["max_len"], T + 1) // 2 + 1) + 2
    n_seg, seg_off, seg_len = ops.ctc_segment(torch.from_numpy(lp).to(device), torch.from_numpy(am).to(device), 0, thr, params["min_silence"],
                                              params["margin"], params["max_len"], max_segments)
    n = int(n_seg.item())
    if n < 0:
        return -1
    off, ln = seg_off.cpu().numpy(), seg_len.cpu().numpy()
    assert off[n] == (off[n - 1] + ln[n - 1] if n else 0)
    return [(int(off[i]), int(off[i] + ln[i])) for i in range(n)]


@pytest.mark.parametrize("name", list(SEGMENT_CASES))
def test_segment_hand_cases(device, name):
    marks, params, want = SEGMENT_CASES[name]
    lp, am = stream(marks)
    assert run_segment(device, lp, am, L.LOG09, **params) == want


@functools.lru_cache(maxsize=None)
def random_reference(seed, T):
    """the seeded stream and the reference's segments for every parameter set, computed once: do not modify"""
    lp, am = L.random_stream(seed, T)
    return lp, am, [L.segment(lp, am, 0, L.LOG09, **p) for p in L.PARAMS]


@pytest.mark.parametrize("T", [1, 63, 64, 65, 1024, 1025, 5000])
def test_segment_random_streams(device, T):
    for seed in (T, T + 7):
        lp, am, want = random_reference(seed, T)
        for p, w in zip(L.PARAMS, want):
            assert run_segment(device, lp, am, L.LOG09, **p) == w, (seed, p)
    lp, am = L.random_stream(T + 1, T, p_flip=0.5, p_nan=0.0)  # pauses and regions of a frame or two: more regions than one wave holds
    for p in L.PARAMS[:2]:
        assert run_segment(device, lp, am, L.LOG09, **p) == L.segment(lp, am, 0, L.LOG09, **p)


def test_segment_overflow_and_refusals(device):
    from joeys2t_amd import ops
    lp, am, want = random_reference(1024, 1024)
    n = len(want[1])
    assert n > 3
    assert run_segment(device, lp, am, L.LOG09, max_segments=n - 1, **L.PARAMS[1]) == -1
    assert run_segment(device, lp, am, L.LOG09, max_segments=0, **L.PARAMS[1]) == -1
    assert run_segment(device, lp, am, L.LOG09, max_segments=n, **L.PARAMS[1]) == want[1]
    t_lp, t_am = torch.from_numpy(lp).to(device), torch.from_numpy(am).to(device)
    for bad in (dict(min_silence=0), dict(margin=-1), dict(max_len=0), dict(max_segments=-1), dict(log_threshold=float("nan"))):
        kw = dict(log_threshold=L.LOG09, min_silence=2, margin=0, max_len=10, max_segments=100)
        kw.update(bad)
        with pytest.raises(ops.Js2tError, match="ctc_segment"):
            ops.ctc_segment(t_lp, t_am, 0, **kw)


# ---------------------------------------------------------------- the packed route
def stub_model(blank, vocab=None):
    """what decode_stream takes of a model: the special indices, the target vocabulary, the encoder's stride"""
    return SimpleNamespace(bos_index=blank, pad_index=1, eos_index=3, trg_vocab=vocab, encoder=SimpleNamespace())


def stitched(device, x):
    """[T, V] logits as stitch_posteriors would hand them on: one window kept whole"""
    from joeys2t_amd import ops
    T = x.shape[0]
    lo, hi = (torch.tensor([v], dtype=torch.int32, device=device) for v in (0, T))
    return ops.ctc_stitch(torch.from_numpy(x).to(device)[None].contiguous(), lo, hi, lo, ROUTE_BLANK, rows=T)


ROUTE_BLANK, ROUTE = 2, dict(min_silence=4, silence_threshold=0.9, margin=2, max_segment=40)
ROUTE_K, ROUTE_NB, ROUTE_C = 6, 3, 5


@functools.lru_cache(maxsize=None)
def route_case():
    """logits f32 [300, 12]: planted words of 20 .. 70 frames (some longer than max_segment) between pauses
    of 3 .. 9 confident blank frames (some shorter than min_silence).  Computed once: do not modify."""
    rs = np.random.RandomState(77)
    parts, T = [], 0
    while T < 300:
        word = R.planted_logits(1000 + len(parts), 1, int(rs.randint(20, 71)), 12, ROUTE_BLANK)[0]
        quiet = rs.randn(int(rs.randint(3, 10)), 12).astype(np.float32)
        quiet[:, ROUTE_BLANK] += 9.0
        parts += [word, quiet]
        T += len(word) + len(quiet)
    return np.concatenate(parts)[:300]


def route_lm():
    from joeys2t_amd.lm import NGramLM
    from joeys2t_amd.vocabulary import Vocabulary
    vocab = Vocabulary(list("abcdefgh"))  # 4 specials + 8: the 12 ids of the logits
    return vocab, NGramLM.from_arpa(Path(__file__).resolve().parent / "golden" / "tiny_lm.arpa", vocab, device=DEV)


def hand_pack(device, st, lp, am, **route):
    """the reference's segments of the stream as a hand-built PackedRows, their lengths, and the candidate tables of the rows"""
    from joeys2t_amd import ops
    segs = L.segment(lp, am, ROUTE_BLANK, float(np.float32(math.log(route["silence_threshold"]))), route["min_silence"], route["margin"],
                     route["max_segment"])
    joints = [c - b for (_, b), (c, _) in zip(segs, segs[1:])]
    assert len(segs) >= 4 and 0 in joints and max(joints) > 0 and max(b - a for a, b in segs) <= route["max_segment"]  # cuts and gaps
    seg = torch.tensor([a for a, _ in segs] + [segs[-1][1]], dtype=torch.int32, device=device)
    pack = ops.PackedRows(seg, len(segs), max(b - a for a, b in segs), st.shape[0])
    in_len = torch.tensor([b - a for a, b in segs], dtype=torch.int64, device=device)
    cand_id, cand_lp, lse = ops.ctc_beam_candidates(st, ROUTE_C, ROUTE_BLANK)
    return segs, pack, in_len, (st, lse, cand_id, cand_lp, in_len)


def check_records(recs, segs, ids, n, score, n_best):
    """decode_stream's records against [B, n_best, T] ids, lengths and scores of a hand-made call: the bits"""
    ids, n, score = ids.cpu().numpy(), n.cpu().numpy(), score.cpu().numpy()
    assert [(r["start_frame"], r["end_frame"]) for r in recs] == segs
    for b, r in enumerate(recs):
        assert len(r["ids"]) == n_best and np.array_equal(bits(r["scores"]), bits(score[b, :n_best]))
        for i in range(n_best):
            assert r["ids"][i].tolist() == ids[b, i, :n[b, i]].tolist()


def test_route_equivalence(device):
    from joeys2t_amd import long_form, ops
    vocab, lm = route_lm()
    model = stub_model(ROUTE_BLANK, vocab)
    stream_ = stitched(device, route_case())
    st, _, am, blp = stream_
    segs, pack, in_len, search = hand_pack(device, st, blp.cpu().numpy(), am.cpu().numpy(), **ROUTE)
    common = dict(beam_size=ROUTE_K, n_best=ROUTE_NB, candidates=ROUTE_C, **ROUTE)
    # plain
    ids, n, score = ops.ctc_beam_search(*search, ROUTE_K, ROUTE_NB, ROUTE_BLANK, model.pad_index, pack=pack)
    recs = long_form.decode_stream(model, stream_, **common)
    check_records(recs, segs, ids, n, score, ROUTE_NB)
    assert all(abs(r["start"] - r["start_frame"] * 0.01) < 1e-9 for r in recs)  # (no subsampler: 10 ms per frame)
    # the LM fused into the beam
    ids, n, score, _, _ = ops.ctc_beam_search_lm(*search, ROUTE_K, ROUTE_NB, ROUTE_BLANK, model.pad_index, lm, model.bos_index, model.eos_index,
                                                 0.5, 0.25, pack=pack)
    fused = long_form.decode_stream(model, stream_, lm=lm, lm_weight=0.5, length_bonus=0.25, lm_fusion="search", **common)
    check_records(fused, segs, ids, n, score, ROUTE_NB)
    assert any(a["ids"][0].tolist() != b["ids"][0].tolist() or a["scores"][0] != b["scores"][0] for a, b in zip(fused, recs))
    # confidence: the whole list of beam_size slots, the votes for the n_best first
    ids, n, score = ops.ctc_beam_search(*search, ROUTE_K, ROUTE_K, ROUTE_BLANK, model.pad_index, pack=pack)
    B = len(segs)
    pivot = torch.arange(ROUTE_NB, dtype=torch.int32, device=device).expand(B, ROUTE_NB).contiguous()
    Lp = min(pack.T + 1, ops.edit_max_len() + 1)
    _, conf, hyp = ops.nbest_confidence(ids, n.reshape(-1), score.reshape(-1), ROUTE_K, pivot, 1.0, Lp=Lp)
    with_conf = long_form.decode_stream(model, stream_, confidence=True, **common)
    check_records(with_conf, segs, ids, n, score, ROUTE_NB)
    conf, hyp = conf.cpu().numpy(), hyp.cpu().numpy()
    for b, r in enumerate(with_conf):
        width = r["parts"]["token_confidence"].shape[1]
        assert np.array_equal(bits(r["parts"]["token_confidence"][:, :min(width, Lp - 1)]), bits(conf[b, :, :width]))
        assert np.array_equal(bits(r["parts"]["confidence"]), bits(hyp[b]))
        assert np.array_equal(r["parts"]["map_rank"], np.arange(ROUTE_NB))


def test_route_timestamps_lie_in_their_segment(device):
    from joeys2t_amd import long_form
    model = stub_model(ROUTE_BLANK)
    recs = long_form.decode_stream(model, stitched(device, route_case()), beam_size=4, timestamps=True, **ROUTE)
    assert len(recs) >= 4 and sum(len(r["ids"][0]) for r in recs) > 20
    for r in recs:
        a = r["alignment"]
        assert a.tokens == r["ids"][0].tolist() and np.isfinite(a.score)
        assert all(r["start_frame"] <= s < e <= r["end_frame"] for s, e in zip(a.start_frame, a.end_frame))
        assert all(r["start"] - 1e-9 <= s < e <= r["end"] + 1e-9 for s, e in zip(a.start, a.end))
        assert a.start_frame == sorted(a.start_frame)


def test_concatenation(device):
    """pauses in which the blank has probability exactly 1: the segments' top-1 labellings concatenate to the top-1 of the stream
    decoded as one utterance and the scores add up (test_long_form_cpu.py: the float64 reference alone does, margin >= 4)"""
    from joeys2t_amd import long_form, ops
    c = L.CONCAT
    x, spans = L.concat_stream()
    want_y, want_s, _, want_ss, margin = L.concat_reference()
    assert margin >= R.DECIDABLE
    model = stub_model(R.BLANK)
    T = x.shape[0]
    lo, hi = (torch.tensor([v], dtype=torch.int32, device=device) for v in (0, T))
    stream_ = ops.ctc_stitch(torch.from_numpy(x).to(device)[None].contiguous(), lo, hi, lo, R.BLANK, rows=T)
    assert stream_[3].cpu().numpy()[:c["pause"]].tolist() == [0.0] * c["pause"]  # log 1, exactly
    kw = dict(beam_size=c["K"], n_best=1, candidates=c["C"])
    recs = long_form.decode_stream(model, stream_, min_silence=c["min_silence"], silence_threshold=1.0, **kw)
    whole, = long_form.decode_stream(model, stream_, **kw)  # no segmentation: one utterance
    assert [(r["start_frame"], r["end_frame"]) for r in recs] == spans and (whole["start_frame"], whole["end_frame"]) == (0, T)
    cat = [v for r in recs for v in r["ids"][0].tolist()]
    total = float(np.sum([np.float64(r["scores"][0]) for r in recs]))
    one = float(whole["scores"][0])
    print(f"summed {total:.8f} whole {one:.8f} reference {want_s:.8f}: |summed - whole| / tol {abs(total - one) / R.bound(one):.4f}, "
          f"|whole - ref| / tol {abs(one - want_s) / R.bound(want_s):.4f}")
    assert cat == whole["ids"][0].tolist() == list(want_y)
    assert abs(total - one) <= R.bound(one)
    assert abs(one - want_s) <= R.bound(want_s) and all(abs(float(r["scores"][0]) - s) <= R.bound(s) for r, s in zip(recs, want_ss))


# ---------------------------------------------------------------- a golden toy model
@pytest.fixture(scope="module")
def golden_model(device):
    from test_hip_model import build
    model, g = build("model_pre", device)
    model.eval()
    return model, g


def single_batch(model, feat, device):
    from joeys2t_amd.batch import Batch
    return Batch(src=torch.from_numpy(feat)[None], src_length=torch.tensor([feat.shape[0]]), src_prompt_mask=None, trg=None, trg_length=None,
                 trg_prompt_mask=None, indices=torch.arange(1), device=device, pad_index=model.pad_index, eos_index=model.eos_index,
                 is_train=False, task="S2T", n_gpu=1)


def test_recording_shorter_than_one_window_is_the_utterance_decoder(device, golden_model):
    import joeys2t_amd
    from joeys2t_amd.search import ctc_beam_search
    model, g = golden_model
    feat = np.ascontiguousarray(g["src"][0, :int(g["src_length"][0])])  # 37 feature frames of 8 channels
    K, nb = 6, 3
    for opts in (dict(), dict(length_bonus=0.5), dict(decision="mbr", return_parts=True)):
        ids, scores, n, *parts = ctc_beam_search(model, single_batch(model, feat, device), beam_size=K, n_best=nb, **opts)
        rec, = joeys2t_amd.transcribe_long(model, feat, window=40, overlap=8, beam_size=K, n_best=nb, **opts)
        assert (rec["start_frame"], rec["end_frame"]) == (0, 10) and abs(rec["end"] - 0.4) < 1e-9  # ceil(37 / 4) frames of 40 ms
        assert np.array_equal(bits(rec["scores"]), bits(scores[:, 0]))
        assert [y.tolist() for y in rec["ids"]] == [ids[i, :n[i]].tolist() for i in range(nb)]
        if parts:
            assert np.array_equal(bits(rec["parts"]["risk"]), bits(parts[0]["risk"]))


def test_waveform_goes_through_the_front_end_once(device, golden_model):
    """a waveform gives what its FbankExtractor features give, and CMVN per window is finalize_features' on that window"""
    from joeys2t_amd import long_form
    from joeys2t_amd.data_augmentation import CMVN, finalize_features
    from joeys2t_amd.helpers_for_audio import get_extractor
    model, _ = golden_model
    wave = torch.from_numpy((np.random.RandomState(5).randn(16000) * 0.1).astype(np.float32))  # 1 s: 98 frames of 8 mel bins
    feat, _, frames = get_extractor(device, 16000, 8).batch(wave.to(device), [wave.numel()], [0])
    assert frames == [98]
    kw = dict(window=32, overlap=8, batch_size=4)
    a = long_form.stitch_posteriors(model, wave, n_mel_bins=8, **kw)
    b = long_form.stitch_posteriors(model, feat, **kw)
    assert a[0].shape == (25, 20) and all(np.array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy())) for x, y in zip(a, b))
    cmvn = CMVN()
    c = long_form.stitch_posteriors(model, feat, cmvn=cmvn, **kw)
    assert not torch.equal(c[0], b[0])
    off = torch.tensor([0, 32], dtype=torch.int64, device=device)
    src, _ = finalize_features(feat[32:64].contiguous(), off, [32], cmvn=cmvn, specaugment=None)  # window 2 = feature frames 32 .. 63
    from joeys2t_amd.alignment import _ctc_frames
    with torch.no_grad():
        own, _, _ = _ctc_frames(model, single_batch(model, src[0].cpu().numpy(), device), want_lse=False)
    assert torch.allclose(own[0, 2:6].float(), c[0][10:14], rtol=1e-4, atol=1e-4)  # its kept frames 2 .. 5 are rows 2 * 4 + 2 ..


def test_recording_of_three_windows(device, golden_model):
    from joeys2t_amd import long_form
    model, _ = golden_model
    feat = np.random.RandomState(3).randn(96, 8).astype(np.float32)
    duration = 24 * 0.04
    st, lse, am, blp = long_form.stitch_posteriors(model, feat, window=32, overlap=8, batch_size=2)  # 5 windows in 3 batches
    assert st.shape == (24, 20) and not torch.isnan(st).any() and not torch.isnan(lse).any()
    # a window's kept frames are that window's own logits: window 1 = feature frames 16 .. 47 keeps its encoder frames 2 .. 5
    from joeys2t_amd.alignment import _ctc_frames
    with torch.no_grad():
        own, _, _ = _ctc_frames(model, single_batch(model, feat[16:48], device), want_lse=False)
    assert torch.allclose(own[0, 2:6].float(), st[6:10], rtol=1e-4, atol=1e-4)
    for seg in (dict(max_segment=7), dict(min_silence=1, silence_threshold=0.05, margin=1, max_segment=7), dict()):
        recs = long_form.transcribe_long(model, feat, window=32, overlap=8, batch_size=2, beam_size=4, n_best=2, timestamps=True, **seg)
        assert len(recs) >= (0 if "min_silence" in seg else 1)
        assert all(0.0 <= r["start"] < r["end"] <= duration + 1e-9 for r in recs)
        for r, nxt in zip(recs, recs[1:] + [None]):
            assert r["start_frame"] < r["end_frame"] and (nxt is None or r["end_frame"] <= nxt["start_frame"])
            assert r["end_frame"] - r["start_frame"] <= seg.get("max_segment", 24) and len(r["ids"]) == 2
            a = r["alignment"]
            if np.isfinite(a.score):
                assert all(r["start_frame"] <= s < e <= r["end_frame"] for s, e in zip(a.start_frame, a.end_frame))
        if not seg:
            assert [(r["start_frame"], r["end_frame"]) for r in recs] == [(0, 24)]


def test_transcribe_long_refusals(device, golden_model):
    import joeys2t_amd
    model, g = golden_model
    feat = np.ascontiguousarray(g["src"][0])
    with pytest.raises(ValueError, match="multiples of the encoder's stride 4"):
        joeys2t_amd.transcribe_long(model, feat, window=42, overlap=8)
    with pytest.raises(ValueError, match="hop"):
        joeys2t_amd.transcribe_long(model, feat, window=16, overlap=8)
    with pytest.raises(ValueError, match="packed encoder rows"):
        joeys2t_amd.transcribe_long(model, feat, window=40, overlap=8, ctc_weight=0.3)
    with pytest.raises(ValueError, match="silence_threshold"):
        joeys2t_amd.transcribe_long(model, feat, window=40, overlap=8, min_silence=2, silence_threshold=1.5)
