"""GPU: the session objects of joeys2t_amd/streaming.py.  CTCStreamDecoder's finals against ctc_search's stage chain over a
hand-made list of the same segments (bits); StreamingTranscriber's pushed rows against long_form.stitch_posteriors(batch_size=1) on
the golden toy model (bits), its front end fed in pieces against the front end run once (bits), and its finals against one push
of the whole stream."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ctc_stream_reference as S

pytestmark = pytest.mark.gpu

BLANK = S.BLANK
RULE = dict(min_silence=S.RULE["min_silence"], silence_threshold=0.9, max_segment=S.RULE["max_len"])


def bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def stub_model():
    """what the decoder takes of a model: the special indices, the target vocabulary, the encoder's stride; and tiny_lm.arpa over it"""
    from joeys2t_amd.lm import NGramLM
    from joeys2t_amd.vocabulary import Vocabulary
    vocab = Vocabulary(list("abcdefgh"))  # 4 specials + 8: the 12 ids of the logits
    lm = NGramLM.from_arpa(Path(__file__).resolve().parent / "golden" / "tiny_lm.arpa", vocab, device="cuda:0")
    return SimpleNamespace(bos_index=BLANK, pad_index=1, eos_index=3, trg_vocab=vocab, encoder=SimpleNamespace()), lm


def same_records(got, want, parts=()):
    assert [(r["start_frame"], r["end_frame"]) for r in got] == [(r["start_frame"], r["end_frame"]) for r in want]
    for a, b in zip(got, want):
        assert [y.tolist() for y in a["ids"]] == [y.tolist() for y in b["ids"]] and np.array_equal(bits(a["scores"]), bits(b["scores"]))
        assert abs(a["start"] - b["start"]) < 1e-9 and abs(a["end"] - b["end"]) < 1e-9
        for key in parts:
            x, y = a["parts"][key], b["parts"][key]
            if key == "token_confidence":  # (as wide as the longest row of the call that made it)
                w = min(x.shape[1], y.shape[1])
                assert not x[:, w:].any() and not y[:, w:].any()
                x, y = x[:, :w], y[:, :w]
            assert np.array_equal(bits(x), bits(y)), key


@pytest.mark.parametrize("options,parts", [
    (dict(decision="mbr", confidence=True), ("risk", "posterior", "map_rank", "token_confidence", "confidence")),
    (dict(lm_weight=0.5, length_bonus=0.25, lm_fusion="rescore", return_parts=True), ("map_rank", )),
    (dict(lm_weight=0.5, length_bonus=0.25, lm_fusion="search"), ()),
])
def test_decoder_finals_are_the_stage_chain_over_the_hand_made_list(device, options, parts):
    from joeys2t_amd import ctc_search, long_form, ops
    from joeys2t_amd.streaming import CTCStreamDecoder
    model, lm = stub_model()
    if "lm_weight" in options:
        options = dict(options, lm=lm)
    K, nb, C = 6, 3, 5
    x = torch.from_numpy(S.stream_case("b")).to(device)
    dec = CTCStreamDecoder(model, 1, beam_size=K, n_best=nb, candidates=C, device=device, max_finals=1, **RULE, **options)
    got = []
    for a in range(0, x.shape[0], 50):
        (finals, ), (partial, ) = dec.push([x[a:a + 50]])
        got += finals
        assert 0 <= partial["stable"] <= len(partial["ids"]) and (partial["start_frame"] >= 0 or len(partial["ids"]) == 0)
    (finals, ), (partial, ) = dec.flush(0)
    got += finals
    assert partial["start_frame"] == -1 and dec.flush(0)[0] == [[]]
    assert dec.launches > -(-x.shape[0] // 50) + 2  # max_finals = 1: a push with a final inside took more than one step
    # by hand: the reference's segments as packed rows through the one-shot search and the same stages
    segs = S.segments(S.stream_reference("b", "k6"))
    assert [(r["start_frame"], r["end_frame"], r["why"]) for r in got] == [(a, b, {1: "endpoint", 2: "forced", 3: "flushed"}[w]) for a, b, w in segs]
    opt, return_parts, K, nb, N = long_form._options(options, K, nb)
    seg = torch.tensor([a for a, _, _ in segs] + [segs[-1][1]], dtype=torch.int32, device=device)
    pack = ops.PackedRows(seg, len(segs), max(b - a for a, b, _ in segs), x.shape[0])
    in_len = torch.tensor([b - a for a, b, _ in segs], dtype=torch.int64, device=device)
    with torch.no_grad():
        lst = ctc_search._search(model, x, in_len, pack, K, N, C, opt)
        ids, scores, n, *extra = ctc_search.ctc_stages(model, lst, opt, nb, return_parts)
    want = []
    for b, (a, e, _) in enumerate(segs):
        rows = slice(b * nb, (b + 1) * nb)
        rec = {"start": a * dec.sec, "end": e * dec.sec, "start_frame": a, "end_frame": e, "ids": [ids[r, :n[r]] for r in range(rows.start, rows.stop)],
               "scores": scores[rows, 0]}
        if extra:
            rec["parts"] = {k: v[rows] for k, v in extra[0].items()}
        want.append(rec)
    same_records(got, want, parts)
    # a reset stream decodes the same again; another stream of the same decoder is not touched by it
    dec.reset(0)
    (again, ), _ = dec.push([x[:120]])
    same_records(again, want[:len(again)], parts)
    assert len(again) >= 2


def test_several_streams_and_refusals(device):
    import joeys2t_amd
    model, _ = stub_model()
    with pytest.raises(ValueError, match="ctc_weight"):
        joeys2t_amd.CTCStreamDecoder(model, 1, device=device, ctc_weight=0.3)
    with pytest.raises(ValueError, match="silence_threshold"):
        joeys2t_amd.CTCStreamDecoder(model, 1, device=device, silence_threshold=1.5)
    with pytest.raises(ValueError, match="at least 1"):
        joeys2t_amd.CTCStreamDecoder(model, 0, device=device)
    dec = joeys2t_amd.CTCStreamDecoder(model, 3, beam_size=6, n_best=3, candidates=5, device=device, **RULE)
    with pytest.raises(ValueError, match="3 streams"):
        dec.push([None])
    xs = [torch.from_numpy(S.stream_case(name)).to(device) for name in ("a", "b", "c")]
    got = [[] for _ in xs]
    for a in range(0, 300, 64):  # streams of different lengths: the short ones run dry (None) while the long one goes on
        finals, _ = dec.push([x[a:a + 64] if a < x.shape[0] else None for x in xs])
        for g, f in zip(got, finals):
            g += f
    for b in range(3):
        got[b] += dec.flush(b)[0][b]
    for b, name in enumerate(("a", "b", "c")):
        segs = S.segments(S.stream_reference(name, "k6"))
        assert [(r["start_frame"], r["end_frame"]) for r in got[b]] == [(a, e) for a, e, _ in segs]
        one = joeys2t_amd.CTCStreamDecoder(model, 1, beam_size=6, n_best=3, candidates=5, device=device, max_finals=16, **RULE)
        (alone, ), _ = one.push([xs[b]])
        alone += one.flush(0)[0][0]
        same_records(got[b], alone)


# ---------------------------------------------------------------- a golden toy model: 8 feature channels, stride 4, 20 ids
@pytest.fixture(scope="module")
def golden_model(device):
    from test_hip_model import build
    model, g = build("model_pre", device)
    model.eval()
    return model, g


WINDOWS = dict(window=32, overlap=8)  # hop 16: windows at 0, 16, 32, ...


@pytest.fixture(scope="module")
def stitched(device, golden_model):
    """long_form.stitch_posteriors(batch_size=1) of the test's recordings, once: do not modify"""
    from joeys2t_amd import long_form
    model, _ = golden_model
    feat = np.random.RandomState(11).randn(101, 8).astype(np.float32)
    return feat, {n: long_form.stitch_posteriors(model, feat[:n], batch_size=1, **WINDOWS) for n in (20, 96, 101)}


# 96 = 64 + 32: the last complete window is the plan's last; 101: a short sixth window follows; 20: shorter than one window
@pytest.mark.parametrize("n_frames", [20, 96, 101])
@pytest.mark.parametrize("piece", [1, 37, 400])
def test_transcriber_pushes_the_rows_of_stitch_posteriors(device, golden_model, stitched, n_frames, piece):
    from joeys2t_amd.streaming import StreamingTranscriber
    model, _ = golden_model
    feat, want = stitched
    tr = StreamingTranscriber(model, keep_rows=True, beam_size=4, **WINDOWS)
    for a in range(0, n_frames, piece):
        tr.feed(feat[a:min(a + piece, n_frames)])
        assert sum(r[0].shape[0] for r in tr.rows) == (0 if tr._w == 0 else 2 + 4 * tr._w)  # window w is pushed when frame 16 w + 31 is in
    tr.finish()
    assert sum(r[0].shape[0] for r in tr.rows) == -(-n_frames // 4)
    for k, w in enumerate(want[n_frames]):
        got = torch.cat([r[k] for r in tr.rows]).cpu().numpy()
        assert np.array_equal(bits(got), bits(w.cpu().numpy())), k


def test_waveform_fed_in_pieces_gives_the_features_of_the_whole_waveform(device, golden_model):
    from joeys2t_amd import long_form
    from joeys2t_amd.helpers_for_audio import get_extractor
    from joeys2t_amd.streaming import StreamingTranscriber
    model, _ = golden_model
    wave = torch.from_numpy((np.random.RandomState(5).randn(16000 + 77) * 0.1).astype(np.float32))  # 98 frames of 8 mel bins, 237 samples over
    whole, _, frames = get_extractor(device, 16000, 8).batch(wave.to(device), [wave.numel()], [0])
    assert frames == [98]
    want = long_form.stitch_posteriors(model, wave, n_mel_bins=8, batch_size=1, **WINDOWS)
    for piece in (1000, 333, 160, 16077):
        tr = StreamingTranscriber(model, keep_rows=True, n_mel_bins=8, beam_size=4, **WINDOWS)
        for a in range(0, wave.numel(), piece):
            tr.feed(wave[a:a + piece])
        tr.finish()
        got = torch.cat(tr.features)
        assert got.shape == whole.shape
        diff = float((got - whole).abs().max())
        print(f"pieces of {piece} samples: {got.shape[0]} frames, largest |difference| to the front end run once {diff:g}")
        assert np.array_equal(bits(got.cpu().numpy()), bits(whole.cpu().numpy()))
        for k, w in enumerate(want):
            assert np.array_equal(bits(torch.cat([r[k] for r in tr.rows]).cpu().numpy()), bits(w.cpu().numpy())), (piece, k)
    with pytest.raises(ValueError, match="after waveform samples"):
        tr.feed(np.zeros((3, 8), dtype=np.float32))
    rows = StreamingTranscriber(model, beam_size=4, **WINDOWS)
    rows.feed(np.zeros((3, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="one kind per session"):
        rows.feed(np.zeros(100, dtype=np.float32))


def test_transcriber_finals_equal_one_push_of_the_whole_stream(device, golden_model, stitched):
    from joeys2t_amd.streaming import CTCStreamDecoder, StreamingTranscriber
    model, _ = golden_model
    feat, want = stitched
    rule = dict(min_silence=1, silence_threshold=0.05, max_segment=7, beam_size=4, n_best=2)
    dec = CTCStreamDecoder(model, 1, max_finals=32, **rule)
    (whole, ), _ = dec.push([want[101]])
    whole += dec.flush(0)[0][0]
    assert len(whole) >= 3 and max(r["end_frame"] - r["start_frame"] for r in whole) <= 7 and whole[-1]["end_frame"] <= 26
    assert all(abs(r["end"] - r["end_frame"] * 0.04) < 1e-9 for r in whole)  # 40 ms per encoder frame
    tr = StreamingTranscriber(model, **rule, **WINDOWS)
    got = []
    for a in range(0, 101, 13):
        finals, partial = tr.feed(feat[a:min(a + 13, 101)])
        got += finals
        assert 0 <= partial["stable"] <= len(partial["ids"])
    got += tr.finish()
    same_records(got, whole)
    assert [r["why"] for r in got] == [r["why"] for r in whole]
    tr.reset()  # a second session in the same object
    again = []
    for a in range(0, 101, 50):
        again += tr.feed(feat[a:min(a + 50, 101)])[0]
    same_records(again + tr.finish(), whole)
