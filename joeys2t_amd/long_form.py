"""Long-form transcription (EXTENSION; the reference and every decoder here take utterances): one RECORDING - a meeting, a lecture,
an hour of radio - through the CTC head.

The usual long-form CTC scheme, in three device steps and then the decoders that were there already:
  1. `stitch_posteriors`: features once for the recording; overlapping windows of it are encoded `batch_size` at a time; of every
     window only the centre frames are kept (a frame near a window's edge lacks context) and the kept frames, back to back, are one
     frame-synchronous posterior stream (js2t_ctc_stitch: the f32 rows and their lse / arg-max / blank log-probability, each logit
     read once);
  2. `segment`: the stream is cut where the model itself says nothing is spoken - long runs of confident blanks - and, where speech
     goes on for too long, at the last silent frame in reach (js2t_ctc_segment, whose header comment is the rule);
  3. the segments are packed rows with offsets, i.e. a ragged batch: `ctc_search._search` and the n-best stage chain decode them in
     parallel, one block per segment, with the options `ctc_beam_search` has.

Frame arithmetic.  `window` and `overlap` are FEATURE frames (10 ms), both multiples of the encoder's total stride s = 2^n_layers;
hop = window - 2 * overlap.  Window w starts at feature frame w * hop, and its encoder frame j is the recording's frame w * hop / s + j:
the windows lie on the stride grid, so no frame is interpolated.  The first window keeps from its first frame, the last to its last,
every other one its frames overlap / s .. (overlap + hop) / s - 1: every encoder frame of the recording is kept exactly once.

What is approximate.  A kept frame has seen at least `overlap` feature frames of context on either side (less only at the ends of
the recording), not the whole recording; self-attention inside a window, CMVN statistics per window.  Whether that costs accuracy on
a trained model has not been measured.  Memory: the stitched stream is T * V * 4 bytes (js2t_ctc_stitch states it).
`min_silence`, `margin` and `max_segment` are ENCODER frames (`alignment.frame_seconds` each)."""
import math
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from joeys2t_amd import ops

WHO = "transcribe_long"
INT32_MAX = 2**31 - 1


class WindowPlan(NamedTuple):
    """`plan_windows`' result, host integers: per window its first feature frame and its feature frames (the last window may be
    shorter), js2t_ctc_stitch's keep_lo / keep_hi / out_row in encoder frames, and `rows`, the encoder frames of the recording."""
    start: List[int]
    length: List[int]
    keep_lo: List[int]
    keep_hi: List[int]
    out_row: List[int]
    rows: int


def plan_windows(n_frames: int, window: int, overlap: int, subsample: int) -> WindowPlan:
    """The windows of a recording of `n_frames` feature frames (module docstring: the frame arithmetic).  Host arithmetic only.
    Refused (ValueError): n_frames < 1, subsample < 1, window or overlap no multiple of subsample, overlap < 0, hop =
    window - 2 * overlap < 1."""
    n_frames, window, overlap, s = int(n_frames), int(window), int(overlap), int(subsample)
    if n_frames < 1 or s < 1:
        raise ValueError(f"{WHO}: {n_frames} feature frames at a stride of {s}: both at least 1 expected")
    if window < 1 or overlap < 0 or window % s or overlap % s:
        raise ValueError(f"{WHO}: window {window} and overlap {overlap} must be multiples of the encoder's stride {s} (window > 0, overlap >= 0)")
    hop = window - 2 * overlap
    if hop < 1:
        raise ValueError(f"{WHO}: window {window} - 2 * overlap {overlap} leaves a hop of {hop}: at least {s} expected")
    T, S, o, h = -(-n_frames // s), window // s, overlap // s, hop // s
    W = 1 if T <= S else -(-(T - S) // h) + 1  # the fewest windows that reach the end: the last one then has more than 2 o frames
    start = [w * hop for w in range(W)]
    length = [min(window, n_frames - st) for st in start]
    keep_lo = [0 if w == 0 else o for w in range(W)]
    keep_hi = [min(S, T - w * h) if w == W - 1 else o + h for w in range(W)]
    out_row = [w * h + lo for w, lo in enumerate(keep_lo)]
    return WindowPlan(start, length, keep_lo, keep_hi, out_row, T)


def _stride(model) -> int:
    sub = getattr(model.encoder, "subsampler", None)
    return 2 ** sub.n_layers if sub is not None else 1


def _features(model, audio, sample_rate, n_mel_bins):
    """f32 [n_frames, F] on the model's device: a 1-d waveform through FbankExtractor, 2-d features as they are"""
    dev = next(model.parameters()).device
    audio = torch.as_tensor(audio)
    if audio.dim() == 2:
        return audio.to(dev, torch.float32).contiguous()
    if audio.dim() != 1:
        raise ValueError(f"{WHO}: a waveform [samples] or features [frames, F] expected, got {tuple(audio.shape)}")
    from joeys2t_amd.helpers_for_audio import get_extractor
    wave = audio.to(dev, torch.float32).contiguous()
    feat, _, _ = get_extractor(dev, sample_rate, n_mel_bins).batch(wave, [wave.numel()], [0])
    return feat


def stitch_posteriors(model, audio, *, window: int, overlap: int, batch_size: int = 8, cmvn=None, sample_rate: int = 16000,
                      n_mel_bins: int = 80):
    """Step 1.  audio: a waveform f32 [samples] (features by helpers_for_audio.FbankExtractor, once for the recording) or the
    features [n_frames, F] themselves.  cmvn: the data_augmentation.CMVN of the model's data config (SpeechProcessor.cmvn) or None;
    the statistics are taken per window (`finalize_features`).  Returns (logits f32 [T, V], lse f32 [T], argmax i64 [T], blank_lp
    f32 [T]) on the device, T = ceil(n_frames / stride); blank = model.bos_index."""
    if int(batch_size) < 1:
        raise ValueError(f"{WHO}: batch_size {batch_size} below 1")
    s = _stride(model)
    plan_windows(1, window, overlap, s)  # (the refusals of the window arithmetic, before the model or the device is touched)
    sub = getattr(model.encoder, "subsampler", None)
    with torch.no_grad():
        feat = _features(model, audio, sample_rate, n_mel_bins)
        if feat.shape[0] < 1:
            raise ValueError(f"{WHO}: the recording is shorter than one feature frame")
        plan = plan_windows(feat.shape[0], window, overlap, s)
        if sub is not None and any(sub.out_len(n) != -(-n // s) for n in set(plan.length)):
            raise ValueError(f"{WHO}: the subsampler's lengths are not ceil(n / {s}): its kernel sizes are not supported")
        dev = feat.device
        lo, hi, row = (torch.tensor(v, dtype=torch.int32, device=dev) for v in (plan.keep_lo, plan.keep_hi, plan.out_row))
        out = None
        for a in range(0, len(plan.start), int(batch_size)):
            b = min(a + int(batch_size), len(plan.start))
            ctc_out = encode_windows(model, feat, plan.start[a:b], plan.length[a:b], cmvn, s)
            out = ops.ctc_stitch(ctc_out, lo[a:b], hi[a:b], row[a:b], model.bos_index, rows=plan.rows, out=out)
    return out


def encode_windows(model, feat, start, frames, cmvn, s):
    """The CTC logits [len(start), max(frames) / s, V] of the windows feat[st : st + n] encoded as ONE batch, CMVN per window: what
    `stitch_posteriors` runs per batch of windows and streaming.StreamingTranscriber per window as it completes (inside the caller's
    no_grad).  start / frames: host lists, feature frames."""
    from joeys2t_amd.alignment import _ctc_frames
    from joeys2t_amd.batch import Batch
    from joeys2t_amd.data_augmentation import finalize_features
    dev = feat.device
    chunk = torch.cat([feat[st:st + n] for st, n in zip(start, frames)])  # (overlapping windows: ragged, back to back)
    off = torch.tensor(np.concatenate([[0], np.cumsum(frames)]), dtype=torch.int64, device=dev)
    src, _ = finalize_features(chunk, off, frames, cmvn=cmvn, specaugment=None)
    batch = Batch(src=src, src_length=torch.tensor(frames, dtype=torch.int64), src_prompt_mask=None, trg=None, trg_length=None,
                  trg_prompt_mask=None, indices=torch.arange(len(start)), device=dev, pad_index=model.pad_index,
                  eos_index=model.eos_index, is_train=False, task="S2T", n_gpu=1)
    ctc_out, _, _ = _ctc_frames(model, batch, who=WHO, want_lse=False)
    if ctc_out.shape[1] != -(-max(frames) // s):
        raise ValueError(f"{WHO}: {ctc_out.shape[1]} encoder frames for windows of {max(frames)} feature frames at stride {s}")
    return ctc_out


def _threshold(silence_threshold) -> float:
    threshold = float(silence_threshold)
    if not 0.0 < threshold <= 1.0:  # (a NaN fails too)
        raise ValueError(f"{WHO}: silence_threshold {threshold} outside (0, 1] (a probability of the blank)")
    return threshold


def _frames_arg(name, v, least):
    v = int(v)
    if v < least:
        raise ValueError(f"{WHO}: {name} {v} below {least} (encoder frames)")
    return min(v, INT32_MAX)


def segment(blank_lp, argmax, *, blank: int, min_silence: Optional[int] = None, silence_threshold: float = 0.9, margin: int = 0,
            max_segment: Optional[int] = None):
    """Step 2.  blank_lp / argmax: `stitch_posteriors`'.  A frame is silent when the blank is its arg-max with a probability of at
    least silence_threshold (in (0, 1]); min_silence (None: no pause is long enough), margin and max_segment (None: never cut) are
    encoder frames; js2t_ctc_segment states the rule.  Returns (ops.PackedRows over the stream's rows, seg_len i64 [B] on the device)
    with ONE host read, the number of segments.  Both None: no segmentation - the whole recording is one utterance, silent or not."""
    T = blank_lp.numel()
    dev = blank_lp.device
    threshold = _threshold(silence_threshold)
    margin = _frames_arg("margin", margin, 0)
    if min_silence is None and max_segment is None:
        return (ops.PackedRows(torch.tensor([0, T], dtype=torch.int32, device=dev), 1, max(T, 1), T),
                torch.tensor([T], dtype=torch.int64, device=dev))
    min_silence = min(T + 1, INT32_MAX) if min_silence is None else _frames_arg("min_silence", min_silence, 1)
    max_len = min(max(T, 1), INT32_MAX) if max_segment is None else _frames_arg("max_segment", max_segment, 1)
    most = T // min_silence + T // (max_len // 2 + 1) + 2  # (js2t_ctc_segment: a forced piece is longer than max_len / 2)
    n_seg, seg_off, seg_len = ops.ctc_segment(blank_lp, argmax, blank, math.log(threshold), min_silence, margin, max_len, most)
    n = int(n_seg.item())  # the one host read
    if n < 0:
        raise ops.Js2tError(f"{WHO}: more than {most} segments")
    return ops.PackedRows(seg_off[:n + 1].contiguous(), n, max(min(max_len, T), 1), T), seg_len[:n].contiguous()


def _options(nbest_options, beam_size, n_best, who=WHO):
    """(NBestOptions, return_parts, beam_size, n_best, the slots to search for) of the options transcribe_long - and, under its own
    name `who`, streaming.CTCStreamDecoder - hands on; every refusal is a ValueError raised before the model is touched"""
    from joeys2t_amd import ctc_search
    o = dict(nbest_options)
    if "ctc_weight" in o:
        raise ValueError(f"{who}: attention rescoring (ctc_weight) is not available over a recording: the decoder is not handed packed "
                         "encoder rows (DESIGN 7), and a segment's frames come from several windows")
    return_parts, n_rescore = bool(o.pop("return_parts", False)), o.pop("n_rescore", None)
    known = dict(lm=None, lm_weight=0.0, length_bonus=0.0, lm_fusion="rescore", decision="map", mbr_scale=1.0, confidence=False,
                 confidence_scale=1.0, context=None, context_weight=0.0)
    if set(o) - set(known):
        raise ValueError(f"{who}: unknown options {sorted(set(o) - set(known))}")
    o = {**known, **o}
    opt = ctc_search.NBestOptions(who, o["lm"], o["lm_weight"], o["length_bonus"], o["lm_fusion"], o["decision"], o["mbr_scale"],
                                  o["confidence"], o["confidence_scale"], o["context"], o["context_weight"])
    return (opt, return_parts or opt.confidence, *ctc_search.nbest_slots(who, opt, beam_size, n_best, n_rescore))


def decode_stream(model, stream, *, min_silence: Optional[int] = None, silence_threshold: float = 0.9, margin: int = 0,
                  max_segment: Optional[int] = None, beam_size: int = 10, n_best: int = 1, candidates: int = 8, timestamps: bool = False,
                  frame_shift_ms: float = 10.0, **nbest_options):
    """Steps 2 and 3 - transcribe_long behind `stitch_posteriors`, whose result `stream` is: (logits f32 [T, V], lse, argmax,
    blank_lp).  Of the model it takes the special indices, the target vocabulary's size (with an lm) and the encoder's stride (for
    the seconds).  Arguments and result: transcribe_long's."""
    from joeys2t_amd import alignment, ctc_search
    opt, return_parts, beam_size, n_best, N = _options(nbest_options, beam_size, n_best)
    st, lse, am, blp = stream
    sec = alignment.frame_seconds(model, frame_shift_ms)
    with torch.no_grad():
        pack, seg_len = segment(blp, am, blank=model.bos_index, min_silence=min_silence, silence_threshold=silence_threshold, margin=margin,
                                max_segment=max_segment)
        if pack.B == 0:
            return []
        lst = ctc_search._search(model, st, seg_len, pack, beam_size, N, candidates, opt)
        ids, scores, n, *parts = ctc_search.ctc_stages(model, lst, opt, n_best, return_parts)
        first = pack.seg.cpu().numpy()[:-1].astype(np.int64)
        length = seg_len.cpu().numpy()
        als = None
        if timestamps:
            trg = torch.from_numpy(np.ascontiguousarray(ids[::n_best])).to(st.device)
            trg_len = torch.from_numpy(np.ascontiguousarray(n[::n_best])).to(st.device)
            _, tok_start, tok_end, frame_logp, score = ops.ctc_align(st, lse, trg, seg_len, trg_len, int(model.bos_index), pack=pack)
            als = alignment.alignments(ids[::n_best], n[::n_best], tok_start, tok_end, frame_logp, score, sec, first_frame=first)
    out = []
    for b in range(pack.B):
        rows = slice(b * n_best, (b + 1) * n_best)
        rec = {"start": float(first[b] * sec), "end": float((first[b] + length[b]) * sec), "start_frame": int(first[b]),
               "end_frame": int(first[b] + length[b]), "ids": [ids[r, :n[r]].copy() for r in range(rows.start, rows.stop)],
               "scores": scores[rows, 0].copy()}
        if parts:
            rec["parts"] = {k: v[rows] for k, v in parts[0].items()}
        if als is not None:
            rec["alignment"] = als[b]
        out.append(rec)
    return out


def transcribe_long(model, audio, *, window: int, overlap: int, batch_size: int = 8, min_silence: Optional[int] = None,
                    silence_threshold: float = 0.9, margin: int = 0, max_segment: Optional[int] = None, beam_size: int = 10,
                    n_best: int = 1, candidates: int = 8, timestamps: bool = False, cmvn=None, sample_rate: int = 16000,
                    n_mel_bins: int = 80, frame_shift_ms: float = 10.0, **nbest_options):
    """A recording to text: `stitch_posteriors` (audio, window, overlap, batch_size, cmvn, sample_rate, n_mel_bins), `segment`
    (min_silence, silence_threshold, margin, max_segment; the first and the last None: the recording is one utterance), then CTC
    prefix beam search and the n-best stage chain over the segments as a packed ragged batch - search.ctc_beam_search's beam_size /
    n_best / candidates and, in nbest_options, its lm / lm_weight / length_bonus / lm_fusion / n_rescore / context / context_weight /
    decision / mbr_scale / confidence / confidence_scale / return_parts, with the meaning and the refusals `NBestOptions` and that
    decoder state.  Attention rescoring (ctc_weight) is refused: the decoder is not handed packed encoder rows, and a segment has
    no encoder output of its own - its frames come from several windows.
    Returns one dict per segment, in time order: "start" / "end" (seconds, `alignment.frame_seconds` per encoder frame), "start_frame" /
    "end_frame", "ids" (a list of n_best i64 arrays, best first - by risk under decision="mbr"), "scores" f32 [n_best], and with
    return_parts or confidence "parts", the decoder's parts dict cut to the segment's rows.  timestamps=True: also "alignment", the
    alignment.Alignment of the segment's first hypothesis (js2t_ctc_align over the packed rows), frames and seconds counted from the
    start of the RECORDING."""
    _options(nbest_options, beam_size, n_best)  # (the refusals, before the model is touched)
    plan_windows(1, window, overlap, _stride(model))
    _threshold(silence_threshold)
    stream = stitch_posteriors(model, audio, window=window, overlap=overlap, batch_size=batch_size, cmvn=cmvn, sample_rate=sample_rate,
                               n_mel_bins=n_mel_bins)
    return decode_stream(model, stream, min_silence=min_silence, silence_threshold=silence_threshold, margin=margin, max_segment=max_segment,
                         beam_size=beam_size, n_best=n_best, candidates=candidates, timestamps=timestamps, frame_shift_ms=frame_shift_ms,
                         **nbest_options)


def align_long(model, audio, tokens, *, window: int, overlap: int, batch_size: int = 8, cmvn=None, sample_rate: int = 16000,
               n_mel_bins: int = 80, free_start: bool = True, free_end: bool = True, frame_shift_ms: float = 10.0, utterances=None):
    """A recording and its transcript to timestamps: `stitch_posteriors` (audio, window, overlap, batch_size, cmvn, sample_rate,
    n_mel_bins), then `alignment.align_stream` - js2t_ctc_align_long over the whole stream, blank = model.bos_index.  tokens: the
    transcript's token ids, a 1-d integer sequence of any length the kernel's header allows.  free_start / free_end (default on): the
    recording may begin / end with audio the text lacks; the header of js2t_ctc_align_long states what that does to the first and
    last token's span.  Returns the alignment.Alignment of the recording (seconds: `alignment.frame_seconds` per encoder frame;
    `alignment.word_segments` works on it unchanged); with utterances = the token count of every sentence of the transcript, the
    pair (Alignment, `alignment.utterance_spans` of it).  Raises ValueError for a model without a CTC layer and for tokens that
    are not a 1-d integer sequence.  Not measured, not claimed: the accuracy of the timestamps on a trained model, and what the
    window stitching does to them."""
    from joeys2t_amd import alignment
    who = "align_long"
    if getattr(model.decoder, "ctc_output_layer", None) is None:
        raise ValueError(f"{who}: the model has no CTC output layer (loss: crossentropy-ctc)")
    ids = alignment._token_ids(tokens, who)
    if utterances is not None and sum(int(n) for n in utterances) != ids.size:
        raise ValueError(f"{who}: utterances sum to {sum(int(n) for n in utterances)} tokens, {ids.size} given")
    plan_windows(1, window, overlap, _stride(model))
    stream = stitch_posteriors(model, audio, window=window, overlap=overlap, batch_size=batch_size, cmvn=cmvn, sample_rate=sample_rate,
                               n_mel_bins=n_mel_bins)
    al = alignment.align_stream(stream, ids, int(model.bos_index), alignment.frame_seconds(model, frame_shift_ms), free_start=free_start,
                                free_end=free_end)
    if utterances is None:
        return al
    return al, alignment.utterance_spans(al, utterances)


def spot_long(model, audio, phrases, *, window: int, overlap: int, batch_size: int = 8, cmvn=None, sample_rate: int = 16000,
              n_mel_bins: int = 80, threshold: float = 0.5, max_hits: int = 64, frame_shift_ms: float = 10.0):
    """Where in a recording are these phrases said: `stitch_posteriors` (audio, window, overlap, batch_size, cmvn, sample_rate,
    n_mel_bins), then `spotting.find_phrases` - js2t_ctc_spot over the whole stream, blank = model.bos_index.  phrases: a list of 1-d
    integer sequences of 1 .. 32 token ids (`spotting.phrases_from_text` makes them from pieces); threshold and max_hits:
    find_phrases'.  Returns the list of spotting.PhraseHit sorted by (start_frame, phrase), frames and seconds
    (`alignment.frame_seconds` per encoder frame) counted from the start of the recording.  Raises ValueError for a model without
    a CTC layer and for what find_phrases refuses, before the model runs.  Not measured, not claimed: detection accuracy or false-alarm
    rate on a trained model, and what the window stitching does to them."""
    from joeys2t_amd import alignment, spotting
    who = "spot_long"
    if getattr(model.decoder, "ctc_output_layer", None) is None:
        raise ValueError(f"{who}: the model has no CTC output layer (loss: crossentropy-ctc)")
    spotting._phrase_ids(phrases, 32)  # (the refusals, before the model is touched)
    spotting._log_threshold(threshold)
    if int(max_hits) < 1:
        raise ValueError(f"{who}: max_hits {max_hits} below 1")
    plan_windows(1, window, overlap, _stride(model))
    stream = stitch_posteriors(model, audio, window=window, overlap=overlap, batch_size=batch_size, cmvn=cmvn, sample_rate=sample_rate,
                               n_mel_bins=n_mel_bins)
    return spotting.find_phrases(stream, phrases, int(model.bos_index), alignment.frame_seconds(model, frame_shift_ms), threshold=threshold,
                                 max_hits=max_hits)
