"""CTC forced alignment (EXTENSION; the reference has no aligner): WHEN was a token spoken?

Every S2T model trains an encoder-side CTC head (`decoder.ctc_output_layer`).  Its frame posteriors and a label sequence - the
reference text, or a hypothesis of `search` / `search.ctc_greedy` - determine a best path through the frames (js2t_ctc_align: the
Viterbi form of the CTC recursion with the back-trace in the same launch), and the path gives every token a span of encoder frames.

Seconds: encoder frame j is reported as starting at j * 2^(subsampler.n_layers) * frame_shift_ms / 1000, i.e. at the LEFT EDGE of
the stride grid of the convolutional subsampler (stride 2 per layer; 40 ms per encoder frame for two layers at the 10 ms shift of
helpers_for_audio.FbankExtractor).  The receptive field of a frame is wider than its stride and centred slightly differently; the
convention is stated rather than corrected for.  A token's `end` is the start of the first frame behind it.
"""
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

WORD_MARKER = "▁"  # sentence-piece: the piece opens a new word


@dataclass
class Alignment:
    """One utterance: per token its id, [start_frame, end_frame) in encoder frames, [start, end) in seconds and the mean
    log-probability of its frames; `score` is the log-probability of the whole best path (-inf: the labels do not fit the frames,
    and the per-token lists then carry -1 / nan)."""
    tokens: List[int]
    start_frame: List[int]
    end_frame: List[int]
    start: List[float]
    end: List[float]
    logp: List[float]
    score: float


def frame_seconds(model, frame_shift_ms: float = 10.0) -> float:
    """length of one encoder frame in seconds (see the module docstring for the convention)"""
    sub = getattr(model.encoder, "subsampler", None)
    return (2 ** (sub.n_layers if sub is not None else 0)) * frame_shift_ms / 1000.0


def _ctc_frames(model, batch, who: str = "forced_align", want_lse: bool = True, want_encoder: bool = False):
    """(ctc logits [B, T', V], lse [B * T'] or None, input lengths i64[B]) the way search.ctc_greedy obtains them; with want_encoder
    also the encoder output and its mask, for a caller that goes on to run the decoder on the same encoding"""
    from joeys2t_amd import ops
    layer = getattr(model.decoder, "ctc_output_layer", None)
    if layer is None:
        raise ValueError(f"{who}: the model has no CTC output layer (loss: crossentropy-ctc)")
    encoder_output, _, src_mask, _ = model(return_type="encode", **vars(batch))
    ctc_out = model.decoder.project(layer, encoder_output, model.runtime.compute_dtype).contiguous()  # [B, T', V]
    B, T, V = ctc_out.shape
    lse = ops.row_lse(ctc_out.view(B * T, V))[0] if want_lse else None
    in_len = src_mask.squeeze(1).sum(dim=1).to(torch.int64).contiguous()
    if want_encoder:
        return ctc_out, lse, in_len, encoder_output, src_mask
    return ctc_out, lse, in_len


def forced_align(model, batch, trg=None, trg_length=None, frame_shift_ms: float = 10.0) -> List[Alignment]:
    """Align `trg` / `trg_length` (default: batch.trg / batch.trg_length - what the CTC loss is trained on) to the utterances of
    `batch`, blank = model.bos_index.  One Alignment per utterance, in the batch's row order.  Raises ValueError for a model
    without a CTC layer."""
    from joeys2t_amd import ops
    with torch.no_grad():
        ctc_out, lse, in_len = _ctc_frames(model, batch)
        dev = ctc_out.device
        trg = batch.trg if trg is None else trg
        trg_length = batch.trg_length if trg_length is None else trg_length
        trg = torch.as_tensor(trg).to(device=dev, dtype=torch.int64).contiguous()
        trg_length = torch.as_tensor(trg_length).to(device=dev, dtype=torch.int64).contiguous()
        if trg.dim() != 2 or trg.shape[0] != ctc_out.shape[0] or trg_length.shape != (trg.shape[0],):
            raise ValueError(f"forced_align: targets [B, L] and lengths [B] for B = {ctc_out.shape[0]} expected, got "
                             f"{tuple(trg.shape)} and {tuple(trg_length.shape)}")
        path, tok_start, tok_end, frame_logp, score = ops.ctc_align(ctc_out, lse, trg, in_len, trg_length, int(model.bos_index))
        return alignments(trg.cpu().numpy(), trg_length.cpu().numpy(), tok_start, tok_end, frame_logp, score, frame_seconds(model, frame_shift_ms))


def alignments(trg_h, len_h, tok_start, tok_end, frame_logp, score, sec: float, first_frame=None) -> List[Alignment]:
    """js2t_ctc_align's outputs as one Alignment per utterance.  trg_h [B, L] / len_h [B]: the labels on the host; first_frame
    (optional, [B]): where each utterance begins in a longer recording - its frames and seconds are then counted from there
    (long_form.transcribe_long's segments; frame_logp stays indexed from the utterance's own first frame)."""
    tok_start, tok_end, frame_logp, score = (t.cpu().numpy() for t in (tok_start, tok_end, frame_logp, score))
    trg_h = np.asarray(trg_h)
    len_h = np.minimum(np.asarray(len_h), trg_h.shape[1])
    out = []
    for b in range(trg_h.shape[0]):
        L = max(int(len_h[b]), 0)
        f0 = 0 if first_frame is None else int(first_frame[b])
        s, e = tok_start[b, :L].tolist(), tok_end[b, :L].tolist()
        ok = np.isfinite(score[b])
        logp = [float(np.mean(frame_logp[b, i:j], dtype=np.float64)) if ok else float("nan") for i, j in zip(s, e)]
        if ok:
            s, e = [i + f0 for i in s], [j + f0 for j in e]
        out.append(Alignment(tokens=trg_h[b, :L].tolist(), start_frame=s, end_frame=e, start=[i * sec if ok else float("nan") for i in s],
                             end=[j * sec if ok else float("nan") for j in e], logp=logp, score=float(score[b])))
    return out


def hypothesis_lengths(ids, eos_index: int, pad_index: int) -> np.ndarray:
    """length of every row of an id array: up to and INCLUDING the first EOS, or up to the first pad, whichever comes first"""
    ids = np.asarray(ids)
    n = np.full(ids.shape[0], ids.shape[1], dtype=np.int64)
    for b, row in enumerate(ids):
        for i, v in enumerate(row.tolist()):
            if v == pad_index:
                n[b] = i
                break
            if v == eos_index:
                n[b] = i + 1
                break
    return n


def align_hypotheses(model, batch, ids, pad_index: Optional[int] = None, frame_shift_ms: float = 10.0) -> List[Alignment]:
    """Align the id arrays `search` and `search.ctc_greedy` return ([B, L], pad-filled) to the utterances of `batch`."""
    pad = model.pad_index if pad_index is None else pad_index
    ids = np.asarray(ids)
    if ids.ndim != 2:
        raise ValueError(f"align_hypotheses: ids [B, L] expected, got {ids.shape}")
    n = hypothesis_lengths(ids, model.eos_index, pad)
    return forced_align(model, batch, trg=torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)), trg_length=torch.from_numpy(n),
                        frame_shift_ms=frame_shift_ms)


def _token_ids(tokens, who: str) -> np.ndarray:
    """a 1-d integer sequence (list, array or tensor) as i64 on the host; anything else is a ValueError"""
    if torch.is_tensor(tokens):
        tokens = tokens.detach().cpu().numpy()
    ids = np.asarray(tokens)
    if ids.ndim == 1 and ids.size == 0:
        return np.zeros(0, dtype=np.int64)
    if ids.ndim != 1 or ids.dtype.kind not in "iu":
        raise ValueError(f"{who}: tokens must be a 1-d integer sequence, got shape {ids.shape} of {ids.dtype}")
    return np.ascontiguousarray(ids, dtype=np.int64)


def align_stream(stream, tokens, blank: int, sec: float, free_start: bool = True, free_end: bool = True) -> Alignment:
    """Align the token ids of a whole recording's transcript to its stitched posterior stream (`long_form.stitch_posteriors`' result:
    logits f32 [T, V], lse, ...) with js2t_ctc_align_long; `sec`: seconds per encoder frame (`frame_seconds`).  free_start / free_end:
    audio in front of / behind the text (music, an announcer) is taken by a state that costs nothing; the first / last token's
    span is then shortened inside its run, and the frames the free state took count 0 in `score` (the header states both)."""
    from joeys2t_amd import ops
    ids = _token_ids(tokens, "align_stream")
    if not isinstance(stream, (tuple, list)) or len(stream) < 2 or not all(torch.is_tensor(t) for t in stream[:2]):
        raise ValueError("align_stream: stream = (logits [T, V], lse [T], ...) as stitch_posteriors returns it expected")
    logits, lse = stream[0], stream[1]
    if logits.dim() != 2 or lse.shape != (logits.shape[0],):
        raise ValueError(f"align_stream: logits [T, V] and lse [T] expected, got {tuple(logits.shape)} and {tuple(lse.shape)}")
    if not sec > 0.0:
        raise ValueError(f"align_stream: {sec} seconds per frame")
    with torch.no_grad():
        trg = torch.from_numpy(ids).to(logits.device)
        _, tok_start, tok_end, frame_logp, score = ops.ctc_align_long(logits.contiguous(), lse.contiguous(), trg, int(blank),
                                                                      free_start=free_start, free_end=free_end)
        return alignments(ids[None, :], [ids.size], tok_start[None, :], tok_end[None, :], frame_logp[None, :], score, float(sec))[0]


def utterance_spans(alignment: Alignment, token_counts: Sequence[int], window: int = 10) -> List[Tuple[float, float, float, float]]:
    """The transcript of an aligned recording is a run of sentences, sentence u has token_counts[u] tokens (their sum: the aligned
    tokens; none is 0).  Returns per sentence (start, end, mean_logp, worst_logp): the seconds of its first token's start and its last
    token's end; the mean of its tokens' `logp` over its FRAMES (weighted as `word_segments` weights a word); and the least such
    mean over every run of `window` consecutive tokens of the sentence (the whole sentence if it is shorter) - low where the text
    does not match the audio.  Pure host code."""
    counts = [int(n) for n in token_counts]
    window = int(window)
    if window < 1:
        raise ValueError(f"utterance_spans: window {window} below 1")
    if any(n < 1 for n in counts):
        raise ValueError("utterance_spans: a sentence of no tokens")
    if sum(counts) != len(alignment.tokens):
        raise ValueError(f"utterance_spans: {sum(counts)} tokens in the sentences, {len(alignment.tokens)} aligned")
    frames = [e - s for s, e in zip(alignment.start_frame, alignment.end_frame)]
    mass = [lp * n for lp, n in zip(alignment.logp, frames)]

    def mean(i, j):
        n = sum(frames[i:j])
        return sum(mass[i:j]) / n if n else float("nan")

    out, i = [], 0
    for n in counts:
        j = i + n
        w = min(window, n)
        out.append((alignment.start[i], alignment.end[j - 1], mean(i, j), min(mean(a, a + w) for a in range(i, j - w + 1))))
        i = j
    return out


def word_segments(pieces: Sequence[str], alignment: Alignment) -> List[Tuple[str, float, float, float]]:
    """Merge the token spans of `alignment` into words: `pieces` are the sentence pieces of its tokens, a piece that begins with the
    word marker opens a new word (so does the first piece).  Returns (word, start, end, mean logp) per word - start / end in seconds,
    the mean taken over the word's FRAMES (every token's mean weighted by its frame count).  Pieces beyond the pieces list (EOS) are
    left out.  Pure host code."""
    if len(pieces) > len(alignment.tokens):
        raise ValueError(f"word_segments: {len(pieces)} pieces for {len(alignment.tokens)} aligned tokens")
    words = []
    for i, piece in enumerate(pieces):
        n = alignment.end_frame[i] - alignment.start_frame[i]
        if i == 0 or piece.startswith(WORD_MARKER):
            words.append([piece.lstrip(WORD_MARKER), alignment.start[i], alignment.end[i], alignment.logp[i] * n, n])
        else:
            w = words[-1]
            w[0] += piece
            w[2] = alignment.end[i]
            w[3] += alignment.logp[i] * n
            w[4] += n
    return [(w[0], w[1], w[2], w[3] / w[4] if w[4] else float("nan")) for w in words]
