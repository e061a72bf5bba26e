"""Phrase spotting (EXTENSION; the reference has no keyword search): WHERE in a recording is a phrase said?

For a list of names or terms, without decoding first: the stitched CTC posterior stream of `long_form.stitch_posteriors` already
holds what is needed.  For every phrase js2t_ctc_spot runs a Viterbi recursion over the phrase's CTC states with a free start in
every frame (one launch, one wavefront per phrase; its header comment is the rule) and picks disjoint hits from the per-frame scores.

The score of a hit is the log of (probability of the phrase's best alignment over its span / probability of the frame-wise best
path over the same span): the per-frame normaliser handed to the kernel is the logit of the frame's arg-max.  It is <= 0, and 0
where the phrase's labels ARE the arg-max of every frame of the span.  `threshold` is that ratio as a probability in (0, 1].  The
default 0.5 is a definition - "the best alignment has at least half the probability of the frame-wise best path" - not a tuned
value.  Not measured, not claimed: detection accuracy or false-alarm rate on a trained model, and what window stitching does to them.
Contextual biasing (`biasing`) only nudges the beam; searching the decoded 1-best misses what the beam pruned; this needs neither.
"""
import math
from typing import List, NamedTuple

import numpy as np
import torch

WHO = "find_phrases"


class PhraseHit(NamedTuple):
    """One occurrence: `phrase` is the index into the list handed to find_phrases; [start_frame, end_frame) in encoder frames - the
    first frame of the first label's run to one past the last label's run, as in alignment.Alignment; [start, end) in seconds;
    score: the log probability ratio of the module docstring."""
    phrase: int
    start_frame: int
    end_frame: int
    start: float
    end: float
    score: float


def phrases_from_text(phrases, vocab):
    """phrases: strings of whitespace-separated pieces, or sequences of pieces, in the vocabulary's own tokens - the lookup and the
    dropping rule of biasing.ContextGraph.from_text: a phrase with a piece the vocabulary does not hold is dropped.  Returns (id lists
    of the phrases kept, in order; the number dropped)."""
    from joeys2t_amd.biasing import phrase_ids
    return phrase_ids(phrases, vocab)


def _phrase_ids(phrases, most: int):
    """the phrases as host i64 arrays; every refusal is a ValueError raised before the device is touched"""
    from joeys2t_amd.alignment import _token_ids
    rows = []
    for k, p in enumerate(phrases):
        ids = _token_ids(p, WHO)
        if ids.size == 0:
            raise ValueError(f"{WHO}: phrase {k} is empty")
        if ids.size > most:
            raise ValueError(f"{WHO}: phrase {k} has {ids.size} tokens, more than {most}")
        rows.append(ids)
    return rows


def _log_threshold(threshold) -> float:
    threshold = float(threshold)
    if not 0.0 < threshold <= 1.0:  # (a NaN fails too)
        raise ValueError(f"{WHO}: threshold {threshold} outside (0, 1] (a probability ratio)")
    return math.log(threshold)


def find_phrases(stream, phrases, blank: int, seconds_per_frame: float, threshold: float = 0.5, max_hits: int = 64,
                 frame_scores: bool = False):
    """stream: what `long_form.stitch_posteriors` returns, (logits f32 [T, V], lse, argmax i64 [T], blank_lp); phrases: a list of 1-d
    integer sequences of 1 .. 32 token ids; blank: the CTC blank (model.bos_index); seconds_per_frame: `alignment.frame_seconds`.
    threshold: the probability ratio of the module docstring, in (0, 1].  max_hits: the hits per phrase to make room for; when a
    phrase has more, the kernel runs once more with room for the largest count, so every hit is returned.
    Returns the hits of all phrases as a list of PhraseHit sorted by (start_frame, phrase); with frame_scores=True the triple (that
    list, frame_score f32 [K, T], frame_start i32 [K, T]) - the dense h_t / s_t of js2t_ctc_spot on the device, a detection curve.
    One host read, the counts (a second after a rerun).  Raises ValueError, before the device is touched, for an empty phrase, one of
    more than 32 tokens, tokens that are not 1-d integers, a threshold outside (0, 1] and max_hits < 1."""
    from joeys2t_amd import ops
    log_threshold = _log_threshold(threshold)
    max_hits = int(max_hits)
    if max_hits < 1:
        raise ValueError(f"{WHO}: max_hits {max_hits} below 1")
    rows = _phrase_ids(phrases, 32)
    if not float(seconds_per_frame) > 0.0:
        raise ValueError(f"{WHO}: {seconds_per_frame} seconds per frame")
    if not isinstance(stream, (tuple, list)) or len(stream) < 3 or not all(torch.is_tensor(t) for t in stream[:3]):
        raise ValueError(f"{WHO}: stream = (logits [T, V], lse [T], argmax [T], ...) as stitch_posteriors returns it expected")
    logits, argmax = stream[0], stream[2]
    if logits.dim() != 2 or argmax.shape != (logits.shape[0],) or argmax.dtype != torch.int64:
        raise ValueError(f"{WHO}: logits [T, V] and argmax i64 [T] expected, got {tuple(logits.shape)} and {argmax.dtype} {tuple(argmax.shape)}")
    K, T = len(rows), logits.shape[0]
    if K == 0 and not frame_scores:
        return []
    Lmax = max((r.size for r in rows), default=1)
    tokens = np.zeros((K, Lmax), dtype=np.int64)
    for k, r in enumerate(rows):
        tokens[k, :r.size] = r
    dev = logits.device
    with torch.no_grad():
        logits = logits.contiguous()
        norm = logits.gather(1, argmax[:, None]).reshape(T).float().contiguous()  # (an indexed copy: the logit at the arg-max)
        tok = torch.from_numpy(tokens).to(dev)
        lengths = torch.tensor([r.size for r in rows], dtype=torch.int32, device=dev)  # 1 .. Lmax by construction
        out = ops.ctc_spot(logits, norm, tok, lengths, int(blank), log_threshold, max_hits=max_hits, frame_scores=frame_scores)
        count = out[0].cpu().numpy()
        if K and int(count.max()) > max_hits:  # the kernel counts what it finds: once more, with room for all
            out = ops.ctc_spot(logits, norm, tok, lengths, int(blank), log_threshold, max_hits=int(count.max()), frame_scores=frame_scores)
            count = out[0].cpu().numpy()
        start, end, score = (t.cpu().numpy() for t in out[1:4])
    sec = float(seconds_per_frame)
    hits = [PhraseHit(k, int(start[k, i]), int(end[k, i]), int(start[k, i]) * sec, int(end[k, i]) * sec, float(score[k, i]))
            for k in range(K) for i in range(int(count[k]))]
    hits.sort(key=lambda h: (h.start_frame, h.phrase))
    return (hits, out[4], out[5]) if frame_scores else hits
