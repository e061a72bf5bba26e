"""Live CTC decoding (EXTENSION; every other decoder here takes finished input): captions while the audio arrives.

Two session objects over js2t_ctc_stream_step, the resumable prefix beam search whose header comment states the endpoint rule:
  `CTCStreamDecoder`: n_streams independent posterior streams (a server's sessions).  `push` takes each stream's new CTC logits
      rows, runs ONE step launch for all of them, reads the result back once, and returns the utterances that ended inside the rows
      (finals, through the n-best stage chain of ctc_search, so lm / decision="mbr" / confidence work) and what is being said now
      (partials, with the length of the prefix that can no longer change).
  `StreamingTranscriber`: one stream from audio.  `feed` takes waveform samples or feature rows as they come, encodes a window as
      soon as its `window` feature frames exist and pushes the window's kept centre frames: the latency of a frame is at most
      window - overlap feature frames plus the encoder's run.  Over a session it pushes the rows `long_form.stitch_posteriors(...,
      batch_size=1)` gives the same features, in order and bit for bit; the windows and their kept frames are that module's.

What is causal here and not there.  `long_form.segment` cuts a finished stream at pause midpoints, with margins; the rule here ends
a segment `min_silence` silent frames after its last spoken one (the trailing silence belongs to it), opens the next at the first
frame that is not silent, and cuts a segment that reaches `max_segment` frames where it stands.  Not measured, not claimed:
recognition accuracy, and what the causal endpoint rule costs against js2t_ctc_segment's on real speech.
`min_silence` and `max_segment` are ENCODER frames (`alignment.frame_seconds` each)."""
import math
from typing import List, Optional

import numpy as np
import torch

from joeys2t_amd import long_form, ops

WHY = {1: "endpoint", 2: "forced", 3: "flushed"}


class CTCStreamDecoder:
    """model: its special indices (blank = bos_index), its target vocabulary (with an lm) and its encoder's stride (for the seconds).
    n_streams: the streams of one launch.  beam_size / n_best / candidates and, in nbest_options, lm / lm_weight / length_bonus /
    lm_fusion / n_rescore / context / context_weight / decision / mbr_scale / confidence / confidence_scale / return_parts:
    search.ctc_beam_search's, with the meaning and the refusals `ctc_search.NBestOptions` states; attention rescoring (ctc_weight) is
    refused as in transcribe_long.  min_silence (None: no endpoints - only max_segment and flush end a segment), silence_threshold
    (the blank's probability from which a frame is silent, in (0, 1]) and max_segment: the rule's.  max_finals: the records a stream
    can hand back per launch; a stream with more endpoints in one push is simply stepped again with the rest of its rows.
    device: where the state lives (default: the model's parameters')."""

    def __init__(self, model, n_streams: int = 1, *, beam_size: int = 10, n_best: int = 1, candidates: int = 8,
                 min_silence: Optional[int] = None, silence_threshold: float = 0.9, max_segment: int = 1500, max_finals: int = 4,
                 frame_shift_ms: float = 10.0, device=None, **nbest_options):
        from joeys2t_amd import alignment
        who = "CTCStreamDecoder"
        self.opt, self.return_parts, self.beam_size, self.n_best, self.N = long_form._options(nbest_options, beam_size, n_best, who=who)
        threshold = float(silence_threshold)
        if not 0.0 < threshold <= 1.0:  # (a NaN fails too)
            raise ValueError(f"{who}: silence_threshold {threshold} outside (0, 1] (a probability of the blank)")
        if int(n_streams) < 1 or int(max_finals) < 1 or int(max_segment) < 1 or (min_silence is not None and int(min_silence) < 1):
            raise ValueError(f"{who}: n_streams {n_streams}, max_finals {max_finals}, max_segment {max_segment} and min_silence "
                             f"{min_silence} must be at least 1 (min_silence may be None)")
        self.model, self.B, self.candidates = model, int(n_streams), int(candidates)
        self.log_threshold, self.min_silence = math.log(threshold), 0 if min_silence is None else int(min_silence)
        self.max_len, self.max_finals = int(max_segment), int(max_finals)
        self.sec = alignment.frame_seconds(model, frame_shift_ms)
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        self.state = ops.ctc_stream_state(self.B, self.beam_size, self.max_len, self.device)
        self._out = ops.ctc_stream_outputs(self.device, self.B, self.N, self.max_finals, self.max_len)
        self._flush = [0] * self.B
        self._V = None  # the width of the logits, known from the first rows
        self.launches = 0

    # ---------------------------------------------------------------- one stream
    def flush(self, b: int = 0):
        """end stream b's open utterance now: its final record (or nothing, if none is open).  Returns push's pair."""
        self._flush[int(b)] = 1
        return self.push([None] * self.B)

    def reset(self, b: int = 0) -> None:
        """stream b starts again at frame 0 (a new session in its slot); an open utterance is dropped"""
        self.state[int(b)].zero_()
        self._flush[int(b)] = 0

    # ---------------------------------------------------------------- all streams
    def _rows(self, chunks):
        """the five row arrays of a step from the chunks, back to back, and each stream's row count"""
        count, logits, argmax = [], [], []
        for c in chunks:
            if c is None:
                count.append(0)
                continue
            st, am = (c[0], c[2]) if isinstance(c, (tuple, list)) else (c, None)  # ops.ctc_stitch's four, or the logits alone
            if st.dim() != 2 or st.dtype != torch.float32:
                raise ValueError(f"CTCStreamDecoder: f32 logits [frames, V] expected, got {st.dtype} {tuple(st.shape)}")
            count.append(st.shape[0])
            logits.append(st)
            argmax.append(am)
        if sum(count) == 0:  # a step without rows (a flush, a poll): the width the lm and the graph are checked against, no data
            V = self._V or (self.opt.lm.V if self.opt.fused and self.opt.lm is not None else self.opt.context.V if self.opt.biased else
                            max(2, int(self.model.bos_index) + 1, int(self.model.eos_index) + 1))
            empty = lambda dt, *shape: torch.empty(shape, dtype=dt, device=self.device)  # noqa: E731
            return count, (empty(torch.float32, 0, V), empty(torch.float32, 0), empty(torch.int64, 0), empty(torch.int64, 0, 1),
                           empty(torch.float32, 0, 1))
        st = logits[0].contiguous() if len(logits) == 1 else torch.cat(logits)
        V = self._V = st.shape[1]
        cand_id, cand_lp, lse = ops.ctc_beam_candidates(st, min(self.candidates, V - 1), self.model.bos_index)
        if any(a is None for a in argmax):
            _, am = ops.row_lse(st, want_argmax=True)
        else:
            am = argmax[0].contiguous() if len(argmax) == 1 else torch.cat(argmax)
        return count, (st, lse, am, cand_id, cand_lp)

    def push(self, chunks: List):
        """chunks: per stream its new rows - f32 logits [t_b, V] on the device, or the four tensors ops.ctc_stitch returns for them -
        or None.  Returns (finals, partials): per stream the list of utterances that ended, in time order, each a dict laid out like
        long_form.decode_stream's - "start" / "end" (seconds), "start_frame" / "end_frame" (counted from the stream's reset), "ids" (n_best
        i64 arrays, best first - by risk under decision="mbr"), "scores" f32 [n_best], "why" ("endpoint", "forced" or "flushed") and
        with return_parts or confidence "parts" - and per stream {"ids": the labels of the best live prefix (before any EOS term),
        "stable": how many of them can no longer change, "start_frame": the open utterance's first frame, -1 when none is open}.
        One launch and one host read per step; a stream that fills its max_finals record slots is stepped again with its rest."""
        from joeys2t_amd import ctc_search
        if len(chunks) != self.B:
            raise ValueError(f"CTCStreamDecoder: {len(chunks)} chunks for {self.B} streams")
        opt, dev, B = self.opt, self.device, self.B
        finals = [[] for _ in range(B)]
        with torch.no_grad():
            count, rows = self._rows(chunks)
            lm = (ctc_search._to(opt.lm, dev), opt.lm_weight, opt.length_bonus) if opt.fused else (None, 0.0, 0.0)
            context = (ctc_search._to(opt.context, dev), opt.context_weight) if opt.biased else (None, 0.0)
            while True:
                off = torch.tensor(np.concatenate([[0], np.cumsum(count)]), dtype=torch.int32, device=dev)
                flush = torch.tensor(self._flush, dtype=torch.int32, device=dev)
                ops.ctc_stream_step(self.state, rows, off, flush, beam=self.beam_size, n_best=self.N, max_finals=self.max_finals,
                                    max_len=self.max_len, blank=self.model.bos_index, pad=self.model.pad_index, lm=lm[0],
                                    bos=self.model.bos_index, eos=self.model.eos_index, lm_weight=lm[1], length_bonus=lm[2], context=context[0],
                                    context_weight=context[1], log_threshold=self.log_threshold, min_silence=self.min_silence, out=self._out)
                self.launches += 1
                host = {k: v.numpy() for k, v in ops.ctc_stream_outputs(self._out["buf"].cpu(), B, self.N, self.max_finals, self.max_len).items()}
                self._stages(host, finals)
                used = host["consumed"].tolist()
                rest = [n - u for n, u in zip(count, used)]
                self._flush = [f if r else 0 for f, r in zip(self._flush, rest)]  # (honoured by the call that consumed all its rows)
                if not any(rest):
                    break
                first = np.concatenate([[0], np.cumsum(count)])[:-1]
                keep = torch.cat([torch.arange(int(a) + u, int(a) + n, device=dev) for a, u, n in zip(first, used, count)])
                rows, count = tuple(r[keep] for r in rows), rest
        partials = [{"ids": host["part_ids"][b, :host["part_len"][b]].copy(), "stable": int(host["stable_len"][b]),
                     "start_frame": int(host["part_start"][b])} for b in range(B)]
        return finals, partials

    def _stages(self, host, finals) -> None:
        """the step's final records through ctc_search.ctc_stages as one list, appended per stream"""
        from joeys2t_amd import ctc_search
        F, N, L, o = self.max_finals, self.N, self.max_len, self._out
        sel = [(b, i) for b in range(self.B) for i in range(int(host["n_final"][b]))]
        if not sel:
            return
        idx = torch.tensor([b * F + i for b, i in sel], dtype=torch.int64, device=self.device)
        pick = lambda name, *shape: o[name].view(self.B * F, *shape)[idx]  # noqa: E731
        lst = ctc_search.NBest(pick("fin_ids", N, L), pick("fin_len", N), pick("fin_ctc", N), pick("fin_score", N),
                               pick("fin_ctx", N) if self.opt.biased else None)
        ids, scores, n, *parts = ctc_search.ctc_stages(self.model, lst, self.opt, self.n_best, self.return_parts)
        for k, (b, i) in enumerate(sel):
            rows = slice(k * self.n_best, (k + 1) * self.n_best)
            first, length = int(host["fin_start"][b, i]), int(host["fin_n"][b, i])
            rec = {"start": float(first * self.sec), "end": float((first + length) * self.sec), "start_frame": first, "end_frame": first + length,
                   "ids": [ids[r, :n[r]].copy() for r in range(rows.start, rows.stop)], "scores": scores[rows, 0].copy(),
                   "why": WHY[int(host["fin_why"][b, i])]}
            if parts:
                rec["parts"] = {key: v[rows] for key, v in parts[0].items()}
            finals[b].append(rec)


class StreamingTranscriber:
    """One live stream from audio to captions.  model, window, overlap, cmvn, sample_rate, n_mel_bins: long_form.stitch_posteriors'
    (window and overlap in FEATURE frames, multiples of the encoder's stride); everything else: CTCStreamDecoder's.
    keep_rows: remember the feature rows as they are completed (`features`) and the stitched rows as they are pushed (`rows`: a list
    of ops.ctc_stitch results), for inspection."""

    def __init__(self, model, *, window: int, overlap: int, cmvn=None, sample_rate: int = 16000, n_mel_bins: int = 80,
                 keep_rows: bool = False, **decoder_options):
        self.s = long_form._stride(model)
        long_form.plan_windows(1, window, overlap, self.s)  # (the refusals of the window arithmetic)
        self.model, self.window, self.overlap, self.hop = model, int(window), int(overlap), int(window) - 2 * int(overlap)
        self.cmvn, self.sample_rate, self.n_mel = cmvn, int(sample_rate), int(n_mel_bins)
        self.decoder = CTCStreamDecoder(model, 1, **decoder_options)
        self.device = self.decoder.device
        self.rows, self.features = ([], []) if keep_rows else (None, None)
        self._wave = self._feat = None   # the samples no complete frame has used up; the feature rows from _f0 on
        self._f0 = self._n = self._w = 0  # first buffered feature frame, feature frames so far, windows encoded so far
        self._last = None                # the newest encoded window's logits [1, S, V]: it may turn out to be the last
        self._partial = {"ids": np.zeros(0, dtype=np.int64), "stable": 0, "start_frame": -1}

    def _features(self, chunk):
        """the new feature rows a chunk completes: feature rows as they are; samples through the front end, frame by whole frame"""
        chunk = torch.as_tensor(chunk)
        if chunk.dim() == 2:
            if self._wave is not None:
                raise ValueError("StreamingTranscriber: feature rows after waveform samples")
            return chunk.to(self.device, torch.float32)
        if chunk.dim() != 1 or (self._wave is None and self._n):
            raise ValueError(f"StreamingTranscriber: waveform samples [n] or feature rows [frames, F] expected, one kind per session; got "
                             f"{tuple(chunk.shape)}")
        from joeys2t_amd.helpers_for_audio import get_extractor
        ext = get_extractor(self.device, self.sample_rate, self.n_mel)
        chunk = chunk.to(self.device, torch.float32)
        wave = chunk if self._wave is None else torch.cat([self._wave, chunk])
        k = ext.n_frames(wave.numel())  # the frames whose 25 ms lie wholly in the buffer
        if k == 0:
            self._wave = wave
            return wave.new_empty((0, self.n_mel))
        feat, _, _ = ext.batch(wave.contiguous(), [wave.numel()], [0])
        self._wave = wave[k * ext.shift:].clone()  # frame k starts there
        return feat

    def _stitch(self, logits, lo, hi):
        """frames lo .. hi - 1 of an encoded window as stream rows, pushed; the finals they close"""
        if hi <= lo:
            return []
        t = lambda v: torch.tensor([v], dtype=torch.int32, device=self.device)  # noqa: E731
        chunk = ops.ctc_stitch(logits, t(lo), t(hi), t(0), self.model.bos_index, rows=hi - lo)
        if self.rows is not None:
            self.rows.append(chunk)
        (finals, ), (self._partial, ) = self.decoder.push([chunk])
        return finals

    def feed(self, chunk):
        """chunk: the next waveform samples f32 [n] or the next feature rows [frames, F] (one kind per session), any length.
        Returns (the utterances that ended, the partial result) - CTCStreamDecoder.push's for this one stream."""
        finals = []
        with torch.no_grad():
            new = self._features(chunk)
            if new.shape[0]:
                if self.features is not None:
                    self.features.append(new)
                self._feat = new if self._feat is None else torch.cat([self._feat, new])
                self._n += new.shape[0]
            o, h = self.overlap // self.s, self.hop // self.s
            while self._n >= self._w * self.hop + self.window:  # window _w is complete: encode it alone, keep what a middle window keeps
                st = self._w * self.hop - self._f0
                self._last = long_form.encode_windows(self.model, self._feat, [st], [self.window], self.cmvn, self.s)
                finals += self._stitch(self._last, 0 if self._w == 0 else o, o + h)
                self._w += 1
                drop = self._w * self.hop - self._f0  # the next window starts there
                self._feat, self._f0 = self._feat[drop:], self._f0 + drop
        return finals, self._partial

    def finish(self):
        """the end of the session: the rest of the recording as `long_form.plan_windows` lays it out for the final length - the short
        last window encoded, or the newest encoded window's remaining frames if it turns out to be the plan's last - then a flush.
        Samples that do not fill a last 25 ms frame are dropped, as the front end drops them.  Returns the utterances that ended."""
        if self._n < 1:
            raise ValueError("StreamingTranscriber: the session is shorter than one feature frame")
        finals = []
        with torch.no_grad():
            plan = long_form.plan_windows(self._n, self.window, self.overlap, self.s)
            W = len(plan.start)
            if self._w == W:  # every planned window is encoded: the newest one keeps to its end after all
                finals += self._stitch(self._last, self.overlap // self.s + self.hop // self.s, plan.keep_hi[-1])
            else:
                assert self._w == W - 1 and plan.start[-1] == self._f0, (self._w, W)
                sub = getattr(self.model.encoder, "subsampler", None)
                if sub is not None and sub.out_len(plan.length[-1]) != -(-plan.length[-1] // self.s):
                    raise ValueError(f"StreamingTranscriber: the subsampler's lengths are not ceil(n / {self.s}): its kernel sizes are not supported")
                last = long_form.encode_windows(self.model, self._feat, [plan.start[-1] - self._f0], [plan.length[-1]], self.cmvn, self.s)
                finals += self._stitch(last, plan.keep_lo[-1], plan.keep_hi[-1])
            more, (self._partial, ) = self.decoder.flush(0)
        return finals + more[0]

    def reset(self) -> None:
        """a new session"""
        self.decoder.reset(0)
        self._wave = self._feat = self._last = None
        self._f0 = self._n = self._w = 0
        if self.rows is not None:
            self.rows, self.features = [], []
        self._partial = {"ids": np.zeros(0, dtype=np.int64), "stable": 0, "start_frame": -1}
