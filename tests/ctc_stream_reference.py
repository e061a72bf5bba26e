"""Plain NumPy / Python restatement of live CTC decoding's rule (js2t_ctc_stream_step, include/joeys2t_hip.h): a stream walks its
frames one at a time, IDLE or in SPEECH; a segment is a list of buffered rows and is decoded, when it ends, by
ctc_beam_reference.beam_search over those rows alone - float64, nothing resumed.  That a resumed f32 search equals this is what
tests/test_hip_ctc_stream.py checks; tests/test_ctc_stream_cpu.py pins this file by hand-written cases.  No GPU, no torch."""
import functools
import math

import numpy as np

import ctc_beam_reference as R
import long_form_reference as L

IDLE, SPEECH = 0, 1
ENDPOINT, FORCED, FLUSHED = 1, 2, 3


def frame_stats(logits, blank):
    """(blank_lp f64 [T], argmax [T]) of raw logits [T, V]: the first maximum; a row of -inf but the blank has blank_lp 0"""
    logits = np.asarray(logits, dtype=np.float64).reshape(-1, np.shape(logits)[-1])
    if logits.shape[0] == 0:
        return np.zeros(0), np.zeros(0, dtype=np.int64)
    return R.log_softmax(logits)[:, blank], logits.argmax(axis=1)


class Stream:
    """One stream.  step() takes the next rows and returns (final records, rows consumed); the records are dicts start / n / why /
    hyps (beam_search's n_best (tuple, score), best first) / margin."""

    def __init__(self, K, C, n_best, blank, log_threshold, min_silence, max_len, max_finals=10**9):
        assert 1 <= n_best <= K and min_silence >= 0 and max_len >= 1 and max_finals >= 1
        self.K, self.C, self.n_best, self.blank = K, C, n_best, blank
        self.log_threshold, self.min_silence, self.max_len, self.max_finals = log_threshold, min_silence, max_len, max_finals
        self.phase, self.frames, self.start, self.run, self.rows = IDLE, 0, 0, 0, []

    @property
    def n(self):
        return len(self.rows)

    def state(self):
        """what must not depend on how the rows were cut into calls"""
        return (self.phase, self.frames, self.start if self.phase == SPEECH else None, self.n if self.phase == SPEECH else None,
                self.run if self.phase == SPEECH else None)

    def _final(self, why):
        x = np.stack(self.rows)
        hyps, margin = R.beam_search(x, self.K, self.C, self.n_best, self.blank)
        rec = dict(start=self.start, n=len(self.rows), why=why, hyps=hyps, margin=margin)
        self.phase, self.rows = IDLE, []
        return rec

    def step(self, logits, flush=False, blank_lp=None, argmax=None):
        logits = np.asarray(logits)
        if blank_lp is None:
            blank_lp, argmax = frame_stats(logits, self.blank)
        silent = L.silent_frames(blank_lp, argmax, self.blank, self.log_threshold)  # (js2t_ctc_segment's test: a NaN is not silent)
        finals, consumed = [], 0
        for t in range(len(silent)):
            if len(finals) == self.max_finals:  # no slot for a further record: the caller sends the rest again
                break
            consumed += 1
            frame, self.frames = self.frames, self.frames + 1
            if self.phase == IDLE:
                if silent[t]:
                    continue
                self.phase, self.start, self.run, self.rows = SPEECH, frame, 0, []
            self.rows.append(logits[t])
            self.run = self.run + 1 if silent[t] else 0
            if self.min_silence > 0 and self.run == self.min_silence:
                finals.append(self._final(ENDPOINT))
            elif len(self.rows) == self.max_len:
                finals.append(self._final(FORCED))
        if consumed == len(silent) and flush and self.phase == SPEECH:
            finals.append(self._final(FLUSHED))
        return finals, consumed

    def partial(self):
        """(labels of the best live prefix, stable length = the longest common prefix of ALL live prefixes, start or -1)"""
        if self.phase == IDLE:
            return (), 0, -1
        hyps, _ = R.beam_search(np.stack(self.rows), self.K, self.C, self.K, self.blank)
        seqs = [y for y, _ in hyps]
        stable = 0
        while all(len(y) > stable for y in seqs) and len({y[stable] for y in seqs}) == 1:
            stable += 1
        return seqs[0], stable, self.start


def run(logits, cuts, flush_last=True, **kw):
    """one stream over logits [T, V] cut into calls of the given sizes (cycled; 0 = an empty call), every call's unconsumed rows sent
    again: (final records in order, the state at the end)"""
    s = Stream(**kw)
    finals, t, i, T = [], 0, 0, len(logits)
    while t < T:
        size = cuts[i % len(cuts)]
        i += 1
        a, b = t, min(t + size, T)
        while True:
            recs, used = s.step(logits[a:b], flush=flush_last and b == T)
            finals += recs
            a += used
            if a == b:
                break
        t = b
    if T == 0 and flush_last:
        finals += s.step(logits[:0], flush=True)[0]
    return finals, s.state()


def segments(finals):
    return [(r["start"], r["start"] + r["n"], r["why"]) for r in finals]


# ---------------------------------------------------------------- the streams of the GPU tests
BLANK, V = 2, 12
LOG09 = float(np.float32(math.log(0.9)))
RULE = dict(log_threshold=LOG09, min_silence=4, max_len=40)
SEARCHES = {"k1": dict(K=1, C=1, n_best=1), "k6": dict(K=6, C=5, n_best=3), "k32": dict(K=32, C=5, n_best=2), "k6c8": dict(K=6, C=8, n_best=6)}
STREAM_BASE = {"a": 2000, "b": 2100, "c": 2200}
STREAM_LEN = {"a": 300, "b": 217, "c": 129}
# the (stream, search) pairs whose kernel results are compared with THIS reference, and so must be decidable (the comparisons of
# kernel against kernel are bitwise and need no margin: they run every search over every stream)
REF_CASES = [("a", "k6"), ("a", "k6c8"), ("b", "k1"), ("b", "k6"), ("c", "k32")]


def planted_stream(seed, T):
    """logits f32 [T, V]: test_hip_long_form.route_case's make - planted words of 20 .. 70 frames (some longer than RULE's max_len)
    between pauses of 3 .. 9 confident blank frames (some shorter than its min_silence) - from one seed"""
    rs = np.random.RandomState(seed)
    parts, n = [], 0
    while n < T:
        word = R.planted_logits(seed * 16 + len(parts), 1, int(rs.randint(20, 71)), V, BLANK)[0]
        quiet = rs.randn(int(rs.randint(3, 10)), V).astype(np.float32)
        quiet[:, BLANK] += 9.0
        parts += [word, quiet]
        n += len(word) + len(quiet)
    return np.concatenate(parts)[:T]


def stream_margin(name, seed, search):
    finals, _ = run(planted_stream(seed, STREAM_LEN[name]), [10**9], blank=BLANK, **SEARCHES[search], **RULE)
    return min(r["margin"] for r in finals), finals


def find_seed(name, tries=64):
    """how SEEDS was made: the first seed from the stream's base on which every segment is decidable under the stream's searches in
    REF_CASES"""
    for seed in range(STREAM_BASE[name], STREAM_BASE[name] + tries):
        if all(stream_margin(name, seed, s)[0] >= R.DECIDABLE for n, s in REF_CASES if n == name):
            return seed
    return None


SEEDS = {"a": 2002, "b": 2102, "c": 2219}


@functools.lru_cache(maxsize=None)
def stream_case(name):
    """the pinned stream: computed once per process, do not modify"""
    return planted_stream(SEEDS[name], STREAM_LEN[name])


@functools.lru_cache(maxsize=None)
def stream_reference(name, search):
    """the pinned stream's final records under RULE and SEARCHES[search], flushed at its end: computed once, do not modify"""
    return run(stream_case(name), [10**9], blank=BLANK, **SEARCHES[search], **RULE)[0]
