"""Plain NumPy / Python restatement of long-form CTC (joeys2t_amd/long_form.py, js2t_ctc_stitch, js2t_ctc_segment): the window
tiling, the stitch with a float64 lse, and the segmentation rule written the slow and obvious way - frame by frame, no scans.
tests/test_long_form_cpu.py pins it by hand-written cases; tests/test_hip_long_form.py compares the kernels against it."""
import math

import numpy as np


# ---------------------------------------------------------------- tiling
def plan_windows(n_frames, window, overlap, subsample):
    """(start, length, keep_lo, keep_hi, out_row, rows): window w starts at feature frame w * hop (hop = window - 2 * overlap), its
    encoder frame j is the recording's frame w * hop / subsample + j; the first window keeps from 0, the last to its end, the others
    [overlap / s, (overlap + hop) / s).  The fewest windows that reach the end of the recording."""
    s = subsample
    assert n_frames >= 1 and window % s == 0 and overlap % s == 0 and window - 2 * overlap >= 1 and overlap >= 0
    hop = window - 2 * overlap
    T = (n_frames + s - 1) // s
    start = [0]
    while start[-1] + window < n_frames:  # (in encoder frames the same test: the window does not reach the end yet)
        start.append(start[-1] + hop)
    W = len(start)
    length = [min(window, n_frames - st) for st in start]
    keep_lo, keep_hi, out_row = [], [], []
    for w, st in enumerate(start):
        frames = (length[w] + s - 1) // s
        lo = 0 if w == 0 else overlap // s
        hi = frames if w == W - 1 else (overlap + hop) // s
        keep_lo.append(lo), keep_hi.append(hi), out_row.append(st // s + lo)
    return start, length, keep_lo, keep_hi, out_row, T


def covered(plan):
    """how often every encoder frame of the recording is kept, and by which (window, frame)"""
    start, length, lo, hi, row, T = plan
    count = np.zeros(T, dtype=np.int64)
    for w in range(len(start)):
        assert 0 <= lo[w] <= hi[w]
        for j in range(lo[w], hi[w]):
            count[row[w] + j - lo[w]] += 1
    return count


# ---------------------------------------------------------------- stitch
def stitch(logits, keep_lo, keep_hi, out_row, rows, blank):
    """logits [W, S, V] (any float dtype, taken as they are) -> (out f32-valued f64 [rows, V], lse f64, argmax, blank_lp f64, written
    bool [rows]); rows nobody writes stay NaN / -1"""
    W, S, V = logits.shape
    out = np.full((rows, V), np.nan)
    lse, blp = np.full(rows, np.nan), np.full(rows, np.nan)
    am = np.full(rows, -1, dtype=np.int64)
    written = np.zeros(rows, dtype=bool)
    for w in range(W):
        for j in range(keep_lo[w], keep_hi[w]):
            r = out_row[w] + j - keep_lo[w]
            x = logits[w, j].astype(np.float64)
            m = x.max()
            out[r], lse[r] = x, m + math.log(np.exp(x - m).sum())
            am[r] = int(np.argmax(x))  # (the first maximum)
            blp[r] = x[blank] - lse[r]
            written[r] = True
    return out, lse, am, blp, written


# ---------------------------------------------------------------- segmentation
def silent_frames(blank_lp, argmax, blank, log_threshold):
    return [bool(a == blank and b >= log_threshold) for a, b in zip(argmax, blank_lp)]  # (NaN >= x is False)


def segment(blank_lp, argmax, blank, log_threshold, min_silence, margin, max_len, max_segments=None):
    """[(start, end)] of the segments, ascending, or -1 when there are more than max_segments"""
    assert min_silence >= 1 and margin >= 0 and max_len >= 1
    sil = silent_frames(blank_lp, argmax, blank, log_threshold)
    T = len(sil)
    pauses, t = [], 0  # maximal silent runs of at least min_silence frames
    while t < T:
        if not sil[t]:
            t += 1
            continue
        e = t
        while e < T and sil[e]:
            e += 1
        if e - t >= min_silence:
            pauses.append((t, e))
        t = e
    regions, a = [], 0  # (region, pause in front or None, pause behind or None)
    for k, (s, e) in enumerate(pauses):
        if s > a:
            regions.append((a, s, pauses[k - 1] if k else None, (s, e)))
        a = e
    if a < T:
        regions.append((a, T, pauses[-1] if pauses else None, None))
    out = []
    for a, b, front, behind in regions:
        lim = 0 if front is None or front[0] == 0 else front[0] + (front[1] - front[0]) // 2
        a2 = max(a - margin, lim)
        lim = T if behind is None or behind[1] == T else behind[0] + (behind[1] - behind[0]) // 2
        b2 = min(b + margin, lim)
        start = a2
        while start < b2:
            c = b2
            if b2 - start > max_len:
                c = start + max_len
                for cut in range(start + max_len, start + max_len // 2, -1):  # the largest cut in (start + max_len / 2, start + max_len]
                    if sil[cut - 1]:
                        c = cut
                        break
            if not all(sil[start:c]):
                out.append((start, c))
            start = c
    if max_segments is not None and len(out) > max_segments:
        return -1
    return out


def random_stream(seed, T, blank=0, V=6, p_flip=0.08, p_nan=0.01):
    """a seeded (blank_lp f32 [T], argmax i64 [T]): a two-state chain of silence and speech, blank_lp around the threshold log(0.9) in
    silence, some NaN"""
    rng = np.random.RandomState(seed)
    am = np.zeros(T, dtype=np.int64)
    lp = np.zeros(T, dtype=np.float32)
    state = rng.rand() < 0.5
    for t in range(T):
        if rng.rand() < p_flip:
            state = not state
        am[t] = blank if state or rng.rand() < 0.2 else rng.randint(1, V)
        lp[t] = np.float32(math.log(rng.choice([0.99, 0.95, 0.9, 0.85, 0.5]))) if am[t] == blank else np.float32(-3.0 - rng.rand())
        if rng.rand() < p_nan:
            lp[t] = np.nan
    return lp, am


LOG09 = float(np.float32(math.log(0.9)))  # what the f32 entry point compares against
PARAMS = [dict(min_silence=1, margin=0, max_len=10**6), dict(min_silence=3, margin=1, max_len=40), dict(min_silence=5, margin=4, max_len=17),
          dict(min_silence=2, margin=100, max_len=1), dict(min_silence=10**6, margin=0, max_len=64), dict(min_silence=8, margin=2, max_len=65)]


# ---------------------------------------------------------------- the stream of the concatenation test
# peak: sharp enough that the mass a beam of K loses to pruning - which differs between the whole stream and a word on its own - is
# far below the score tolerance (float64: the two differ by 0.08 tolerances); seed: the first from 9100 that is decidable
CONCAT = dict(V=12, K=4, C=3, words=(23, 31, 18, 27), pause=5, min_silence=2, peak=(13.0, 15.0), seed=9100)


def concat_stream(seed=None):
    """(logits f32 [T, V], [(start, end)] of the words): "words" of planted peaked posteriors (ctc_beam_reference.planted_logits)
    separated, opened and closed by pauses in which the blank has probability EXACTLY 1 - the labels' logits are -inf, so blank_lp
    is 0.0 and the frame adds exactly 0 to every score.  Inside a word the blank never reaches probability 1, so with
    silence_threshold = 1 the pauses are the silent runs and the words the segments."""
    import ctc_beam_reference as R
    c = CONCAT
    seed = c["seed"] if seed is None else seed
    quiet = np.full((c["pause"], c["V"]), -np.inf, dtype=np.float32)
    quiet[:, R.BLANK] = 0.0
    parts, spans, t = [quiet], [], c["pause"]
    for i, n in enumerate(c["words"]):
        parts += [R.planted_logits(seed + i, 1, n, c["V"], R.BLANK, peak=c["peak"])[0], quiet]
        spans.append((t, t + n))
        t += n + c["pause"]
    return np.concatenate(parts), spans


def concat_reference(seed=None):
    """float64: (top-1 of the whole stream, its score, [top-1 of every word], [their scores], the smallest pruning margin)"""
    import ctc_beam_reference as R
    c = CONCAT
    x, spans = concat_stream(seed)
    (whole, margin), = [R.beam_search(x, c["K"], c["C"], 1, R.BLANK)]
    per = [R.beam_search(x[a:b], c["K"], c["C"], 1, R.BLANK) for a, b in spans]
    return whole[0][0], whole[0][1], [h[0][0] for h, _ in per], [h[0][1] for h, _ in per], min([margin] + [m for _, m in per])
