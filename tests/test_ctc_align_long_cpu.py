"""CPU: the reference of js2t_ctc_align_long (tests/ctc_align_long_reference.py) pinned by brute-force enumeration of all state
paths, with and without free ends; the planted-path property that free ends exist for; alignment.utterance_spans on a
hand-computed case; the argument refusals of alignment.align_stream that need no device; the C ABI declares the entry points."""
import numpy as np
import pytest
import torch

import ctc_align_long_reference as RL
import ctc_align_reference as R
from joeys2t_amd import alignment
from joeys2t_amd._lib import Js2tError, declared_symbols

FLAGS = [(False, False), (True, False), (False, True), (True, True)]


def test_header_declares_the_long_aligner():
    assert {"js2t_ctc_align_long", "js2t_ctc_align_long_workspace_bytes", "js2t_ctc_align_long_tiles"} <= set(declared_symbols())


def state_paths(T, S, skip):
    """every state path of T frames: starts in state 0 or 1, moves by 0, 1 or (where the skip is allowed) 2, ends in S-1 or S-2"""
    out = []

    def walk(path):
        if len(path) == T:
            if path[-1] in (S - 1, S - 2):
                out.append(tuple(path))
            return
        s = path[-1]
        for step in (0, 1, 2):
            n = s + step
            if n < S and (step < 2 or skip[n]):
                walk(path + [n])

    for s in (0, 1):
        if s < S:
            walk([s])
    return out


@pytest.mark.parametrize("free_start,free_end", FLAGS)
@pytest.mark.parametrize("target", [[], [1], [2], [1, 2], [2, 1], [1, 1], [2, 2]])
def test_reference_against_enumeration_of_state_paths(target, free_start, free_end):
    V, blank = 3, 0
    rs = np.random.RandomState(23 + 31 * len(target) + sum(target))
    ext = R.extended(target, blank)
    S, skip = len(ext), R.skip_allowed(ext, blank)
    for T in range(1, 7):
        logp = R.log_softmax(rs.randn(T, V) * 2.0)
        got = RL.align_free(logp, target, blank, free_start, free_end)
        paths = state_paths(T, S, skip)
        if not paths:
            assert got["path"] is None and got["score"] == -np.inf, (T, target)
            continue
        scores = {p: RL.path_score_free(logp, target, blank, p, free_start, free_end) for p in paths}
        best = max(scores.values())
        tol = 1e-12 * max(1.0, abs(best))
        assert abs(got["score"] - best) <= tol, (T, target, got["score"], best)
        R.check_path(got["path"], target, blank)
        assert scores[tuple(got["path"].tolist())] >= best - tol
        assert abs(float(got["frame_logp"].sum()) - got["score"]) <= tol
        free = ((got["path"] == 0) & free_start) | ((got["path"] == S - 1) & free_end)
        assert (got["frame_logp"][free] == 0).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_flags_off_is_the_utterance_reference(dtype):
    rs = np.random.RandomState(4)
    for T, target in ((1, []), (9, [3, 3, 1]), (30, [1, 2, 2, 5, 9]), (4, [1, 1, 1]), (12, [2, 40])):
        logp = R.log_softmax(rs.randn(T, 12), dtype)
        a, b = R.align(logp, target, 0, dtype), RL.align_free(logp, target, 0, dtype=dtype)
        assert a.keys() == b.keys()
        for k in a:
            if a[k] is None:
                assert b[k] is None
            else:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])) and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype


def test_planted_path_needs_the_free_ends():
    """200 recordings with a head and a tail the text lacks (RL.planted_case): with free ends every label lies inside its planted run
    and the inner ones ARE their runs; without them the head and tail frames must be explained by blanks and labels of the text,
    which drags labels out of their runs - the property fails for most cases (a reference without the free columns fails here)."""
    with_free = without = 0
    for seed in range(200):
        x, target, runs = RL.planted_case(seed)
        logp = R.log_softmax(x)
        with_free += RL.planted_ok(RL.align_free(logp, target, 0, True, True), runs)
        without += RL.planted_ok(RL.align_free(logp, target, 0, False, False), runs)
    print(f"planted path: {with_free} of 200 with free ends, {without} of 200 without")
    assert with_free == 200
    assert without < 100


def test_utterance_spans_known_answer():
    a = alignment.Alignment(tokens=[10, 11, 12, 13, 14], start_frame=[1, 3, 4, 9, 12], end_frame=[3, 4, 6, 10, 13],
                            start=[0.04, 0.12, 0.16, 0.36, 0.48], end=[0.12, 0.16, 0.24, 0.40, 0.52],
                            logp=[-0.5, -1.0, -0.25, -2.0, -0.1], score=-7.0)
    spans = alignment.utterance_spans(a, [3, 2], window=2)
    assert [(s[0], s[1]) for s in spans] == [(0.04, 0.24), (0.36, 0.52)]
    # sentence 1: tokens of 2, 1, 2 frames; windows of 2 tokens: (-0.5 * 2 - 1.0) / 3 and (-1.0 - 0.25 * 2) / 3
    assert spans[0][2] == pytest.approx((-0.5 * 2 - 1.0 * 1 - 0.25 * 2) / 5) and spans[0][3] == pytest.approx(-2.0 / 3)
    # sentence 2: tokens of 1 and 1 frame; one window, the sentence itself
    assert spans[1][2] == pytest.approx(-1.05) and spans[1][3] == pytest.approx(-1.05)
    whole, = alignment.utterance_spans(a, [5])  # shorter than the default window of 10: the sentence is the one window
    assert whole[2] == whole[3] == pytest.approx((-1.0 - 1.0 - 0.5 - 2.0 - 0.1) / 7) and (whole[0], whole[1]) == (0.04, 0.52)
    assert alignment.utterance_spans(a, [1, 1, 1, 1, 1], window=1)[3] == (0.36, 0.40, pytest.approx(-2.0), pytest.approx(-2.0))
    assert [w[0] for w in alignment.word_segments(["▁a", "b", "▁c", "d", "e"], a)] == ["ab", "cde"]  # (works on it unchanged)
    for bad in ([3, 1], [5, 0], [0, 5], [6]):
        with pytest.raises(ValueError):
            alignment.utterance_spans(a, bad)
    with pytest.raises(ValueError):
        alignment.utterance_spans(a, [5], window=0)


def test_align_stream_refusals_without_a_device():
    logits, lse = torch.zeros(6, 5), torch.zeros(6)
    for bad in ([[1, 2]], [1.0, 2.0], np.zeros((2, 2), dtype=np.int64), torch.zeros(3)):
        with pytest.raises(ValueError, match="1-d integer"):
            alignment.align_stream((logits, lse), bad, 0, 0.04)
    with pytest.raises(ValueError, match="stream"):
        alignment.align_stream(logits, [1], 0, 0.04)
    with pytest.raises(ValueError, match="lse"):
        alignment.align_stream((logits, torch.zeros(5)), [1], 0, 0.04)
    with pytest.raises(ValueError, match="seconds"):
        alignment.align_stream((logits, lse), [1], 0, 0.0)
    with pytest.raises(Js2tError, match="CPU tensor"):  # no fall-back: the kernel runs on the device only
        alignment.align_stream((logits, lse), [1, 2], 0, 0.04)
