"""CPU: the reference of long-form CTC (tests/long_form_reference.py) pinned by hand-written cases - the window tiling and the
segmentation rule js2t_ctc_segment states - plus what needs no device of the feature itself: the host arithmetic of
joeys2t_amd.long_form.plan_windows, the declarations, the refusals made before a launch, and the decidability of the stream the GPU
concatenation test uses (tests/test_hip_long_form.py)."""
import math

import numpy as np
import pytest

import ctc_beam_reference as R
import long_form_reference as L

BLANK = 0
MARK = {"S": (BLANK, math.log(0.99)), "x": (1, -3.0), "b": (BLANK, math.log(0.5)), "n": (BLANK, float("nan"))}
# hand-written streams: S a silent frame, x speech, b a blank that is not confident, n a blank whose log-probability is NaN
SEGMENT_CASES = {
    "empty": ("", dict(min_silence=2, margin=0, max_len=4), []),
    "all_silent_one_pause": ("SSSSS", dict(min_silence=2, margin=3, max_len=4), []),
    "all_silent_no_pause": ("SSSSS", dict(min_silence=10, margin=0, max_len=100), []),  # one region, of silent frames only: dropped
    "no_silence_forced": ("xxxxxxxxxx", dict(min_silence=2, margin=0, max_len=4), [(0, 4), (4, 8), (8, 10)]),
    "pause_of_min_silence_and_one_less": ("xxSSSxxSSxx", dict(min_silence=3, margin=0, max_len=100), [(0, 2), (5, 11)]),
    "pauses_at_both_ends": ("SSSxxxSSS", dict(min_silence=2, margin=1, max_len=100), [(2, 7)]),
    "pauses_at_both_ends_wide_margin": ("SSSxxxSSS", dict(min_silence=2, margin=50, max_len=100), [(0, 9)]),
    "margins_meet_in_a_short_pause": ("xxSSSxx", dict(min_silence=2, margin=5, max_len=100), [(0, 3), (3, 7)]),
    "margin_smaller_than_the_pause": ("xxSSSSSSxx", dict(min_silence=2, margin=1, max_len=100), [(0, 3), (7, 10)]),
    "cut_behind_a_silent_frame_of_the_upper_half": ("xxxxxSxxxx", dict(min_silence=5, margin=0, max_len=8), [(0, 6), (6, 10)]),
    "cut_without_one": ("xxSxxxxxxx", dict(min_silence=5, margin=0, max_len=8), [(0, 8), (8, 10)]),
    "cut_takes_the_last_silent_frame": ("xxxxxSxSxx", dict(min_silence=5, margin=0, max_len=8), [(0, 8), (8, 10)]),
    "silent_piece_dropped": ("xxxxSSSSxxxx", dict(min_silence=10, margin=0, max_len=4), [(0, 4), (8, 12)]),
    "max_len_one": ("xSx", dict(min_silence=5, margin=0, max_len=1), [(0, 1), (2, 3)]),
    "nan_is_not_silent": ("xxSnSxx", dict(min_silence=3, margin=0, max_len=100), [(0, 7)]),
    "nan_replaced": ("xxSSSxx", dict(min_silence=3, margin=0, max_len=100), [(0, 2), (5, 7)]),
    "unconfident_blank_is_not_silent": ("xxSbSxx", dict(min_silence=3, margin=0, max_len=100), [(0, 7)]),
}


def stream(marks):
    am = np.array([MARK[m][0] for m in marks], dtype=np.int64)
    lp = np.array([MARK[m][1] for m in marks], dtype=np.float32)
    return lp, am


@pytest.mark.parametrize("name", list(SEGMENT_CASES))
def test_segmentation_rule_by_hand(name):
    marks, params, want = SEGMENT_CASES[name]
    lp, am = stream(marks)
    assert L.segment(lp, am, BLANK, L.LOG09, **params) == want


def test_segments_are_ascending_disjoint_and_never_silent_only():
    for seed in range(20):
        lp, am = L.random_stream(seed, 300)
        sil = L.silent_frames(lp, am, BLANK, L.LOG09)
        for params in L.PARAMS:
            segs = L.segment(lp, am, BLANK, L.LOG09, **params)
            bound = 300 // params["min_silence"] + 300 // (params["max_len"] // 2 + 1) + 2
            assert len(segs) <= bound
            for (a, b), (c, _) in zip(segs, segs[1:] + [(300, 300)]):
                assert 0 <= a < b <= c and b - a <= params["max_len"] and not all(sil[a:b])
    assert L.segment(*L.random_stream(3, 300), BLANK, L.LOG09, max_segments=2, **L.PARAMS[1]) == -1


TILING = [(10, "below one window"), (16, "one window"), (24, "one hop more"), (25, "one frame more"), (30, "no multiple of the stride"),
          (1, "one frame"), (1003, "long")]


@pytest.mark.parametrize("n_frames", [n for n, _ in TILING])
def test_tiling_covers_every_frame_once(n_frames):
    from joeys2t_amd.long_form import plan_windows
    for window, overlap, s in ((16, 4, 4), (16, 0, 4), (24, 8, 4), (6, 2, 2), (5, 1, 1)):
        plan = L.plan_windows(n_frames, window, overlap, s)
        assert (L.covered(plan) == 1).all() and plan[5] == -(-n_frames // s)
        assert tuple(plan_windows(n_frames, window, overlap, s)) == plan
        start, length, lo, hi, row, _ = plan
        hop = window - 2 * overlap
        assert start == [w * hop for w in range(len(start))] and all(0 < n <= window for n in length)
        assert lo[0] == 0 and hi[-1] == -(-length[-1] // s) and row == [st // s + k for st, k in zip(start, lo)]


def test_tiling_by_hand():
    assert L.plan_windows(10, 16, 4, 4) == ([0], [10], [0], [3], [0], 3)
    assert L.plan_windows(24, 16, 4, 4) == ([0, 8], [16, 16], [0, 1], [3, 4], [0, 3], 6)
    assert L.plan_windows(25, 16, 4, 4) == ([0, 8, 16], [16, 16, 9], [0, 1, 1], [3, 3, 3], [0, 3, 5], 7)
    assert L.plan_windows(30, 16, 4, 4) == ([0, 8, 16], [16, 16, 14], [0, 1, 1], [3, 3, 4], [0, 3, 5], 8)


@pytest.mark.parametrize("bad", [dict(window=18, overlap=4), dict(window=16, overlap=2), dict(window=16, overlap=8), dict(window=16, overlap=-4),
                                 dict(window=0, overlap=0), dict(window=16, overlap=4, n_frames=0)])
def test_plan_windows_refusals(bad):
    from joeys2t_amd.long_form import plan_windows
    with pytest.raises(ValueError, match="transcribe_long"):
        plan_windows(bad.pop("n_frames", 100), subsample=4, **bad)


def test_stitch_reference_by_hand():
    x = np.array([[[0.0, 1.0, 1.0], [2.0, 0.0, 0.0]], [[5.0, 5.0, 5.0], [0.0, 0.0, 3.0]]], dtype=np.float32)
    out, lse, am, blp, written = L.stitch(x, [1, 0], [2, 0], [2, 0], 4, blank=0)
    assert written.tolist() == [False, False, True, False] and am.tolist() == [-1, -1, 0, -1]  # window 1 keeps nothing
    assert out[2].tolist() == [2.0, 0.0, 0.0] and abs(lse[2] - math.log(math.exp(2) + 2)) < 1e-12 and abs(blp[2] - (2 - lse[2])) < 1e-12
    _, _, am, _, _ = L.stitch(x, [0, 0], [1, 1], [0, 1], 2, blank=0)
    assert am.tolist() == [1, 0]  # the FIRST maximum of a tie


def test_concatenation_stream_is_decidable():
    """what test_hip_long_form.py's concatenation test relies on, in float64 alone: the words' top-1 labellings concatenate to the
    whole stream's, the scores add up within the tolerance, and no pruning decision is closer than 4 tolerances"""
    y, s, ys, ss, margin = L.concat_reference()
    assert margin >= R.DECIDABLE
    assert tuple(v for w in ys for v in w) == y and all(len(w) > 0 for w in ys)
    assert abs(sum(ss) - s) <= 0.25 * R.bound(s)
    x, spans = L.concat_stream()
    lp = R.log_softmax(x)[:, BLANK].astype(np.float32)
    segs = L.segment(lp, x.argmax(axis=1), BLANK, 0.0, L.CONCAT["min_silence"], 0, 10**6)  # silence_threshold = 1: log 1 = 0
    assert segs == spans


def test_declarations_and_export():
    import joeys2t_amd
    from joeys2t_amd import _lib
    for name, n_args in (("js2t_ctc_stitch", 15), ("js2t_ctc_segment", 14), ("js2t_ctc_segment_workspace_bytes", 1)):
        assert name in _lib.FUNCTIONS and len(_lib.FUNCTIONS[name][1]) == n_args
    assert joeys2t_amd.transcribe_long is joeys2t_amd.long_form.transcribe_long and callable(joeys2t_amd.plan_windows)
    with pytest.raises(AttributeError):
        joeys2t_amd.no_such_name


def test_refusals_before_the_model_is_touched():
    """bad options and bad window arithmetic are ValueErrors raised before anything of the model but its stride is looked at"""
    from types import SimpleNamespace
    from joeys2t_amd.long_form import transcribe_long
    model = SimpleNamespace(encoder=SimpleNamespace(subsampler=SimpleNamespace(n_layers=2)))
    ok = dict(window=16, overlap=4)
    with pytest.raises(ValueError, match="packed encoder rows"):
        transcribe_long(model, None, ctc_weight=0.3, **ok)
    with pytest.raises(ValueError, match="multiples of the encoder's stride 4"):
        transcribe_long(model, None, window=18, overlap=4)
    with pytest.raises(ValueError, match="hop"):
        transcribe_long(model, None, window=16, overlap=8)
    with pytest.raises(ValueError, match="transcribe_long: n_best"):
        transcribe_long(model, None, beam_size=2, n_best=3, **ok)
    with pytest.raises(ValueError, match="transcribe_long: lm_weight"):
        transcribe_long(model, None, lm_weight=0.5, **ok)
    with pytest.raises(ValueError, match="unknown options"):
        transcribe_long(model, None, temperature=2.0, **ok)
