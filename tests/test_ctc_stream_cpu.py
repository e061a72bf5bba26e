"""The rule of live CTC decoding (js2t_ctc_stream_step) pinned without a GPU: tests/ctc_stream_reference.py on hand-written streams
whose segments can be read off the script, its own invariance under cutting, and the decidability of every pinned stream the GPU
tests compare against it - asserted here, so that no GPU case is skipped."""
import math

import numpy as np
import pytest

import ctc_beam_reference as R
import ctc_stream_reference as S

V, BLANK = 4, 0
THR = math.log(0.9)


def script(text):
    """logits f32 [T, V] of a script: 'x' a frame that says a label (the labels cycle), 's' a confident blank (p > 0.99), 'b' a
    blank arg-max that is NOT confident (p about 0.5)"""
    x = np.zeros((len(text), V), dtype=np.float32)
    for t, ch in enumerate(text):
        if ch == "x":
            x[t, 1 + t % (V - 1)] = 8.0
        else:
            x[t, BLANK] = 9.0 if ch == "s" else 1.2
    return x


def stream(**kw):
    return S.Stream(**{**dict(K=3, C=2, n_best=2, blank=BLANK, log_threshold=THR, min_silence=3, max_len=100), **kw})


def test_script_frames_are_what_they_say():
    lp, am = S.frame_stats(script("xsb"), BLANK)
    assert am.tolist() == [1, BLANK, BLANK] and lp[1] > math.log(0.99) and math.log(0.4) < lp[2] < math.log(0.6) and lp[0] < -5


def test_a_pause_one_short_of_min_silence_then_exactly_min_silence():
    s = stream()
    finals, used = s.step(script("xx" + "ss" + "xx" + "sss" + "s" + "x"))
    assert used == 11 and S.segments(finals) == [(0, 9, S.ENDPOINT)]  # the trailing silence belongs to the segment
    assert s.state() == (S.SPEECH, 11, 10, 1, 0)  # frame 9 was skipped in IDLE, frame 10 opened the next segment
    assert finals[0]["hyps"][0][0] == (1, 2, 2, 3)  # frames 0, 1, 4, 5 say 1, 2, 2, 3 - the blank in between keeps the repeat


def test_an_unconfident_blank_is_not_silence():
    finals, _ = stream().step(script("xx" + "sbs" + "x" + "sss"))
    assert S.segments(finals) == [(0, 9, S.ENDPOINT)]


def test_an_endpoint_on_a_calls_last_row():
    s = stream()
    finals, used = s.step(script("xxsss"))
    assert used == 5 and S.segments(finals) == [(0, 5, S.ENDPOINT)] and s.state() == (S.IDLE, 5, None, None, None)
    finals, used = s.step(script("ssx"), flush=True)
    assert S.segments(finals) == [(7, 8, S.FLUSHED)]


def test_a_forced_cut_and_the_next_segment_behind_skipped_silence():
    s = stream(max_len=5)
    finals, _ = s.step(script("xxxxx" + "ss" + "xx"), flush=True)
    assert S.segments(finals) == [(0, 5, S.FORCED), (7, 9, S.FLUSHED)]
    # an endpoint that falls on the max_len-th frame is an endpoint
    finals, _ = stream(max_len=5).step(script("xxsss"))
    assert S.segments(finals) == [(0, 5, S.ENDPOINT)]
    # a forced cut inside a pause: the rest of the pause is skipped, no segment of silence alone
    finals, _ = stream(max_len=4).step(script("xxss" + "ss" + "x"), flush=True)
    assert S.segments(finals) == [(0, 4, S.FORCED), (6, 7, S.FLUSHED)]


def test_a_stream_of_silence_only():
    s = stream()
    finals, used = s.step(script("s" * 20), flush=True)
    assert finals == [] and used == 20 and s.state() == (S.IDLE, 20, None, None, None) and s.partial() == ((), 0, -1)


def test_min_silence_zero_never_ends_a_segment():
    finals, _ = stream(min_silence=0).step(script("xx" + "s" * 30 + "x"))
    assert finals == []


def test_nan_blank_lp_is_not_silent():
    x = script("sss" + "xx" + "sss")
    lp, am = S.frame_stats(x, BLANK)
    lp[1] = np.nan  # in IDLE: opens a segment
    lp[6] = np.nan  # in SPEECH: breaks the run
    s = stream()
    finals, _ = s.step(x, blank_lp=lp, argmax=am)
    assert finals == [] and s.state() == (S.SPEECH, 8, 1, 7, 1)


def test_flush_in_idle_and_in_speech():
    s = stream()
    assert s.step(script("ss"), flush=True) == ([], 2) and s.step(script(""), flush=True) == ([], 0)
    finals, _ = s.step(script("xxs"), flush=True)
    assert S.segments(finals) == [(2, 5, S.FLUSHED)] and s.state()[0] == S.IDLE
    assert s.step(script(""), flush=True) == ([], 0)


def test_max_finals_one_with_two_endpoints_in_one_call():
    x = script("xxsss" + "s" + "xsss" + "x")
    s = stream(max_finals=1)
    finals, used = s.step(x, flush=True)
    assert used == 5 and S.segments(finals) == [(0, 5, S.ENDPOINT)]  # (the flush waits for a call that consumes all its rows)
    more, used = s.step(x[5:], flush=True)
    assert used == 5 and S.segments(more) == [(6, 10, S.ENDPOINT)]
    last, used = s.step(x[10:], flush=True)
    assert used == 1 and S.segments(last) == [(10, 11, S.FLUSHED)]
    whole, _ = stream().step(x, flush=True)
    assert S.segments(whole) == S.segments(finals + more + last) and [r["hyps"] for r in whole] == [r["hyps"] for r in finals + more + last]
    assert S.segments(S.run(x, [10**9], max_finals=1, K=3, C=2, n_best=2, blank=BLANK, log_threshold=THR, min_silence=3, max_len=100)[0]) == \
        S.segments(whole)


def test_partial_and_stable_prefix():
    s = stream()
    s.step(script("xx" + "s" + "x"))
    ids, stable, start = s.partial()
    assert ids == (1, 2, 1) and start == 0 and 0 <= stable <= len(ids)


@pytest.mark.parametrize("cuts", [[1], [7], [63], [64], [65], [0, 5, 0, 0, 33], [3, 64, 1]])
def test_the_reference_does_not_depend_on_the_cuts(cuts):
    want = S.stream_reference("c", "k6")
    whole_state = S.run(S.stream_case("c"), [10**9], blank=S.BLANK, **S.SEARCHES["k6"], **S.RULE)[1]
    got, state = S.run(S.stream_case("c"), cuts, blank=S.BLANK, **S.SEARCHES["k6"], **S.RULE)
    assert S.segments(got) == S.segments(want) and [r["hyps"] for r in got] == [r["hyps"] for r in want] and state == whole_state
    for mf in (1, 2):
        again, state = S.run(S.stream_case("c"), cuts, blank=S.BLANK, max_finals=mf, **S.SEARCHES["k6"], **S.RULE)
        assert S.segments(again) == S.segments(want) and state == whole_state


def test_the_words_of_the_concatenation_stream_are_the_segments():
    """long_form_reference.concat_stream: pauses in which the blank has probability exactly 1.  With the threshold at probability 1
    every word ends min_silence frames into the pause behind it, and those frames add exactly 0: the word's own labels and score"""
    import long_form_reference as L
    c = L.CONCAT
    x, spans = L.concat_stream()
    _, _, want, want_s, margin = L.concat_reference()
    assert margin >= R.DECIDABLE
    finals, state = S.run(x, [17], K=c["K"], C=c["C"], n_best=1, blank=R.BLANK, log_threshold=0.0, min_silence=c["min_silence"], max_len=10**6)
    assert S.segments(finals) == [(a, b + c["min_silence"], S.ENDPOINT) for a, b in spans] and state[0] == S.IDLE
    assert [r["hyps"][0][0] for r in finals] == want
    assert all(abs(r["hyps"][0][1] - s) <= 1e-9 for r, s in zip(finals, want_s))


def test_pinned_streams_have_every_kind_of_segment():
    for name in S.SEEDS:
        segs = S.segments(S.stream_reference(name, "k6"))
        assert len(segs) >= 3 and {w for _, _, w in segs} >= {S.ENDPOINT, S.FORCED}, (name, segs)
        assert max(b - a for a, b, _ in segs) == S.RULE["max_len"]
    assert S.segments(S.stream_reference("a", "k6"))[-1][2] == S.FLUSHED


@pytest.mark.parametrize("name,search", S.REF_CASES)
def test_pinned_streams_are_decidable(name, search):
    finals = S.stream_reference(name, search)
    margin = min(r["margin"] for r in finals)
    print(f"{name} / {search}: {len(finals)} segments, margin {margin:.1f} tolerances")
    assert margin >= R.DECIDABLE


def test_pinned_seeds_are_the_first_decidable_ones():
    assert {name: S.find_seed(name) for name in S.SEEDS} == S.SEEDS
