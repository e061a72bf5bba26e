"""CPU: tests/ctc_spot_reference.py, the NumPy restatement of js2t_ctc_spot's rule that test_hip_ctc_spot.py holds the kernel to, is
itself pinned here: the float64 h_t against the enumeration of every start and every state path, the planted property, and the
picker's tie cases by hand."""
import itertools
import math

import numpy as np

import ctc_spot_reference as RS

BLANK = 0


def exhaustive(em, skip, starts=None):
    """h[t] = the best sum of emissions over all frames a <= t (a in `starts`, if given) and all state paths that are in state 0 in
    frame a, in state S - 1 in frame t, and move by 0, 1 or (where skip allows the target) 2 states per frame"""
    T, S = em.shape
    h = np.full(T, -np.inf)
    for a in (range(T) if starts is None else starts):
        for t in range(a, T):
            n = t - a + 1
            for moves in itertools.product((0, 1, 2), repeat=n - 1):
                if sum(moves) != S - 1:
                    continue
                j, total, ok = 0, em[a, 0], True
                for i, m in enumerate(moves):
                    j += m
                    if m == 2 and not skip[j]:
                        ok = False
                        break
                    total += em[a + 1 + i, j]
                if ok:
                    h[t] = max(h[t], total)
    return h


def test_float64_reference_equals_the_enumeration():
    rs = np.random.RandomState(0)
    n, with_repeat, with_skip = 0, 0, 0
    for case in range(60):
        T, V, L = int(rs.randint(1, 8)), 4, int(rs.randint(1, 4))
        phrase = [int(v) for v in rs.randint(1, V, size=L)]  # (repeats included)
        if case % 5 == 0 and L >= 2:
            phrase[1] = phrase[0]
        x = (rs.randn(T, V) * 2.0)
        norm = x.max(axis=1) if case % 2 == 0 else rs.randn(T)  # the row maximum, and a normaliser that leaves emissions above 0
        lab = RS.states(phrase, BLANK)
        skip = RS.skip_allowed(lab)
        want = exhaustive(RS.emissions(x, norm, lab, np.float64), skip)
        h, s = RS.spot(x, norm, phrase, BLANK)
        for t in range(T):
            if want[t] == -np.inf:
                assert h[t] == -np.inf and s[t] == -1, (case, t)
            else:
                assert abs(h[t] - want[t]) <= 1e-12 and 0 <= s[t] <= t, (case, t, h[t], want[t])
        n += 1
        with_repeat += any(a == b for a, b in zip(phrase[:-1], phrase[1:]))
        with_skip += bool(skip.any())
    assert n >= 40 and with_repeat >= 8 and with_skip >= 8


def test_start_is_the_start_of_a_best_path():
    """s[t] names a start whose best path reaches h[t]: the recursion restricted to that start gives the same value"""
    rs = np.random.RandomState(1)
    for _ in range(20):
        T, V = 7, 4
        phrase = [int(v) for v in rs.randint(1, V, size=int(rs.randint(1, 4)))]
        x = rs.randn(T, V) * 2.0
        norm = x.max(axis=1)
        h, s = RS.spot(x, norm, phrase, BLANK)
        lab = RS.states(phrase, BLANK)
        em, skip = RS.emissions(x, norm, lab, np.float64), RS.skip_allowed(lab)
        for t in range(T):
            if s[t] >= 0:
                assert abs(exhaustive(em[:t + 1], skip, starts=[int(s[t])])[t] - h[t]) <= 1e-12


def test_planted_phrases_are_found_exactly():
    thr = math.log(0.5)
    for seed in range(6):
        x, expected = RS.planted_case(seed)
        norm = x.max(axis=1)
        assert len(expected[0]) == len(expected[3]) == 6
        for dtype in (np.float64, np.float32):
            for phrase, want in zip(RS.PHRASES, expected):
                hits = RS.pick(*RS.spot(x, norm, phrase, BLANK, dtype), thr)
                assert [(a, b) for a, b, _ in hits] == want, (seed, phrase)
                assert all(sc == 0.0 for _, _, sc in hits)
            assert RS.pick(*RS.spot(x, norm, RS.ABSENT, BLANK, dtype), thr) == []


def test_picker_tie_cases():
    ninf = -np.inf
    # the same start and the same score: the end moves over the last label's run
    assert RS.pick(np.array([ninf, 0.0, 0.0, 0.0, ninf]), np.array([-1, 1, 1, 1, -1]), -1.0) == [(1, 4, 0.0)]
    # the same score from a later start inside the current hit: dropped
    assert RS.pick(np.array([-0.5, -0.5, -0.5]), np.array([0, 0, 1]), -1.0) == [(0, 2, -0.5)]
    # a later, better, overlapping candidate replaces the current one (frame 2 starts at 1 <= ce = 1)
    assert RS.pick(np.array([ninf, -0.5, -0.25]), np.array([-1, 0, 1]), -1.0) == [(1, 3, -0.25)]
    # a worse overlapping candidate is dropped, a disjoint one emits the current hit
    assert RS.pick(np.array([-0.25, -0.5, -0.5]), np.array([0, 0, 2]), -1.0) == [(0, 1, -0.25), (2, 3, -0.5)]
    # a candidate that starts inside an emitted hit is ignored, however good: hit (0, 3) is out once frame 4 starts at 4 > 2, and
    # frame 5's path starts at 2 <= last_end; frame 6 extends the hit that frame 4 opened
    h = np.array([ninf, ninf, -0.5, ninf, -0.5, 0.0, -0.5])
    s = np.array([-1, -1, 0, -1, 4, 2, 4])
    assert RS.pick(h, s, -1.0) == [(0, 3, -0.5), (4, 7, -0.5)]
    # below the threshold, and a NaN: no candidate
    assert RS.pick(np.array([-2.0, np.nan, -1.0]), np.array([0, 1, 2]), -1.0) == [(2, 3, -1.0)]
    assert RS.pick(np.zeros(0), np.zeros(0, dtype=np.int64), -1.0) == []
