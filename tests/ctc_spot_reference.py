"""NumPy reference of js2t_ctc_spot (imports nothing from the package): the rule of the header comment, restated.

spot: the Viterbi recursion over the 2 L - 1 CTC states of one phrase with a free start in every frame - h[t], the best score over
all starts and all alignments that end in frame t, and s[t], the frame that best alignment started in.  pick: the sweep that turns
(h, s) into disjoint hits.  One rounding per step in `dtype`: run in float32 on f32 inputs it is what the kernel computes, bit for
bit; run in float64 it is pinned by enumeration in test_ctc_spot_cpu.py.
"""
import numpy as np

PHRASES = ([3, 4, 4, 5], [7], [9, 10, 11, 12, 13, 14], [4, 5])  # planted_case: the last one occurs inside every first one
ABSENT = [1, 2]                                                 # ... and this one nowhere


def states(phrase, blank):
    """labels of the S = 2 L - 1 states: y_1, blank, y_2, ..., y_L"""
    lab = []
    for i, y in enumerate(phrase):
        if i:
            lab.append(int(blank))
        lab.append(int(y))
    return lab


def skip_allowed(lab):
    """state j may be entered from j - 2: even j >= 2 whose label differs from the label two states back"""
    return np.array([j >= 2 and j % 2 == 0 and lab[j] != lab[j - 2] for j in range(len(lab))], dtype=bool)


def emissions(x, norm, lab, dtype):
    """e[t, j] = x[t, label_j] - norm[t], one rounding in `dtype`; -inf for an id outside 0 .. V-1"""
    x, norm = np.asarray(x).astype(dtype), np.asarray(norm).astype(dtype)
    T, V = x.shape
    em = np.full((T, len(lab)), -np.inf, dtype=dtype)
    for j, l in enumerate(lab):
        if 0 <= l < V:
            em[:, j] = x[:, l] - norm
    return em


def spot(x, norm, phrase, blank, dtype=np.float64):
    """(h [T] of `dtype`, s i64 [T]) of one phrase through x [T, V] with the per-frame normaliser norm [T]"""
    lab = states(phrase, blank)
    S = len(lab)
    em = emissions(x, norm, lab, dtype)
    T = em.shape[0]
    skip = skip_allowed(lab)
    ninf = dtype(-np.inf)
    v, b = np.full(S, ninf, dtype=dtype), np.full(S, -1, dtype=np.int64)
    h, s = np.full(T, ninf, dtype=dtype), np.full(T, -1, dtype=np.int64)
    for t in range(T):
        best, bb = v.copy(), b.copy()
        if not v[0] >= 0:  # the free start: a path that lies below 0 is replaced by one that starts here
            best[0], bb[0] = 0, t
        p1v, p1b = np.concatenate(([ninf], v[:-1])), np.concatenate(([-1], b[:-1]))
        take = p1v > best  # (never state 0: its left neighbour is -inf)
        best[take], bb[take] = p1v[take], p1b[take]
        p2v, p2b = np.concatenate(([ninf, ninf], v[:-2]))[:S], np.concatenate(([-1, -1], b[:-2]))[:S]
        take = skip & (p2v > best)
        best[take], bb[take] = p2v[take], p2b[take]
        v = (best + em[t]).astype(dtype)
        b = np.where(v == -np.inf, -1, bb)
        h[t], s[t] = v[S - 1], b[S - 1]
    return h, s


def pick(h, s, log_threshold):
    """the hits [(start, end, score)] of one phrase: ascending, disjoint, end one past the last frame"""
    hits = []
    have, cs, cb, ce, last_end = False, 0.0, 0, 0, -1
    for t in range(len(h)):
        if not (h[t] >= log_threshold and s[t] > last_end):
            continue
        if not have:
            have, cs, cb, ce = True, h[t], int(s[t]), t
        elif s[t] > ce:
            hits.append((cb, ce + 1, cs))
            last_end = ce
            cs, cb, ce = h[t], int(s[t]), t
        elif h[t] > cs or (h[t] == cs and s[t] == cb):
            cs, cb, ce = h[t], int(s[t]), t
    if have:
        hits.append((cb, ce + 1, cs))
    return hits


def planted_case(seed, V=32, copies=6):
    """(logits f32 [T, V], expected): PHRASES[0 .. 2] each planted `copies` times in a random order, every label held for 1 .. 3
    frames (a blank frame between repeated labels) with +8 on the planted id, and 1 .. 11 frames between two occurrences (3 .. 19 at
    the ends) that favour ids 16 .. 31, which no phrase holds.  expected[p] = [(first frame of y_1's run, one past y_L's run)] of
    PHRASES[p], ascending; PHRASES[3] = [4, 5] from the second 4 of every [3, 4, 4, 5].  Blank is id 0."""
    rs = np.random.RandomState(seed)
    order = rs.permutation(np.repeat(np.arange(3), copies))
    ids, expected = [], [[] for _ in PHRASES]
    ids += [-1] * int(rs.randint(3, 20))
    for n_done, p in enumerate(order):
        phrase, start, sub = PHRASES[p], len(ids), None
        for i, y in enumerate(phrase):
            if i and y == phrase[i - 1]:
                ids.append(0)
            if p == 0 and i == 2:
                sub = len(ids)
            ids += [y] * int(rs.randint(1, 4))
        expected[p].append((start, len(ids)))
        if sub is not None:
            expected[3].append((sub, len(ids)))
        ids += [-1] * int(rs.randint(3, 20) if n_done == len(order) - 1 else rs.randint(1, 12))
    x = rs.randn(len(ids), V).astype(np.float32)
    for t, y in enumerate(ids):
        x[t, y if y >= 0 else int(rs.randint(16, 32))] += 8.0
    return x, expected
