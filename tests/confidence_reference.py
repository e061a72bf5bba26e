"""Plain Python / float64 NumPy reference of the token confidence of an n-best list (js2t_nbest_confidence,
include/joeys2t_hip.h), written from the header.  No GPU, no torch.

Semantics.  R = B * N hypotheses, N slots per utterance; ids [R, T], label counts n [R], scores [R]; pivot [B, P] slots.
    dead, posterior = mbr_reference's (the rule and the statement js2t_mbr_rescore has)
    D               = the unit-cost Levenshtein table of a pivot a (m labels) and a slot b (k labels), D[x][0] = x, D[0][y] = y
    path            = traced back from (m, k); at (x, y) the FIRST of: 1. x, y > 0, a[x-1] == b[y-1], D[x][y] == D[x-1][y-1]: match,
                      position x-1 of the pivot is matched, (x-1, y-1); 2. x, y > 0, D[x][y] == D[x-1][y-1] + 1: (x-1, y-1);
                      3. x > 0, D[x][y] == D[x-1][y] + 1: (x-1, y); 4. (x, y-1)
    match[b,p,j,l]  = 1 where position l of pivot p is matched by slot j; all ones inside the length for j == the pivot; 0 for a dead j,
                      for a dead pivot (outside 0 .. N-1 or a dead slot) and behind the pivot's length
    conf[b,p,l]     = sum over live j of posterior[j] * match[b,p,j,l]
    hyp_conf[b,p]   = posterior[pivot]; 0 for a dead pivot
"""
import numpy as np

import mbr_reference as M
from mbr_reference import bound  # noqa: F401  (one statement of the tolerance)


def table(a, b):
    """D as a list of lists of ints, (len(a) + 1) x (len(b) + 1)"""
    m, k = len(a), len(b)
    D = [[0] * (k + 1) for _ in range(m + 1)]
    for x in range(m + 1):
        D[x][0] = x
    for y in range(k + 1):
        D[0][y] = y
    for x in range(1, m + 1):
        for y in range(1, k + 1):
            D[x][y] = min(D[x - 1][y - 1] + (0 if a[x - 1] == b[y - 1] else 1), D[x - 1][y] + 1, D[x][y - 1] + 1)
    return D


def trace(a, b):
    """(the matched pairs (x-1, y-1) of the path in the order the back-trace meets them, the path's cost)"""
    a, b = [int(v) for v in a], [int(v) for v in b]
    D = table(a, b)
    x, y = len(a), len(b)
    pairs, cost = [], 0
    while x > 0 or y > 0:
        if x > 0 and y > 0 and a[x - 1] == b[y - 1] and D[x][y] == D[x - 1][y - 1]:
            pairs.append((x - 1, y - 1))
            x, y = x - 1, y - 1
        elif x > 0 and y > 0 and D[x][y] == D[x - 1][y - 1] + 1:
            x, y, cost = x - 1, y - 1, cost + 1
        elif x > 0 and D[x][y] == D[x - 1][y] + 1:
            x, cost = x - 1, cost + 1
        else:
            y, cost = y - 1, cost + 1
    return pairs, cost


def flags(a, b):
    """the pivot a's match flags against b: a list of len(a) 0 / 1"""
    out = [0] * len(a)
    for x, _ in trace(a, b)[0]:
        out[x] = 1
    return out


def flags_suffix_trimmed(a, b):
    """flags(a, b) computed the way the kernel may: the common suffix cut off and marked matched"""
    a, b = list(a), list(b)
    s = 0
    while s < min(len(a), len(b)) and a[len(a) - 1 - s] == b[len(b) - 1 - s]:
        s += 1
    return flags(a[:len(a) - s], b[:len(b) - s]) + [1] * s


def flags_prefix_trimmed(a, b):
    """what trimming the common PREFIX would give: NOT the rule (a = [0, 0], b = [0])"""
    a, b = list(a), list(b)
    s = 0
    while s < min(len(a), len(b)) and a[s] == b[s]:
        s += 1
    return [1] * s + flags(a[s:], b[s:])


def confidence(ids, n, score, N, pivot, Lp, scale):
    """(posterior f64 [R], conf f64 [B, P, Lp - 1], hyp_conf f64 [B, P], match u8 [B, P, N, Lp - 1]); reads ids of live slots at
    positions < n only"""
    n = np.asarray(n).reshape(-1)
    R = n.size
    assert R % N == 0
    B = R // N
    ids = np.asarray(ids).reshape(R, -1) if R else np.zeros((0, 0), dtype=np.int64)
    score32 = np.asarray(score, dtype=np.float32).reshape(R)
    pivot = np.asarray(pivot).reshape(B, -1)
    P = pivot.shape[1]
    dead = M.dead_slots(n, score32, Lp)
    post = M.mbr(ids, n, score32, N, Lp, scale)[1]  # the posterior is mbr_reference's, not a second statement of it
    W = max(Lp - 1, 0)
    match = np.zeros((B, P, N, W), dtype=np.uint8)
    conf = np.zeros((B, P, W))
    hyp = np.zeros((B, P))
    for b in range(B):
        for p in range(P):
            pv = int(pivot[b, p])
            if not 0 <= pv < N or dead[b * N + pv]:
                continue
            ra = b * N + pv
            a = ids[ra, :n[ra]].tolist()
            hyp[b, p] = post[ra]
            for j in range(N):
                rj = b * N + j
                if dead[rj]:
                    continue
                match[b, p, j, :len(a)] = 1 if j == pv else flags(a, ids[rj, :n[rj]].tolist())
                conf[b, p] += post[rj] * match[b, p, j]
    return post, conf, hyp, match
