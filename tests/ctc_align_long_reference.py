"""NumPy reference of js2t_ctc_align_long (imports nothing from the package): the loop of ctc_align_reference.align with free ends.

With free_start the emission of state 0 is 0 in every frame, with free_end that of state S-1 (for L = 0 the one state is both);
everything else - recursion, -inf for an id outside the vocabulary, the tie rule - is ctc_align_reference's.  With both flags off
align_free returns exactly what R.align returns.  Pinned by brute-force enumeration in test_ctc_align_long_cpu.py.
"""
import numpy as np

import ctc_align_reference as R


def free_emissions(logp, ext, free_start, free_end):
    """R.emissions with column 0 / S-1 set to 0"""
    em = R.emissions(logp, ext)
    if free_start:
        em[:, 0] = 0
    if free_end:
        em[:, -1] = 0
    return em


def align_free(logp, target, blank, free_start=False, free_end=False, dtype=np.float64):
    """R.align's dict for `target` through logp [T, V] with the free columns; one rounding per step in `dtype`"""
    logp = np.asarray(logp, dtype=dtype)
    T = logp.shape[0]
    ext = R.extended(target, blank)
    S, L = len(ext), len(target)
    none = dict(path=None, tok_start=None, tok_end=None, frame_logp=None, score=-np.inf)
    if T <= 0:
        return none
    em = free_emissions(logp, ext, free_start, free_end)
    skip = R.skip_allowed(ext, blank)
    ninf = dtype(-np.inf)
    v = np.full(S, ninf, dtype=dtype)
    v[:2] = em[0, :2]
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        best, code = v.copy(), np.zeros(S, dtype=np.int8)
        p1 = np.concatenate(([ninf], v[:-1]))
        take = p1 > best
        best[take], code[take] = p1[take], 1
        p2 = np.concatenate(([ninf, ninf], v[:-2]))[:S]
        take = skip & (p2 > best)
        best[take], code[take] = p2[take], 2
        v = (best + em[t]).astype(dtype)
        back[t] = code
    s = S - 1
    if S > 1 and v[S - 2] > v[S - 1]:
        s = S - 2
    if not v[s] > -np.inf:
        return none
    score = v[s]
    path = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        s -= int(back[t, s])
    tok_start, tok_end = R.spans(path, L)
    return dict(path=path, tok_start=tok_start, tok_end=tok_end, frame_logp=em[np.arange(T), path], score=score)


def path_score_free(logp, target, blank, path, free_start, free_end):
    """float64 log-probability of a given state path, the free columns counted as 0 (R.path_score with them zeroed)"""
    em = free_emissions(np.asarray(logp, dtype=np.float64), R.extended(target, blank), free_start, free_end)
    return float(em[np.arange(len(path)), np.asarray(path)].sum())


def planted_case(seed, V=32):
    """(logits f32 [T, V], target, runs): a head and a tail of 5 .. 59 frames that favour ids 16 .. 31 (ids the text lacks); between
    them the labels, drawn from ids 1 .. 15, each held for 1 .. 3 frames with +8 on the planted id; runs[l] = (first frame, one past
    the last) of label l.  Blank is id 0."""
    rs = np.random.RandomState(seed)
    head, tail = int(rs.randint(5, 60)), int(rs.randint(5, 60))
    L = int(rs.randint(2, 13))
    target, runs, ids = [], [], []
    t = head
    for _ in range(L):
        lab = int(rs.randint(1, 16))
        if target and lab == target[-1]:  # a repeat needs a blank frame between the two runs
            ids.append(0)
            t += 1
        n = int(rs.randint(1, 4))
        target.append(lab)
        runs.append((t, t + n))
        ids += [lab] * n
        t += n
    T = t + tail
    x = rs.randn(T, V).astype(np.float32)
    for f in list(range(head)) + list(range(T - tail, T)):
        x[f, int(rs.randint(16, 32))] += 8.0
    for i, lab in enumerate(ids):
        x[head + i, lab] += 8.0
    return x, target, runs


def planted_ok(res, runs):
    """the planted-path property: every label's span inside its planted run, every label but the first and last exactly its run"""
    if res["path"] is None:
        return False
    for l, (a, b) in enumerate(runs):
        s, e = int(res["tok_start"][l]), int(res["tok_end"][l])
        if not (a <= s < e <= b):
            return False
        if 0 < l < len(runs) - 1 and (s, e) != (a, b):
            return False
    return True
