"""float64 NumPy reference of CTC forced alignment (the checker of js2t_ctc_align; imports nothing from the package).

Extended sequence of a target of L labels: ext(s) = blank for even s, target[s // 2] for odd s, S = 2 L + 1.  With the emission
lp_t(s) = log_softmax(x_t)[ext(s)] (-inf for an id outside 0..V-1):

    v_0(s) = lp_0(s) for s < 2, else -inf
    v_t(s) = lp_t(s) + max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2) if s >= 2 and ext(s) != blank and ext(s) != ext(s-2))

Tie rule: a predecessor replaces the best so far only if strictly greater, tried in the order stay, s-1, s-2; the path ends in state
S-1 unless S > 1 and v(S-2) is strictly greater.  Pinned by brute-force enumeration and a known answer in test_ctc_align_cpu.py.
"""
import numpy as np


def log_softmax(x, dtype=np.float64):
    """row-wise log-softmax of [T, V] logits in `dtype`"""
    x = np.asarray(x, dtype=dtype)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def extended(target, blank):
    ext = np.full(2 * len(target) + 1, blank, dtype=np.int64)
    ext[1::2] = np.asarray(target, dtype=np.int64)
    return ext


def skip_allowed(ext, blank):
    ok = np.zeros(len(ext), dtype=bool)
    ok[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    return ok


def emissions(logp, ext):
    """[T, S] lp_t(s); -inf where the id is outside the vocabulary"""
    T, V = logp.shape
    inside = (ext >= 0) & (ext < V)
    em = np.full((T, len(ext)), -np.inf, dtype=logp.dtype)
    em[:, inside] = logp[:, ext[inside]]
    return em


def align(logp, target, blank, dtype=np.float64):
    """Best path of `target` through logp [T, V] (log-probabilities; T may be 0).  Returns a dict: path i64[T], tok_start / tok_end
    i64[L], frame_logp [T], score - or, for an utterance without a path, score = -inf and path / tok_start / tok_end = None."""
    logp = np.asarray(logp, dtype=dtype)
    T = logp.shape[0]
    ext = extended(target, blank)
    S, L = len(ext), len(target)
    none = dict(path=None, tok_start=None, tok_end=None, frame_logp=None, score=-np.inf)
    if T <= 0:
        return none
    em = emissions(logp, ext)
    skip = skip_allowed(ext, blank)
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
    tok_start, tok_end = spans(path, L)
    return dict(path=path, tok_start=tok_start, tok_end=tok_end, frame_logp=em[np.arange(T), path], score=score)


def spans(path, L):
    """first frame of every label and one past its last, from a path over the extended states"""
    tok_start, tok_end = np.full(L, -1, dtype=np.int64), np.full(L, -1, dtype=np.int64)
    for t, s in enumerate(path):
        if s & 1:
            if tok_start[s >> 1] < 0:
                tok_start[s >> 1] = t
            tok_end[s >> 1] = t + 1
    return tok_start, tok_end


def path_score(logp, target, blank, path):
    """float64 log-probability of a given state path"""
    em = emissions(np.asarray(logp, dtype=np.float64), extended(target, blank))
    return float(em[np.arange(len(path)), np.asarray(path)].sum())


def check_path(path, target, blank):
    """structural invariants of a state path for `target`; raises AssertionError naming the first one broken"""
    path = np.asarray(path, dtype=np.int64)
    ext = extended(target, blank)
    S = len(ext)
    skip = skip_allowed(ext, blank)
    assert len(path) > 0 and path[0] in (0, 1), f"start state {path[:1]}"
    assert path[-1] in (S - 1, S - 2) and path[-1] >= 0, f"end state {path[-1]} of {S}"
    assert path.min() >= 0 and path.max() < S, "state out of range"
    step = np.diff(path)
    assert ((step >= 0) & (step <= 2)).all(), f"steps {sorted(set(step.tolist()))}"
    two = np.nonzero(step == 2)[0]
    assert skip[path[two + 1]].all(), "a skip where none is allowed"
    assert collapse(ext[path], blank) == [int(v) for v in target], "collapsed labels differ from the target"


def collapse(labels, blank):
    """CTC collapse of frame labels: merge repeats, drop blanks"""
    out, prev = [], None
    for v in labels:
        v = int(v)
        if v != prev and v != blank:
            out.append(v)
        prev = v
    return out
