"""Float64 NumPy reference of attention rescoring (js2t_rescore, include/joeys2t_hip.h), the inputs of the GPU tests and their pinned
seeds.  No GPU, no torch.

Semantics (natural logarithms).  R = B * N hypotheses, N slots per utterance; logits [R, Lp, V], row (r, l) = the distribution after l
labels.  gold(r, l) = ids[r, l] for l < n[r] and eos for l == n[r]: the LENGTH decides, no id is a sentinel.
    tok_lp[r, l] = logits[r, l, gold] - lse(logits[r, l, :]) for l <= n[r] (-inf where gold is outside 0 .. V-1), 0 behind that
    att[r]       = the sum of tok_lp[r, 0 .. n[r]]
    score[r]     = w * ctc[r] + (1 - w) * att[r], a term whose weight is exactly 0 left out (w = 1: ctc, w = 0: att)
A slot is dead if ctc = -inf, n < 0 or n > Lp - 1: att = score = -inf, tok_lp all 0; nothing of its logits or ids is read.
order[b] = the slots of utterance b by score descending, equal scores in slot order, a NaN ranked as -inf: always a permutation.

Margin.  The f32 kernel and this reference may order two nearly equal scores differently, so an input's order is compared exactly
only where the input is DECIDABLE (ctc_beam_reference): the smallest gap between adjacent finite combined scores of an utterance is
at least 4 tolerances, the tolerance being ctc_beam_reference.bound (1e-4 max(1, |score|), the project's budget for accumulated
log-likelihoods).
"""
import functools

import numpy as np

from ctc_beam_reference import DECIDABLE, bf16_round, bound  # noqa: F401  (one statement of the tolerance)

NEG = -np.inf


def dead_slots(n, ctc, Lp):
    n, ctc = np.asarray(n), np.asarray(ctc, dtype=np.float64)
    return (ctc == NEG) | (n < 0) | (n > Lp - 1)


def token_log_probs(logits, ids, n, ctc, eos):
    """tok_lp f64 [R, Lp]; reads the logits of live rows at positions <= n and ids at positions < n only"""
    R, Lp, V = logits.shape
    dead = dead_slots(n, ctc, Lp)
    out = np.zeros((R, Lp), dtype=np.float64)
    for r in range(R):
        if dead[r]:
            continue
        for l in range(int(n[r]) + 1):
            g = int(ids[r, l]) if l < n[r] else int(eos)
            if not 0 <= g < V:
                out[r, l] = NEG
                continue
            x = np.asarray(logits[r, l], dtype=np.float64)
            m = x.max()
            out[r, l] = x[g] - (m + np.log(np.exp(x - m).sum()))
    return out


def combine(ctc, att, w):
    if w == 1:
        return float(ctc)
    if w == 0:
        return float(att)
    return w * float(ctc) + (1 - w) * float(att)


def rank(scores):
    """slots by score descending, equal scores in slot order, NaN as -inf"""
    key = [NEG if s != s else s for s in scores]
    return sorted(range(len(key)), key=lambda k: (-key[k], k))


def rescore(logits, ids, n, ctc, N, eos, w):
    """(tok_lp [R, Lp], att [R], score [R], order [B, N]) in float64 / int64"""
    logits = np.asarray(logits)
    R, Lp, V = logits.shape
    assert R % N == 0
    ids, n, ctc = np.asarray(ids).reshape(R, -1), np.asarray(n).reshape(R), np.asarray(ctc, dtype=np.float64).reshape(R)
    dead = dead_slots(n, ctc, Lp)
    tok = token_log_probs(logits, ids, n, ctc, eos)
    att = np.full(R, NEG)
    score = np.full(R, NEG)
    with np.errstate(invalid="ignore"):
        for r in range(R):
            if not dead[r]:
                a = 0.0
                for l in range(int(n[r]) + 1):
                    a += tok[r, l]
                att[r] = a
                score[r] = combine(ctc[r], a, w)
    order = np.array([rank(score[b * N:(b + 1) * N].tolist()) for b in range(R // N)], dtype=np.int64).reshape(R // N, N)
    return tok, att, score, order


def margin(scores):
    """the smallest gap between adjacent finite scores of ONE utterance, in units of `bound` (the larger of the two); inf for fewer
    than two finite scores"""
    s = sorted((float(v) for v in scores if np.isfinite(v)), reverse=True)
    return min(((hi - lo) / max(bound(hi), bound(lo)) for hi, lo in zip(s, s[1:])), default=np.inf)


# ---------------------------------------------------------------- the inputs of the GPU tests
EOS = 3
WEIGHTS = (0.3, 0.5)  # every pinned case is decidable at both
# name: B, N, Lp, V, seed base, bf16-rounded logits, planted slots.  T (the row length of the id table) = Lp + 1: one more than
# the kernel may ever read.  SEEDS holds, per case, the first seed from its base that is decidable at every weight of WEIGHTS.
CASES = {
    "v11": dict(B=2, N=4, Lp=5, V=11, base=100),           # the element-wise path
    "v20": dict(B=2, N=4, Lp=5, V=20, base=200),           # 16-byte rows, one chunk per lane at most
    "v5000": dict(B=2, N=3, Lp=4, V=5000, base=300),       # the f32 16-byte path, every unroll depth
    "v5003": dict(B=2, N=3, Lp=4, V=5003, base=400),       # a vector-sized V whose rows are not all aligned, and a tail chunk
    "bf16_4096": dict(B=2, N=3, Lp=4, V=4096, base=500, bf16=True),
    "bf16_4100": dict(B=2, N=3, Lp=4, V=4100, base=600, bf16=True),
    "n1": dict(B=3, N=1, Lp=4, V=20, base=700),
    "n5": dict(B=2, N=5, Lp=6, V=37, base=800),
    "n32": dict(B=2, N=32, Lp=4, V=20, base=900),
    "lp1": dict(B=2, N=4, Lp=1, V=20, base=1000),          # every hypothesis empty: only EOS is scored
    "ragged": dict(B=3, N=5, Lp=9, V=20, base=1100, planted=True),
}
SEEDS = {"v11": 100, "v20": 200, "v5000": 300, "v5003": 400, "bf16_4096": 500, "bf16_4100": 600, "n1": 700, "n5": 800, "n32": 902,
         "lp1": 1000, "ragged": 1100}


def case_inputs(name, seed=None):
    """dict(logits f32 [R, Lp, V] (bf16-representable for a bf16 case), ids i64 [B, N, T], n i32 [B, N], ctc f32 [B, N]): logits
    randn * 4, random labels anywhere in the vocabulary (pad and EOS included), random lengths, CTC scores random negatives of the
    magnitude of the attention sums (so that the weight matters).  The planted case has, in utterance 0: slot 0 with n = Lp - 1, slot 1
    with n = 0, slot 2 dead by ctc = -inf, slot 3 dead by n = Lp; in utterance 1 a slot dead by n = -1."""
    c = CASES[name]
    seed = SEEDS[name] if seed is None else seed
    rs = np.random.RandomState(seed)
    B, N, Lp, V = c["B"], c["N"], c["Lp"], c["V"]
    R, T = B * N, Lp + 1
    logits = (rs.randn(R, Lp, V) * 4.0).astype(np.float32)
    if c.get("bf16"):
        logits = bf16_round(logits)
    ids = rs.randint(0, V, size=(B, N, T)).astype(np.int64)
    n = rs.randint(0, Lp, size=(B, N)).astype(np.int32)
    per_token = np.log(V) + 8.0  # about lse - a random logit for randn * 4
    if c.get("planted"):
        n[0, 0], n[0, 1], n[0, 3], n[1, 2] = Lp - 1, 0, Lp, -1
    ctc = (-rs.uniform(0.5, 1.5, size=(B, N)) * (np.clip(n, 0, Lp - 1) + 1) * per_token).astype(np.float32)
    if c.get("planted"):
        ctc[0, 2] = NEG
    return dict(logits=logits, ids=ids, n=n, ctc=ctc)


def run_case(name, w, seed=None):
    c = CASES[name]
    x = case_inputs(name, seed)
    return rescore(x["logits"], x["ids"], x["n"], x["ctc"], c["N"], EOS, w)


@functools.lru_cache(maxsize=None)
def case_reference(name, w):
    """the pinned case's reference result at weight w, computed once per process and shared by the tests: do not modify"""
    return run_case(name, w)


def case_margin(name, w, seed=None):
    """the smallest margin over the utterances of the case at weight w"""
    N = CASES[name]["N"]
    score = run_case(name, w, seed)[2] if seed is not None else case_reference(name, w)[2]
    return min(margin(score[b * N:(b + 1) * N]) for b in range(CASES[name]["B"]))


def find_seed(name, tries=64):
    """how SEEDS was made: the first seed from the case's base at which every utterance is decidable at every weight of WEIGHTS;
    None if `tries` seeds give none"""
    for seed in range(CASES[name]["base"], CASES[name]["base"] + tries):
        if all(case_margin(name, w, seed) >= DECIDABLE for w in WEIGHTS):
            return seed
    return None
