"""Float64 NumPy reference of n-gram LM rescoring (js2t_ngram_rescore, include/joeys2t_hip.h): a dict-based scorer of the back-off
rule with the combine and rank rules, a generator of NORMALISED back-off LMs, a pure-Python emulation of the device table's probe
rule, the inputs of the GPU tests and their pinned seeds.  No GPU, no torch.

Semantics (natural logarithms).  An LM is a dict {(id, ..): (logp, backoff)} holding every unigram.  R = B * N hypotheses, N slots
per utterance.  gold(r, l) = ids[r, l] for l < n[r] and eos for l == n[r]: the LENGTH decides.  The history of position l is
(bos, ids[r, :l]); its last order - 1 tokens are the context, cut behind the newest id outside 0 .. V-1.
    p(w | ctx): acc = 0; for k = len(ctx) .. 1: (ctx[-k:], w) stored -> acc + its logp; else acc += backoff of ctx[-k:] if stored
                (else 0); no match: acc + logp of (w,); w outside 0 .. V-1: -inf
    lm_tok[r, l] = that for l <= n[r], 0 behind;  lm[r] = the sum of lm_tok[r, 0 .. n[r]]
    score[r]     = base[r] + lm_weight * lm[r] + length_bonus * n[r], a term whose weight is exactly 0 left out; with lm_weight 0 the
                   model is left out altogether (lm_tok = 0, lm = 0)
A slot is dead if base = -inf, n < 0 or n > Lp - 1: lm = score = -inf, lm_tok all 0, none of its ids read.
order[b] = the slots of utterance b by score descending, equal scores in slot order, a NaN ranked as -inf: always a permutation.

Margin: as in rescore_reference - orders are compared exactly only where the input is DECIDABLE (adjacent finite scores of an
utterance at least 4 tolerances apart, the tolerance ctc_beam_reference.bound = 1e-4 max(1, |score|)).
"""
import functools

import numpy as np

from ctc_beam_reference import DECIDABLE, bound  # noqa: F401  (one statement of the tolerance)
from rescore_reference import margin, rank  # noqa: F401  (one statement of the tie and NaN rules)

NEG = -np.inf
PAD, BOS, EOS = 1, 2, 3


# ---------------------------------------------------------------- the scorer
def context_of(hist, V, order):
    """the last order - 1 tokens of the history, cut behind the newest id outside 0 .. V-1"""
    ctx = []
    for t in reversed(list(hist)[-(order - 1):] if order > 1 else []):
        if not 0 <= t < V:
            break
        ctx.insert(0, int(t))
    return tuple(ctx)


def token_logp(lm, w, hist, V, order):
    if not 0 <= w < V:
        return NEG
    ctx = context_of(hist, V, order)
    acc = 0.0
    for k in range(len(ctx), 0, -1):
        c = ctx[-k:]
        hit = lm.get(c + (int(w), ))
        if hit is not None:
            return acc + hit[0]
        acc += lm.get(c, (0.0, 0.0))[1]
    return acc + lm[(int(w), )][0]


def dead_slots(n, base, Lp):
    n, base = np.asarray(n), np.asarray(base, dtype=np.float64)
    return (base == NEG) | (n < 0) | (n > Lp - 1)


def combine(base, lm_sum, n, lm_weight, length_bonus):
    s = float(base)
    if lm_weight != 0:
        s = s + lm_weight * float(lm_sum)
    if length_bonus != 0:
        s = s + length_bonus * float(n)
    return s


def rescore(ids, n, base, N, Lp, lm, V, order, bos, eos, lm_weight, length_bonus, logp=token_logp):
    """(lm_tok f64 [R, Lp], lm f64 [R], score f64 [R], order i64 [B, N]); reads the ids of live slots at positions < n only.
    logp: the token rule (the dict scorer, or the table emulation with an NGramLM in place of the dict)"""
    n, base = np.asarray(n).reshape(-1), np.asarray(base, dtype=np.float64).reshape(-1)
    R = n.shape[0]
    assert R % N == 0
    ids = np.asarray(ids).reshape(R, -1)
    dead = dead_slots(n, base, Lp)
    tok, lms, score = np.zeros((R, Lp)), np.full(R, NEG), np.full(R, NEG)
    with np.errstate(invalid="ignore"):
        for r in range(R):
            if dead[r]:
                continue
            a = 0.0
            if lm_weight != 0:
                y = [int(v) for v in ids[r, :n[r]]]
                for l in range(int(n[r]) + 1):
                    tok[r, l] = logp(lm, y[l] if l < n[r] else eos, [bos] + y[:l], V, order)
                    a += tok[r, l]
            lms[r] = a
            score[r] = combine(base[r], a, n[r], lm_weight, length_bonus)
    order_out = np.array([rank(score[b * N:(b + 1) * N].tolist()) for b in range(R // N)], dtype=np.int64).reshape(R // N, N)
    return tok, lms, score, order_out


# ---------------------------------------------------------------- a normalised back-off LM
def make_lm(V, order, seed, density=0.3):
    """{(id, ..): (logp, backoff)}, natural logarithms, float64: a NORMALISED back-off LM of the given order built directly.
    Every unigram is there (probabilities summing to 1).  The (k+1)-grams are drawn among (g, w) with g a stored k-gram and
    (g[1:], w) a stored k-gram - closed under prefix and suffix, as ARPA requires - each candidate with probability `density` (a
    number, or one per order 2 ..), never all V words of one context.  Per context the explicit probabilities sum to S < 1 and
        backoff(ctx) = (1 - S) / (1 - sum over the same words of p(w | ctx[1:]))
    with p(. | ctx[1:]) the model built so far, which makes sum_w p(w | ctx) = 1 for every context, stored or not."""
    rs = np.random.RandomState(seed)
    dens = [density] * (order - 1) if np.isscalar(density) else list(density)
    p = rs.uniform(0.2, 1.0, size=V)
    p /= p.sum()
    lm = {(w, ): (float(np.log(p[w])), 0.0) for w in range(V)}
    level = sorted(lm)  # the k-grams
    for k in range(1, order):
        succ = {}  # (k-1)-gram prefix -> the last words of the k-grams that start with it
        for g in level:
            succ.setdefault(g[:-1], []).append(g[-1])
        nxt = []
        for g in level:
            cands = succ.get(g[1:], [])
            m = min(int(rs.binomial(len(cands), dens[k - 1])), V - 1) if cands else 0
            if m == 0:
                continue
            words = sorted(cands[i] for i in rs.choice(len(cands), m, replace=False))
            raw = rs.uniform(0.5, 1.5, size=m)
            S = rs.uniform(0.3, 0.8)
            q = raw / raw.sum() * S
            lower = sum(np.exp(token_logp(lm, w, g[1:], V, k)) for w in words)  # p(w | g[1:]): context of k - 1 tokens
            assert lower < 1.0
            lm[g] = (lm[g][0], float(np.log((1.0 - S) / (1.0 - lower))))
            for w, qw in zip(words, q):
                lm[g + (w, )] = (float(np.log(qw)), 0.0)
                nxt.append(g + (w, ))
        level = sorted(nxt)
    return lm


def lm_order(lm):
    return max(len(g) for g in lm)


def sample_labels(lm, V, order, rs, length, follow=0.7):
    """`length` labels: with probability `follow` a stored successor of the longest stored context (so that hits, back-offs and
    misses all occur), else any id of the vocabulary, bos / eos / pad included"""
    succ = sample_labels.cache.get(id(lm))
    if succ is None:
        succ = {}
        for g in lm:
            if len(g) > 1:
                succ.setdefault(g[:-1], []).append(g[-1])
        sample_labels.cache = {id(lm): succ}
    y = []
    for _ in range(length):
        hist = [BOS] + y
        pick = None
        if rs.uniform() < follow:
            for k in range(min(order - 1, len(hist)), 0, -1):
                c = succ.get(tuple(hist[-k:]))
                if c:
                    pick = c[rs.randint(len(c))]
                    break
        y.append(int(rs.randint(V)) if pick is None else int(pick))
    return y


sample_labels.cache = {}


# ---------------------------------------------------------------- the device table, emulated (plain Python integers)
M64 = (1 << 64) - 1


def fmix_py(z):
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def key_of(gram):
    """field j (0 = newest) = id + 1 in bits 16j .. 16j+15"""
    return sum((int(w) + 1) << (16 * j) for j, w in enumerate(reversed(gram)))


def table_lookup(t, gram):
    """(logp, backoff, slots examined) of a 2 .. order-gram in the NGramLM `t`, None in place of the values if absent: slots home,
    home + 1, ... (wrapping) until the key, an empty slot or max_probe slots"""
    key, cap = key_of(gram), t.capacity
    home = fmix_py(key) & (cap - 1)
    for i in range(t.max_probe):
        e = t.table[(home + i) & (cap - 1)]
        k = int(e["key"])
        if k == key:
            return float(e["logp"]), float(e["backoff"]), i + 1
        if k == 0:
            return None, None, i + 1
    return None, None, t.max_probe


def table_token_logp(t, w, hist, V, order):
    """token_logp over the NGramLM's arrays instead of the dict"""
    if not 0 <= w < V:
        return NEG
    ctx = context_of(hist, V, order)
    acc = 0.0
    for k in range(len(ctx), 0, -1):
        c = ctx[-k:]
        lp, _, _ = table_lookup(t, c + (int(w), ))
        if lp is not None:
            return acc + lp
        acc += float(t.uni[c[0], 1]) if k == 1 else (table_lookup(t, c)[1] or 0.0)
    return acc + float(t.uni[int(w), 0])


# ---------------------------------------------------------------- the inputs of the GPU tests
LM_WEIGHTS = (0.3, 0.7)
BONUSES = (0.0, 0.5)
COMBOS = tuple((w, b) for w in LM_WEIGHTS for b in BONUSES)  # every pinned case is decidable at all four
# name: B, N, Lp, V, the LM's order, its seed and density, the table's max_load, seed base, planted slots.  T (the row length of the
# id table) = Lp + 1: one more than the kernel may ever read.  SEEDS holds, per case, the first seed from its base that is
# decidable at every combination of COMBOS.
# 20551 n-grams, 15551 of them in the table: capacity 32768 at max_load 0.5 and 16384 at 0.97 (load 0.949, max_probe 41, 40 wrapped)
BIG = dict(V=5000, order=4, lm_seed=7, density=(0.00037, 0.3, 0.3))
CASES = {
    "o1": dict(B=2, N=4, Lp=5, V=11, order=1, lm_seed=1, density=0.3, base=100),
    "o2": dict(B=2, N=4, Lp=5, V=11, order=2, lm_seed=2, density=0.3, base=200),
    "o3": dict(B=2, N=4, Lp=5, V=11, order=3, lm_seed=3, density=0.3, base=300),
    "o4": dict(B=2, N=4, Lp=6, V=11, order=4, lm_seed=4, density=0.3, base=400),
    "n32": dict(B=2, N=32, Lp=4, V=20, order=3, lm_seed=5, density=0.2, base=500),
    "n1": dict(B=3, N=1, Lp=4, V=20, order=3, lm_seed=5, density=0.2, base=600),
    "lp1": dict(B=2, N=4, Lp=1, V=20, order=3, lm_seed=5, density=0.2, base=700),  # every hypothesis empty: only EOS is scored
    "big": dict(B=2, N=3, Lp=8, base=800, **BIG),                                  # max_load 0.5
    "big_full": dict(B=2, N=3, Lp=8, base=800, max_load=0.97, **BIG),              # long chains, wrap-around
    "ragged": dict(B=3, N=5, Lp=9, V=20, order=3, lm_seed=5, density=0.2, base=900, planted=True),
}
SEEDS = {"o1": 100, "o2": 200, "o3": 300, "o4": 400, "n32": 503, "n1": 600, "lp1": 700, "big": 800, "big_full": 800, "ragged": 900}


@functools.lru_cache(maxsize=None)
def lm_dict(V, order, lm_seed, density):
    """the LM of a case, built once per process and shared: do not modify"""
    return make_lm(V, order, lm_seed, density)


def case_lm(name):
    c = CASES[name]
    return lm_dict(c["V"], c["order"], c["lm_seed"], c["density"])


def case_inputs(name, seed=None):
    """dict(ids i64 [B, N, T], n i32 [B, N], base f32 [B, N]): labels by sample_labels up to the length and any id behind it, random
    lengths, base scores random negatives of the magnitude of the LM sums (so that the weight matters).  The planted case has, in
    utterance 0: slot 0 with n = Lp - 1, slot 1 with n = 0, slot 2 dead by base = -inf, slot 3 dead by n = Lp; in utterance 1 a slot
    dead by n = -1."""
    c = CASES[name]
    seed = SEEDS[name] if seed is None else seed
    rs = np.random.RandomState(seed)
    B, N, Lp, V = c["B"], c["N"], c["Lp"], c["V"]
    T = Lp + 1
    lm = case_lm(name)
    ids = rs.randint(0, V, size=(B, N, T)).astype(np.int64)
    n = rs.randint(0, Lp, size=(B, N)).astype(np.int32)
    if c.get("planted"):
        n[0, 0], n[0, 1], n[0, 3], n[1, 2] = Lp - 1, 0, Lp, -1
    for b in range(B):
        for k in range(N):
            m = int(np.clip(n[b, k], 0, Lp - 1))
            ids[b, k, :m] = sample_labels(lm, V, c["order"], rs, m)
    base = (-rs.uniform(0.5, 1.5, size=(B, N)) * (np.clip(n, 0, Lp - 1) + 1) * np.log(V)).astype(np.float32)
    if c.get("planted"):
        base[0, 2] = NEG
    return dict(ids=ids, n=n, base=base)


def run_case(name, lm_weight, length_bonus, seed=None):
    c = CASES[name]
    x = case_inputs(name, seed)
    return rescore(x["ids"], x["n"], x["base"], c["N"], c["Lp"], case_lm(name), c["V"], c["order"], BOS, EOS, lm_weight, length_bonus)


@functools.lru_cache(maxsize=None)
def case_reference(name, lm_weight, length_bonus):
    """the pinned case's reference result, computed once per process and shared by the tests: do not modify"""
    return run_case(name, lm_weight, length_bonus)


def case_margin(name, lm_weight, length_bonus, seed=None):
    """the smallest margin over the utterances of the case"""
    N = CASES[name]["N"]
    score = run_case(name, lm_weight, length_bonus, seed)[2] if seed is not None else case_reference(name, lm_weight, length_bonus)[2]
    return min(margin(score[b * N:(b + 1) * N]) for b in range(CASES[name]["B"]))


def find_seed(name, tries=64):
    """how SEEDS was made: the first seed from the case's base at which every utterance is decidable at every combination of
    COMBOS; None if `tries` seeds give none"""
    for seed in range(CASES[name]["base"], CASES[name]["base"] + tries):
        if all(case_margin(name, w, b, seed) >= DECIDABLE for w, b in COMBOS):
            return seed
    return None


# ---------------------------------------------------------------- the builder's pinned cases (tests/test_ngram_cpu.py)
def builder_grams(seed, count, V=50, k=3):
    """`count` distinct random k-grams over V ids with values that name them: (ids i64 [count, k], logp, backoff)"""
    rs = np.random.RandomState(seed)
    flat = rs.choice(V**k, size=count, replace=False)
    ids = np.stack([(flat // V**j) % V for j in reversed(range(k))], axis=1).astype(np.int64)
    return ids, -(1.0 + np.arange(count)).astype(np.float32), -(0.5 + np.arange(count)).astype(np.float32)


def find_builder_seed(count, max_load, want, tries=256):
    """the first seed whose table has `want`: "wrap" (a stored key in a slot below its home) or "probe4" (max_probe >= 4)"""
    from joeys2t_amd.lm import NGramLM, fmix, pack_keys
    for seed in range(tries):
        ids, lp, bo = builder_grams(seed, count)
        t = NGramLM.from_arrays(np.zeros((50, 2), dtype=np.float32), {3: (ids, lp, bo)}, max_load=max_load)
        if want == "probe4" and t.max_probe >= 4:
            return seed
        if want == "wrap":
            stored = t.table["key"] != 0
            home = (fmix(t.table["key"]) & np.uint64(t.capacity - 1)).astype(np.int64)
            if (np.nonzero(stored)[0] < home[stored]).any():
                return seed
    return None


BUILDER_WRAP = dict(count=62, max_load=0.97, seed=0)    # capacity 64: nearly full
BUILDER_PROBE4 = dict(count=40, max_load=0.7, seed=1)   # capacity 64
