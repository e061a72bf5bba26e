"""Float64 NumPy reference of minimum-Bayes-risk ranking (js2t_mbr_rescore, js2t_edit_distance, include/joeys2t_hip.h), the inputs of
the GPU tests and their pinned seeds.  No GPU, no torch.

Semantics.  R = B * N hypotheses, N slots per utterance; ids [R, T], label counts n [R], scores [R] (natural logarithms).
    dead        = score -inf, n < 0, n > Lp - 1 (the rule of the list), or a score that is NaN or +inf (no log mass)
    dist[b,i,j] = the unit-cost Levenshtein distance of the labels of live i, j (full 64-bit ids); -1 in the row and the column of a
                  dead slot, the diagonal included
    posterior   = softmax over the live slots of z = scale * score, z rounded to f32 as the kernel's is; 0 for a dead slot
    risk[i]     = sum over live j of posterior[j] * dist[i, j]; +inf for a dead slot
    order[b]    = the slots by ASCENDING risk, equal risks in slot order, dead slots last in slot order: always a permutation

Margin.  The f32 kernel and this reference may order two nearly equal risks differently, so an input's order is compared exactly only
where the input is DECIDABLE (ctc_beam_reference): the smallest gap between adjacent finite risks of an utterance is at least 4
tolerances, the tolerance being ctc_beam_reference.bound (1e-4 max(1, |risk|), the project's one statement of it).  Slots that are
MEANT to tie (identical rows with identical scores) have risks that are equal in exact arithmetic; the kernel's are equal bit for
bit, because both sum the same products in the same order, and `margin` leaves gaps of exactly 0 out.
"""
import functools

import numpy as np

from ctc_beam_reference import DECIDABLE, bound  # noqa: F401  (one statement of the tolerance)

NEG = -np.inf
EDIT_MAX_LEN = 2047  # JS2T_EDIT_MAX_LEN of the header (test_mbr_cpu.py checks that the two agree)


def edit_distance(a, b):
    """unit-cost Levenshtein distance of two id sequences: an integer DP, one row of the table at a time.  The row's recurrence
    new[j] = min(prev[j] + 1, prev[j-1] + cost, new[j-1] + 1) is evaluated without a loop over j: with c[j] = min(prev[j] + 1,
    prev[j-1] + cost), new[j] = min over k <= j of c[k] + (j - k), a running minimum of c[k] - k."""
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    nb = b.size
    j = np.arange(nb + 1, dtype=np.int64)
    prev = j.copy()
    for i in range(a.size):
        c = np.empty(nb + 1, dtype=np.int64)
        c[0] = i + 1
        c[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != a[i]))
        prev = np.minimum.accumulate(c - j) + j
    return int(prev[nb])


def dead_slots(n, score, Lp):
    n, score = np.asarray(n), np.asarray(score, dtype=np.float64)
    return (score == NEG) | (n < 0) | (n > Lp - 1) | np.isnan(score) | (score == np.inf)


def rank(risks):
    """slots by risk ascending, equal risks in slot order (dead slots carry +inf: last, in slot order)"""
    return sorted(range(len(risks)), key=lambda k: (risks[k], k))


def mbr(ids, n, score, N, Lp, scale):
    """(dist i64 [B, N, N], posterior f64 [R], risk f64 [R], order i64 [B, N]); reads ids of live slots at positions < n only"""
    n = np.asarray(n).reshape(-1)
    R = n.size
    assert R % N == 0
    B = R // N
    ids = np.asarray(ids).reshape(R, -1) if R else np.zeros((0, 0), dtype=np.int64)
    score32 = np.asarray(score, dtype=np.float32).reshape(R)
    dead = dead_slots(n, score32, Lp)
    dist = np.full((B, N, N), -1, dtype=np.int64)
    post = np.zeros(R)
    risk = np.full(R, np.inf)
    order = np.zeros((B, N), dtype=np.int64)
    for b in range(B):
        live = [k for k in range(N) if not dead[b * N + k]]
        for x, i in enumerate(live):
            dist[b, i, i] = 0
            for j in live[x + 1:]:
                ri, rj = b * N + i, b * N + j
                dist[b, i, j] = dist[b, j, i] = edit_distance(ids[ri, :n[ri]], ids[rj, :n[rj]])
        if live:
            with np.errstate(over="ignore"):
                z = np.array([np.float32(scale) * score32[b * N + k] for k in live], dtype=np.float32).astype(np.float64)
            e = np.where(z == z.max(), 1.0, np.exp(z - z.max()))
            p = e / e.sum()
            for k, pk in zip(live, p):
                post[b * N + k] = pk
            for i in live:
                risk[b * N + i] = sum(post[b * N + j] * float(dist[b, i, j]) for j in live)
        order[b] = rank(risk[b * N:(b + 1) * N].tolist())
    return dist, post, risk, order


def margin(risks):
    """the smallest non-zero gap between adjacent finite risks of ONE utterance, in units of `bound` (the larger of the two); inf for
    fewer than two distinct finite risks.  A gap of exactly 0 is a tie that slot order decides in the kernel as it does here."""
    s = sorted(float(v) for v in risks if np.isfinite(v))
    return min(((hi - lo) / max(bound(hi), bound(lo)) for lo, hi in zip(s, s[1:]) if hi != lo), default=np.inf)


# ---------------------------------------------------------------- the inputs of the GPU tests
SCALES = (1.0, 0.3)  # every pinned case is decidable at both
V = 29               # the ids of the random rows are 1 .. V-1
EDGE_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129)
HI = 1 << 40
# name: B, N, the row width T of the id table (Lp = T + 1), seed base.  SEEDS holds, per case, the first seed from its base that is
# decidable at every scale of SCALES (test_mbr_cpu.py::test_pinned_cases_are_decidable recomputes the margins).
CASES = {
    "n1": dict(B=3, N=1, T=8, base=100),
    "n2": dict(B=3, N=2, T=8, base=200),
    "n5": dict(B=2, N=5, T=8, base=300),
    "n32": dict(B=2, N=32, T=8, base=400),
    "edges": dict(B=2, N=6, T=131, base=500),
    "long": dict(B=1, N=3, T=EDIT_MAX_LEN, base=600),
    "ragged": dict(B=4, N=5, T=8, base=700),
    "consensus": dict(B=1, N=5, T=12, base=800),
    "hi_bits": dict(B=1, N=4, T=8, base=900),
}
SEEDS = {"n1": 100, "n2": 200, "n5": 300, "n32": 425, "edges": 500, "long": 600, "ragged": 700, "consensus": 800, "hi_bits": 900}


def variant(rs, base, n_edits, length=None):
    """`base` with n_edits random substitutions, insertions and deletions; with `length`, cut or filled with random ids to it"""
    row = list(base)
    for _ in range(n_edits):
        kind = rs.randint(3)
        pos = rs.randint(len(row) + 1)
        if kind == 0 and row:
            row[min(pos, len(row) - 1)] = int(rs.randint(1, V))
        elif kind == 1:
            row.insert(pos, int(rs.randint(1, V)))
        elif row:
            del row[min(pos, len(row) - 1)]
    if length is not None:
        row = row[:length] + [int(v) for v in rs.randint(1, V, size=max(length - len(row), 0))]
    return row


def _fill(ids, n, b, k, row):
    ids[b, k, :len(row)] = row
    n[b, k] = len(row)


def case_inputs(name, seed=None):
    """dict(ids i64 [B, N, T], n i32 [B, N], score f32 [B, N]).  Scores lie within a few nats of each other, so the posterior is not
    one-hot.  Ids behind a row's length are random too: nothing may depend on them."""
    c = CASES[name]
    seed = SEEDS[name] if seed is None else seed
    rs = np.random.RandomState(seed)
    B, N, T = c["B"], c["N"], c["T"]
    ids = rs.randint(1, V, size=(B, N, T)).astype(np.int64)
    n = rs.randint(0, T + 1, size=(B, N)).astype(np.int32)
    score = (-10.0 - rs.uniform(0.0, 3.0, size=(B, N))).astype(np.float32)
    if name == "edges":  # variants of one base row at the lengths where a tile ends, and one unrelated row per utterance
        for b in range(B):
            base = rs.randint(1, V, size=129).tolist()
            for k in range(N - 1):
                length = int(EDGE_LENGTHS[rs.randint(len(EDGE_LENGTHS))])
                _fill(ids, n, b, k, variant(rs, base[:length] if k % 2 else base[len(base) - length:], int(rs.randint(0, 4)), length))
            n[b, N - 1] = EDGE_LENGTHS[rs.randint(2, len(EDGE_LENGTHS))]  # (the random row it was filled with)
    elif name == "long":  # two near-duplicates at the limit, one of them a label shorter, and an unrelated row at the limit
        base = rs.randint(1, V, size=T).tolist()
        _fill(ids, n, 0, 0, base)
        _fill(ids, n, 0, 1, variant(rs, base, 5, T - 1))
        n[0, 2] = T
    elif name == "ragged":
        n[0] = [8, 0, 3, 9, 5]                 # n = Lp: dead
        score[0, 2] = NEG                      # dead by score
        n[1, 1] = -1                           # dead by a negative length
        score[1, 3] = np.nan                   # dead: no log mass
        score[1, 4] = np.inf                   # dead: no log mass
        score[2] = [NEG, np.nan, np.inf, NEG, NEG]   # an utterance all dead
        n[2, 3] = -1
        score[3, [0, 1, 3, 4]] = NEG           # a single live slot
        n[3, 2] = 4
    elif name == "consensus":  # slot 0: the best score, an outlier; slots 1 - 3: near-duplicates of one row, slightly lower scores
        base = rs.randint(1, V, size=10).tolist()
        _fill(ids, n, 0, 0, rs.randint(1, V, size=10).tolist())
        _fill(ids, n, 0, 1, base)
        _fill(ids, n, 0, 2, variant(rs, base, 1))
        _fill(ids, n, 0, 3, variant(rs, base, 1))
        _fill(ids, n, 0, 4, variant(rs, base, 4))
        score[0] = -10.0 - np.array([0.0, 0.3, 0.4, 0.5, 2.0]) - rs.uniform(0.0, 0.05, size=5)
    elif name == "hi_bits":  # rows that differ only above bit 32 of an id
        base = rs.randint(1, V, size=6)
        for k in range(N):
            row = base.copy()
            row[rs.choice(6, size=k, replace=False)] += HI * (k + 1)
            _fill(ids, n, 0, k, row.tolist())
    return dict(ids=ids, n=n, score=score)


def run_case(name, scale, seed=None):
    c = CASES[name]
    x = case_inputs(name, seed)
    return mbr(x["ids"], x["n"], x["score"], c["N"], c["T"] + 1, scale)


@functools.lru_cache(maxsize=None)
def case_reference(name, scale):
    """the pinned case's reference result at `scale`, computed once per process and shared by the tests: do not modify"""
    return run_case(name, scale)


def case_margin(name, scale, seed=None):
    """the smallest margin over the utterances of the case at `scale`"""
    N = CASES[name]["N"]
    risk = run_case(name, scale, seed)[2] if seed is not None else case_reference(name, scale)[2]
    return min(margin(risk[b * N:(b + 1) * N]) for b in range(CASES[name]["B"]))


def find_seed(name, tries=64):
    """how SEEDS was made: the first seed from the case's base at which every utterance is decidable at every scale of SCALES (and,
    for the consensus case, at which the MBR top is not slot 0 at either); None if `tries` seeds give none"""
    for seed in range(CASES[name]["base"], CASES[name]["base"] + tries):
        if all(case_margin(name, s, seed) >= DECIDABLE for s in SCALES) and \
                (name != "consensus" or all(run_case(name, s, seed)[3][0, 0] != 0 for s in SCALES)):
            return seed
    return None
