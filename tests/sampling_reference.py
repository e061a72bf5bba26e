"""Float64 restatement of js2t_sample_step's rule (include/joeys2t_hip.h): the checker of the sampling kernel - the reference project
has no sampling.  `ref` draws ONE row; `CASES` / `SEEDS` / `case_inputs` pin the inputs of the GPU tests the way the sibling
reference modules do: every seed is the first from its base on which EVERY row of the case is decidable.

Tolerances.  Log-probabilities and scores: the project's 1e-4 * max(1, |x|) (`bound`).  Normalised masses (out_cdf, the nucleus
sum): TAU_MASS = 2e-5 - a blocked f32 scan of at most 256 sequential additions per thread plus 8 tree levels and the exp / argument
roundings is bounded by about 280 * 2^-24 = 1.7e-5 relative.  (The kernel sums 2^-40 fixed-point integers, which leaves the exp and
argument roundings only; the bound is the contract's, not the implementation's.)  Decidable, by the project's practice of 4
tolerances: u at least 4 * TAU_MASS from both ends of the chosen interval; for top_p < 1 the two cumulative sums around the cut at
least 4 * TAU_MASS from top_p; for epsilon > 0 |q0_v / epsilon - 1| >= 4e-4 for every eligible v."""
import functools

import numpy as np

from ctc_beam_reference import bound  # noqa: F401  (one statement of the tolerance)

NEG = -np.inf
TAU_MASS = 2e-5
EPS_REL = 4e-4
U_MAX = float(np.nextafter(np.float32(1), np.float32(0)))  # u is clamped into [0, 1)
EOS, PAD = 2, 1  # of the pinned cases
MAX_V = 65536


def clamp_u(u):
    u = float(u)
    return 0.0 if np.isnan(u) else min(max(u, 0.0), U_MAX)


def ref(row, u, T=1.0, k=0, p=1.0, eps=0.0, forbid=()):
    """One live row.  Returns a dict: id (None: nothing eligible - the eos rule), logp, q, kept (the count j), cdf (lo, hi), order (the
    kept ids in the order pi), n_a / n_eps / n_k / n0, and the margins u_margin, p_margin (in normalised mass) and eps_margin
    (relative)."""
    x = np.asarray(row, dtype=np.float64).copy()
    x[np.isnan(x)] = NEG
    m = x.max()
    lse = NEG if m == NEG else m + np.log(np.exp(x - m).sum())
    xa = x.copy()
    xa[[f for f in forbid if 0 <= f < len(x)]] = NEG
    A = np.nonzero(xa > NEG)[0]
    if len(A) == 0:
        return dict(id=None, logp=NEG, q=0.0, kept=0, cdf=(0.0, 0.0), order=np.zeros(0, np.int64), n_a=0, u_margin=np.inf,
                    p_margin=np.inf, eps_margin=np.inf)
    pi = A[np.lexsort((A, -xa[A]))]  # raw logit descending, id ascending among equals
    z = xa / T
    zmax = z[pi[0]]
    e = np.exp(z[pi] - zmax)
    q0 = e / e.sum()
    n_eps = max(1, int((q0 >= eps).sum()))
    n_k = len(A) if k == 0 else min(int(k), len(A))
    n0 = min(n_eps, n_k)
    cum = np.cumsum(e[:n0])
    if p == 1.0:
        j, p_margin = n0, np.inf
    else:
        j = int(np.argmax(cum >= p * cum[-1])) + 1
        below = cum[j - 2] / cum[-1] if j >= 2 else 0.0
        p_margin = min(p - below, cum[j - 1] / cum[-1] - p)
    kept = np.sort(pi[:j])
    ek = np.exp(z[kept] - zmax)
    C = np.cumsum(ek)
    W = C[-1]
    uu = clamp_u(u)
    over = C > uu * W
    i = int(np.argmax(over)) if over.any() else len(kept) - 1
    lo, hi = (C[i] - ek[i]) / W, C[i] / W
    eps_margin = float(np.abs(q0 / eps - 1.0).min()) if eps > 0 else np.inf
    return dict(id=int(kept[i]), logp=float(x[kept[i]] - lse), q=float(np.log(ek[i] / W)), kept=j, cdf=(float(lo), float(hi)), order=pi[:j],
                n_a=len(A), n_eps=n_eps, n_k=n_k, n0=n0, u_margin=float(min(uu - lo, hi - uu)), p_margin=float(p_margin),
                eps_margin=eps_margin)


def decidable(r):
    return r["u_margin"] >= 4 * TAU_MASS and r["p_margin"] >= 4 * TAU_MASS and r["eps_margin"] >= EPS_REL


# ---------------------------------------------------------------- the pinned cases
CASES = {
    "tiny": dict(V=11, scale=2.0, T=1.0, k=0, p=1.0, eps=0.0, rows=64, n_forbid=1, base=100),
    "tiny_all": dict(V=11, scale=2.0, T=0.7, k=5, p=0.9, eps=0.05, rows=64, n_forbid=2, base=200, special=True),
    "k1": dict(V=37, scale=2.0, T=1.0, k=1, p=1.0, eps=0.0, rows=16, n_forbid=0, base=300),
    "v5000": dict(V=5000, scale=5.0, T=1.0, k=0, p=1.0, eps=0.0, rows=32, n_forbid=3, base=400),
    "v5000_k": dict(V=5000, scale=4.0, T=1.0, k=50, p=1.0, eps=0.0, rows=32, n_forbid=2, base=500),
    "v5000_p": dict(V=5000, scale=5.0, T=1.0, k=0, p=0.9, eps=0.0, rows=32, n_forbid=1, base=600),
    "eps": dict(V=5000, scale=5.0, T=1.0, k=0, p=1.0, eps=0.02, rows=32, n_forbid=3, base=700),
    "v5003_all": dict(V=5003, scale=5.0, T=0.8, k=40, p=0.95, eps=0.005, rows=32, n_forbid=3, base=800, special=True),
    "v10000_p": dict(V=10000, scale=6.0, T=1.3, k=0, p=0.9, eps=0.0, rows=16, n_forbid=2, base=900),
    "vmax": dict(V=65536, scale=7.0, T=1.0, k=64, p=0.9, eps=0.0, rows=4, n_forbid=3, base=1000),
}
SEEDS = {"tiny": 100, "tiny_all": 200, "k1": 300, "v5000": 401, "v5000_k": 500, "v5000_p": 604, "eps": 700, "v5003_all": 801,
         "v10000_p": 902, "vmax": 1000}
FINISHED_ROWS = (3, 10)  # of the `special` cases


def case_inputs(name, seed=None):
    """dict(logits f32 [rows, V], u f32 [rows], finished u8 [rows], forbid [ids], score f32 [rows], length i32 [rows]) and the case's
    parameters.  `special` cases carry finished rows (their logits and u poisoned with NaN) and rows with -inf / NaN entries: row 1 a
    quarter -inf, row 5 NaN entries, row 7 all but three ids -inf."""
    c = CASES[name]
    rs = np.random.RandomState(SEEDS[name] if seed is None else seed)
    V, rows = c["V"], c["rows"]
    logits = (c["scale"] * rs.randn(rows, V)).astype(np.float32)
    u = rs.rand(rows).astype(np.float32)
    forbid = sorted(int(v) for v in rs.choice(np.arange(3, V), c["n_forbid"], replace=False))
    finished = np.zeros(rows, np.uint8)
    if c.get("special"):
        logits[1, rs.choice(V, V // 4, replace=False)] = NEG
        logits[5, rs.choice(V, max(V // 8, 2), replace=False)] = np.nan
        alive = rs.choice(V, 3, replace=False)
        dead = np.ones(V, bool)
        dead[alive] = False
        logits[7, dead] = NEG
        for r in FINISHED_ROWS:
            finished[r] = 1
            logits[r] = np.nan
            u[r] = np.nan
    score = rs.randn(rows).astype(np.float32)
    length = rs.randint(0, 7, rows).astype(np.int32)
    return dict(c, logits=logits, u=u, finished=finished, forbid=forbid, score=score, length=length)


def run_case(name, seed=None):
    """[ref(...) per row; None for a finished row]"""
    c = case_inputs(name, seed)
    return [None if c["finished"][r] else ref(c["logits"][r], c["u"][r], c["T"], c["k"], c["p"], c["eps"], c["forbid"])
            for r in range(c["rows"])]


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """the pinned case's reference result, computed once per process and shared by the tests: do not modify"""
    return run_case(name)


def case_decidable(name, seed=None):
    return all(r is None or decidable(r) for r in run_case(name, seed))


def find_seed(name, tries=64):
    """how SEEDS was made: the first seed from the case's base on which every row is decidable; None if `tries` seeds give none"""
    for seed in range(CASES[name]["base"], CASES[name]["base"] + tries):
        if case_decidable(name, seed):
            return seed
    return None


def brute_force_kept(row, T, k, p, eps, forbid=()):
    """the kept set by "sort, renormalise, cut", written independently of `ref`: a Python sort of (-logit, id) pairs, then the three
    filters one after the other, each on the renormalised survivors of the one before"""
    pairs = sorted((-float(x), v) for v, x in enumerate(row) if v not in forbid and not np.isnan(x) and float(x) > NEG)
    if not pairs:
        return []
    top = -pairs[0][0] / T
    mass = [np.exp(-nx / T - top) for nx, _ in pairs]
    total = sum(mass)
    by_eps = [i for i in range(len(pairs)) if mass[i] / total >= eps] or [0]
    survivors = by_eps if k == 0 else by_eps[:k]
    if p < 1.0:
        sub = sum(mass[i] for i in survivors)
        run, cut = 0.0, len(survivors)
        for n, i in enumerate(survivors):
            run += mass[i]
            if run >= p * sub:
                cut = n + 1
                break
        survivors = survivors[:cut]
    return [pairs[i][1] for i in survivors]
