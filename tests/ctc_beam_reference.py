"""Float64 NumPy reference of CTC prefix beam search (js2t_ctc_beam_search, include/joeys2t_hip.h), the brute-force enumeration
that pins it, the planted inputs of the GPU tests and their pinned seeds.  No GPU, no torch.

Semantics (natural logarithms).  Per frame the candidates are the C largest raw logits among the labels (value descending, id
ascending, blank excluded - js2t_beam_pick's order); the distribution of the frame is truncated to them and the blank.  The beam
starts as {(): pb = 0, pnb = -inf}; per frame, for every prefix y of the beam, tot = lae(pb, pnb), e = its last label:
    next[y].pb += tot + lp(blank);  for every candidate (c, lp):
    c == e: next[y].pnb += pnb + lp and next[y + c].pnb += pb + lp (skipped when pb = -inf);  else: next[y + c].pnb += tot + lp
`next` is a dict keyed by the token TUPLE; the K entries with the largest lae(pb, pnb) are the new beam.

Margin.  An f32 kernel and this reference may legitimately prune differently where two scores nearly tie, so every result carries
its margin: the minimum, over frames, of (K-th kept score - best dropped score) and, at the end, of the gaps between neighbouring
scores among the first n_best + 1, each gap divided by TOL * max(1, |score|) (the larger magnitude of the two).  TOL = 1e-4 is the
project's budget for accumulated log-likelihoods (tests/test_hip_ctc_align.py) and the score tolerance of the GPU tests.  An input
is DECIDABLE when its margin is >= 4: two scores each wrong by the full tolerance in opposite directions close a gap of 2, the
factor 2 on top is slack.  On a decidable input a kernel within tolerance makes exactly the reference's decisions.
"""
import functools
import itertools

import numpy as np

NEG = -np.inf
TOL = 1e-4
DECIDABLE = 4.0


def lae(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = max(a, b)
    return m + np.log1p(np.exp(min(a, b) - m))


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def candidates(logits, C, blank):
    """ids [T, C] of the C largest logits of every frame among the labels: value descending, id ascending among equal values"""
    logits = np.asarray(logits, dtype=np.float64)
    T, V = logits.shape
    assert 1 <= C <= V - 1
    out = np.zeros((T, C), dtype=np.int64)
    for t in range(T):
        order = sorted((v for v in range(V) if v != blank), key=lambda v: (-logits[t, v], v))
        out[t] = order[:C]
    return out


def bound(score):
    return TOL * max(1.0, abs(score))


def _gap_units(hi, lo):
    """(hi - lo) in units of the tolerance; two -inf scores do not separate"""
    if hi == NEG and lo == NEG:
        return 0.0
    if lo == NEG:
        return np.inf
    return (hi - lo) / (TOL * max(1.0, abs(hi), abs(lo)))


def beam_search(logits, K, C, n_best, blank, identity="sequence"):
    """logits [T_b, V] (raw; the frames of ONE utterance).  Returns (hyps, margin): hyps = the n_best best (tuple, score), best first.
    identity = "node": the variant that identifies a prefix by its trie node (parent node, token) - nodes exist only for members of
    the beam, so a prefix that was pruned and is created again is a NEW node and its extensions no longer meet the surviving
    children of the old one.  It is here to show that the pinned identity case tells the two apart."""
    logits = np.asarray(logits, dtype=np.float64)
    T = logits.shape[0]
    lp = log_softmax(logits) if T else logits
    cand = candidates(logits, C, blank) if T else None
    beam = [dict(seq=(), pb=0.0, pnb=NEG, node=0, parent=-1)]
    n_nodes = 1
    margin = np.inf
    for t in range(T):
        nxt = {}

        def add(key, seq, which, v, parent):
            ent = nxt.setdefault(key, dict(seq=seq, pb=NEG, pnb=NEG, parent=parent))
            ent[which] = lae(ent[which], v)

        for ent in beam:
            y, pb, pnb = ent["seq"], ent["pb"], ent["pnb"]
            tot = lae(pb, pnb)
            e = y[-1] if y else None
            stay = y if identity == "sequence" else ent["node"]
            add(stay, y, "pb", tot + lp[t, blank], ent["parent"])
            for c in cand[t].tolist():
                v = lp[t, c]
                if v == NEG:
                    continue
                if identity == "sequence":
                    ext = y + (c, )
                else:
                    child = [o["node"] for o in beam if o["parent"] == ent["node"] and o["seq"][-1] == c]
                    ext = child[0] if child else ("new", ent["node"], c)
                if c == e:
                    add(stay, y, "pnb", pnb + v, ent["parent"])
                    if pb != NEG:
                        add(ext, y + (c, ), "pnb", pb + v, ent["node"])
                else:
                    add(ext, y + (c, ), "pnb", tot + v, ent["node"])
        ranked = sorted(nxt.items(), key=lambda kv: -lae(kv[1]["pb"], kv[1]["pnb"]))  # (stable: dict order among equal scores)
        if len(ranked) > K:
            margin = min(margin, _gap_units(lae(ranked[K - 1][1]["pb"], ranked[K - 1][1]["pnb"]), lae(ranked[K][1]["pb"], ranked[K][1]["pnb"])))
        beam = []
        for key, ent in ranked[:K]:
            if isinstance(key, tuple) and identity == "node":
                ent["node"] = n_nodes
                n_nodes += 1
            elif identity == "node":
                ent["node"] = key
            else:
                ent["node"] = -1
            beam.append(ent)
    scores = [lae(e["pb"], e["pnb"]) for e in beam]
    order = sorted(range(len(beam)), key=lambda i: -scores[i])
    for a, b in zip(order[:n_best], order[1:n_best + 1]):
        margin = min(margin, _gap_units(scores[a], scores[b]))
    return [(beam[i]["seq"], scores[i]) for i in order[:n_best]], float(margin)


def collapse(path, blank):
    out = []
    prev = None
    for v in path:
        if v != prev and v != blank:
            out.append(v)
        prev = v
    return tuple(out)


def brute_force(logits, C, blank):
    """{labelling: log-sum over all V^T frame labellings that are admissible under the truncated distribution and collapse to it}"""
    logits = np.asarray(logits, dtype=np.float64)
    T, V = logits.shape
    lp = log_softmax(logits)
    cand = candidates(logits, C, blank)
    allowed = [set(cand[t].tolist()) | {blank} for t in range(T)]
    sums = {}
    for path in itertools.product(range(V), repeat=T):
        if all(path[t] in allowed[t] for t in range(T)):
            sums.setdefault(collapse(path, blank), []).append(sum(lp[t, path[t]] for t in range(T)))
    return {k: float(np.logaddexp.reduce(np.array(v))) for k, v in sums.items()}


# ---------------------------------------------------------------- the inputs of the GPU tests
def planted_path(rs, T, V, blank):
    """a frame labelling that alternates labels (one or two frames) and blanks (one to three), the third label repeating the second"""
    labels = [v for v in range(V) if v != blank]
    path, prev, n = [], None, 0
    while len(path) < T:
        if n == 2 and prev is not None:
            lab = prev  # the immediate repeat: the same label again behind a blank
        else:
            lab = labels[rs.randint(len(labels))]
            while lab == prev and len(labels) > 1:
                lab = labels[rs.randint(len(labels))]
        path += [lab] * rs.randint(1, 3) + [blank] * rs.randint(1, 4)
        prev, n = lab, n + 1
    return np.array(path[:T])


def planted_logits(seed, B, T, V, blank=0, peak=(6.0, 8.0)):
    """f32 [B, T, V]: randn noise plus a peak on a planted frame labelling - what trained CTC posteriors look like"""
    rs = np.random.RandomState(seed)
    x = rs.randn(B, T, V)
    for b in range(B):
        path = planted_path(rs, T, V, blank)
        x[b, np.arange(T), path] += rs.uniform(peak[0], peak[1], size=T)
    return x.astype(np.float32)


def random_logits(seed, B, T, V, scale=4.0):
    return (np.random.RandomState(seed).randn(B, T, V) * scale).astype(np.float32)


def bf16_round(x):
    """f32 -> the nearest bf16 (ties to even), as f32"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


# name: generator, seed base, B, T, V, K, C, n_best, in_len, bf16-rounded input.  SEEDS holds, per case, the first seed from its
# base that is decidable (test_ctc_beam_cpu.py::test_pinned_cases_are_decidable recomputes the margins).
CASES = {
    "short": dict(gen="planted", base=100, B=3, T=33, V=11, K=4, C=3, n_best=4, in_len=(33, 20, 1)),
    "k8": dict(gen="planted", base=200, B=1, T=48, V=37, K=8, C=8, n_best=4, in_len=(48, )),
    "k16": dict(gen="planted", base=300, B=1, T=96, V=37, K=16, C=8, n_best=4, in_len=(96, )),
    "k32": dict(gen="planted", base=400, B=1, T=64, V=37, K=32, C=8, n_best=4, in_len=(64, )),
    "long_k2": dict(gen="planted", base=500, B=1, T=375, V=37, K=2, C=2, n_best=2, in_len=(375, )),
    "long_k1": dict(gen="planted", base=600, B=1, T=375, V=37, K=1, C=8, n_best=1, in_len=(375, )),
    "identity": dict(gen="random", base=700, B=1, T=10, V=3, K=3, C=2, n_best=3, in_len=(10, )),
    "bf16": dict(gen="planted", base=800, B=2, T=48, V=37, K=8, C=8, n_best=4, in_len=(48, 31), bf16=True),
}
SEEDS = {"short": 100, "k8": 201, "k16": 300, "k32": 400, "long_k2": 500, "long_k1": 600, "identity": 719, "bf16": 800}
BLANK = 0


def case_logits(name, seed=None):
    c = CASES[name]
    seed = SEEDS[name] if seed is None else seed
    x = planted_logits(seed, c["B"], c["T"], c["V"], BLANK) if c["gen"] == "planted" else random_logits(seed, c["B"], c["T"], c["V"])
    return bf16_round(x) if c.get("bf16") else x


def run_case(name, seed=None, identity="sequence"):
    """[(hyps, margin)] per utterance of the case"""
    c = CASES[name]
    x = case_logits(name, seed)
    return [beam_search(x[b, :min(c["in_len"][b], c["T"])], c["K"], c["C"], c["n_best"], BLANK, identity) for b in range(c["B"])]


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """the pinned case's reference result, computed once per process and shared by the tests: do not modify"""
    return run_case(name)


def differs(res_a, res_b):
    """do two results of run_case differ by more than rounding: other labellings, or scores further apart than the tolerance?"""
    for (ha, _), (hb, _) in zip(res_a, res_b):
        if [y for y, _ in ha] != [y for y, _ in hb] or any(abs(u - v) > bound(u) for (_, u), (_, v) in zip(ha, hb)):
            return True
    return False


def find_seed(name, tries=64):
    """how SEEDS was made: the first seed from the case's base whose every utterance is decidable (and, for the identity case, on
    which the node-identity variant returns something else); None if `tries` seeds give none"""
    for seed in range(CASES[name]["base"], CASES[name]["base"] + tries):
        res = run_case(name, seed)
        if min(m for _, m in res) >= DECIDABLE and (name != "identity" or differs(res, run_case(name, seed, "node"))):
            return seed
    return None
