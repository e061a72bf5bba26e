"""Float64 NumPy reference of CTC prefix beam search with contextual biasing inside the beam (js2t_ctc_beam_search_ctx,
include/joeys2t_hip.h), the route it is compared with, the inputs of the GPU tests and their pinned seeds.  No GPU, no torch.  It
extends ctc_beam_lm_reference.beam_search by the context term; the automaton is context_reference's.

Semantics.  Everything of ctc_beam_lm_reference; every prefix also carries the automaton's (node, bank).  Per frame
    key(y) = lae(pb, pnb) + lm_weight * lm(y) + context_weight * m(y) + length_bonus * |y|     (a term of weight 0 left out)
with m(y) = bank + depth(node); after the last frame final(y) uses ctx(y) = bank + keep(node) in place of m(y) and the LM's EOS
term.  Hypotheses are (seq, final, ctc, lm, ctx); ctx is 0 when context_weight is 0 (the graph is left out altogether).

Margin and DECIDABLE as in ctc_beam_reference.
"""
import functools

import numpy as np

import context_reference as X
import ctc_beam_lm_reference as F
import ctc_beam_reference as R
import ngram_reference as G
from ctc_beam_reference import DECIDABLE, NEG, TOL, bound, candidates, lae, log_softmax  # noqa: F401
from ngram_reference import token_logp

BLANK, BOS, EOS = F.BLANK, F.BOS, F.EOS
_gap_units = R._gap_units


def combine(base, lm, count, n, lm_weight, context_weight, length_bonus):
    s = float(base)
    if lm_weight != 0:
        s = s + lm_weight * float(lm)
    if context_weight != 0:
        s = s + context_weight * float(count)
    if length_bonus != 0:
        s = s + length_bonus * float(n)
    return s


def beam_search(logits, K, C, n_best, blank, lm, V, order, bos, eos, lm_weight, length_bonus, auto, context_weight):
    """logits [T_b, V] (raw; the frames of ONE utterance); lm: ngram_reference's dict (not read when lm_weight is 0); auto: a
    context_reference.Automaton (not read when context_weight is 0).  Returns (hyps, margin): the n_best best (tuple, final, ctc, lm,
    ctx), best first."""
    logits = np.asarray(logits, dtype=np.float64)
    T = logits.shape[0]
    lp = log_softmax(logits) if T else logits
    cand = candidates(logits, C, blank) if T else None
    use_lm, use_ctx = lm_weight != 0, context_weight != 0

    def key_of(ent):
        m = ent["bank"] + auto.depth[ent["cnode"]] if use_ctx else 0
        return combine(lae(ent["pb"], ent["pnb"]), ent["lm"], m, len(ent["seq"]), lm_weight, context_weight, length_bonus)

    beam = [dict(seq=(), pb=0.0, pnb=NEG, lm=0.0, cnode=0, bank=0)]
    margin = np.inf
    for t in range(T):
        nxt = {}

        def add(seq, which, v, lmv, cnode, bank):
            ent = nxt.setdefault(seq, dict(seq=seq, pb=NEG, pnb=NEG, lm=lmv, cnode=cnode, bank=bank))
            ent[which] = lae(ent[which], v)

        for ent in beam:
            y, pb, pnb = ent["seq"], ent["pb"], ent["pnb"]
            tot = lae(pb, pnb)
            e = y[-1] if y else None
            add(y, "pb", tot + lp[t, blank], ent["lm"], ent["cnode"], ent["bank"])
            for c in cand[t].tolist():
                v = lp[t, c]
                if v == NEG:
                    continue
                if c == e:
                    add(y, "pnb", pnb + v, ent["lm"], ent["cnode"], ent["bank"])
                    if pb == NEG:
                        continue
                lmv = ent["lm"] + token_logp(lm, c, [bos] + list(y), V, order) if use_lm else 0.0
                if use_lm and (lmv == NEG or lmv != lmv):
                    continue  # an extension the LM forbids is not proposed
                cnode, bank = auto.step(ent["cnode"], ent["bank"], c) if use_ctx else (0, 0)
                add(y + (c, ), "pnb", (pb if c == e else tot) + v, lmv, cnode, bank)
        ranked = sorted(nxt.values(), key=lambda ent: -key_of(ent))  # (stable: dict order among equal keys)
        if len(ranked) > K:
            margin = min(margin, _gap_units(key_of(ranked[K - 1]), key_of(ranked[K])))
        beam = ranked[:K]
    out = []
    for ent in beam:
        ctc = lae(ent["pb"], ent["pnb"])
        lmf = ent["lm"] + token_logp(lm, eos, [bos] + list(ent["seq"]), V, order) if use_lm else 0.0
        ctx = ent["bank"] + auto.keep[ent["cnode"]] if use_ctx else 0
        if use_ctx:
            assert (ent["cnode"], ent["bank"]) == auto.state(ent["seq"])  # the state is a function of the sequence alone
        out.append((ent["seq"], combine(ctc, lmf, ctx, len(ent["seq"]), lm_weight, context_weight, length_bonus), ctc, lmf, ctx))
    rk = [NEG if h[1] != h[1] else h[1] for h in out]
    order_ = sorted(range(len(out)), key=lambda i: -rk[i])  # (stable: the beam's order among equal finals)
    for a, b in zip(order_[:n_best], order_[1:n_best + 1]):
        margin = min(margin, _gap_units(rk[a], rk[b]))
    return [out[i] for i in order_[:n_best]], float(margin)


def rescore_route(logits, K, C, blank, auto, context_weight):
    """what re-ranking can do: the CTC-only beam of K, every prefix of it re-scored by context_reference.rescore with base = ctc.
    Returns (hyps best first as (tuple, score), the CTC-only beam's tuples, margin)"""
    hyps, margin = R.beam_search(logits, K, C, K, blank)
    N = len(hyps)
    L = max(max(len(y) for y, _ in hyps), 1)
    ids = np.zeros((N, L), dtype=np.int64)
    for i, (y, _) in enumerate(hyps):
        ids[i, :len(y)] = y
    _, score, od = X.rescore(ids, [len(y) for y, _ in hyps], [s for _, s in hyps], N, L + 1, auto, context_weight)
    margin = min(margin, X.margin(score))
    return [(hyps[i][0], float(score[i])) for i in od[0]], [y for y, _ in hyps], float(margin)


# ---------------------------------------------------------------- the inputs of the GPU tests
# The shapes of ctc_beam_reference's pinned cases short, k8, k32 and the identity case (ctc_beam_lm_reference's identity_lm, whose
# V = 5 holds bos and eos), the case's LM as ctc_beam_lm_reference has it, and a phrase set drawn from the case's labels: half of it
# sub-sequences of the UNBIASED search's hypotheses on the same logits (so that phrases do occur, also in lower-ranked hypotheses),
# half random ones with shared prefixes.  Every case is pinned with the LM (lm_weight 0.5, bonus 0.5) and without one; SEEDS holds
# the first seed from the case's base at which every utterance is decidable (find_seed).
CTX_WEIGHT = 1.0
COMBOS = ((0.5, 0.5), (0.0, 0.0))  # (lm_weight, length_bonus)
CASES = {name: dict(F.CASES[name], n_phrases=n, phrase_seed=s) for name, n, s in
         (("short", 8, 21), ("k8", 24, 22), ("k32", 24, 23), ("identity_lm", 4, 24))}
SEEDS = {}  # filled below


def case_logits(name, seed):
    c = CASES[name]
    return R.planted_logits(seed, c["B"], c["T"], c["V"], BLANK) if c["gen"] == "planted" else R.random_logits(seed, c["B"], c["T"], c["V"], c["scale"])


def case_phrases(name, seed):
    c = CASES[name]
    x = case_logits(name, seed)
    rs = np.random.RandomState(c["phrase_seed"] * 1000 + seed)
    out = []
    for u in range(c["B"]):
        hyps, _ = R.beam_search(x[u, :min(c["in_len"][u], c["T"])], c["K"], c["C"], c["K"], BLANK)
        for y, _ in hyps[1:]:
            if len(y) >= 2 and len(out) < c["n_phrases"] // 2:
                L = int(rs.randint(2, min(len(y), 4) + 1))
                i = int(rs.randint(0, len(y) - L + 1))
                out.append(tuple(int(v) for v in y[i:i + L]))
    out += X.random_phrases(rs, c["V"], c["n_phrases"] - len(out), lengths=(1, 4), share=0.5, lo=1)
    return out


def run_case(name, w, b, seed=None):
    """[(hyps, margin)] per utterance of the case at lm_weight w, length_bonus b and CTX_WEIGHT"""
    c = CASES[name]
    seed = SEEDS[(name, w, b)] if seed is None else seed
    x = case_logits(name, seed)
    auto = X.Automaton(case_phrases(name, seed), c["V"])
    return [beam_search(x[u, :min(c["in_len"][u], c["T"])], c["K"], c["C"], c["n_best"], BLANK, F.case_lm(name), c["V"], c["order"], BOS, EOS,
                        w, b, auto, CTX_WEIGHT) for u in range(c["B"])]


@functools.lru_cache(maxsize=None)
def case_reference(name, w, b):
    """the pinned case's reference result, computed once per process and shared by the tests: do not modify"""
    return run_case(name, w, b)


def find_seed(name, w, b, tries=64):
    """how SEEDS was made: the first seed from the case's base whose every utterance is decidable and on which the context term
    counts (some returned hypothesis has ctx > 0); None if `tries` seeds give none"""
    for seed in range(CASES[name]["base"], CASES[name]["base"] + tries):
        res = run_case(name, w, b, seed)
        if min(m for _, m in res) >= DECIDABLE and any(h[4] > 0 for hyps, _ in res for h in hyps):
            return seed
    return None


SEEDS.update({("short", 0.5, 0.5): 100, ("short", 0.0, 0.0): 100, ("k8", 0.5, 0.5): 200, ("k8", 0.0, 0.0): 200, ("k32", 0.5, 0.5): 421,
              ("k32", 0.0, 0.0): 401, ("identity_lm", 0.5, 0.5): 700, ("identity_lm", 0.0, 0.0): 700})
PINNED = tuple(sorted(SEEDS))  # (case, lm_weight, length_bonus)

# ---------------------------------------------------------------- inputs on which biasing wins
# Weakly peaked planted logits and no LM: a labelling the CTC-only beam of K has pruned holds a phrase; the biased search of the same
# K returns it first, at least 4 tolerances ahead of the best that re-ranking the CTC-only beam can return.  The phrases are
# sub-sequences of a hypothesis that a WIDE CTC-only beam (WINS["wide"]) keeps and the beam of K does not.  One utterance per K;
# WINS_SEEDS holds the first seed from the base at which it holds with both routes decidable (find_wins_seed).
WINS = dict(T=33, V=11, C=3, peak=(1.5, 3.0), context_weight=1.5, wide=32, n_phrases=3, base=1000)
WINS_K = (2, 3, 4)
WINS_SEEDS = {}


def wins_logits(K, seed=None):
    return R.planted_logits(WINS_SEEDS[K] if seed is None else seed, 1, WINS["T"], WINS["V"], BLANK, peak=WINS["peak"])


def wins_phrases(K, seed=None):
    """sub-sequences of 3 tokens of the best hypothesis of the wide beam that the beam of K does not hold"""
    w = WINS
    x = wins_logits(K, seed)[0]
    narrow = {y for y, _ in R.beam_search(x, K, w["C"], K, BLANK)[0]}
    wide = [y for y, _ in R.beam_search(x, w["wide"], w["C"], w["wide"], BLANK)[0] if y not in narrow and len(y) >= 3]
    if not wide:
        return []
    y = wide[0]
    starts = np.linspace(0, len(y) - 3, num=min(w["n_phrases"], len(y) - 2)).astype(int)
    return sorted({tuple(y[i:i + 3]) for i in starts})


def wins_property(K, seed=None):
    """(holds?, biased hyps, rescore-route hyps, the CTC-only beam, the phrases)"""
    w = WINS
    x = wins_logits(K, seed)[0]
    phrases = wins_phrases(K, seed)
    if not phrases:
        return False, None, None, None, phrases
    auto = X.Automaton(phrases, w["V"])
    biased, m1 = beam_search(x, K, w["C"], 1, BLANK, None, w["V"], 1, BOS, EOS, 0.0, 0.0, auto, w["context_weight"])
    route, ctc_beam, m2 = rescore_route(x, K, w["C"], BLANK, auto, w["context_weight"])
    ok = min(m1, m2) >= DECIDABLE and biased[0][0] not in ctc_beam and biased[0][4] > 0 and _gap_units(biased[0][1], route[0][1]) >= DECIDABLE
    return ok, biased, route, ctc_beam, phrases


@functools.lru_cache(maxsize=None)
def wins_reference(K):
    """the pinned input's result, computed once per process and shared by the tests: do not modify"""
    return wins_property(K)


def find_wins_seed(K, tries=64):
    for seed in range(WINS["base"], WINS["base"] + tries):
        if wins_property(K, seed)[0]:
            return seed
    return None


WINS_SEEDS.update({2: 1003, 3: 1001, 4: 1012})
