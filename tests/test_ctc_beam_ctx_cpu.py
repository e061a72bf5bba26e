"""CPU: the float64 reference of the biased search (tests/ctc_beam_ctx_reference.py) pinned by enumeration and against the reference
it extends, the pinned inputs of the GPU tests (tests/test_hip_ctc_beam_ctx.py) and the entry points' signatures."""
import numpy as np
import pytest

import context_reference as X
import ctc_beam_ctx_reference as Z
import ctc_beam_lm_reference as F
import ctc_beam_reference as R
import ngram_reference as G

BOS, EOS = Z.BOS, Z.EOS


def test_the_header_declares_the_entry_points():
    """js2t_ctc_beam_search_lm's 31 parameters, the graph's 6, context_weight and out_ctx; the rescore takes js2t_ngram_rescore's layout"""
    from joeys2t_amd import _lib
    C = _lib.C
    restype, argtypes = _lib.FUNCTIONS["js2t_ctc_beam_search_ctx"]
    assert len(argtypes) == 31 + 6 + 2 and restype is C.c_int and argtypes.count(C.c_float) == 3
    restype, argtypes = _lib.FUNCTIONS["js2t_context_rescore"]
    assert len(argtypes) == 19 and restype is C.c_int and argtypes.count(C.c_float) == 1
    assert len(_lib.FUNCTIONS["js2t_context_walk_host"][1]) == 13


def lm_sum(lm, y, V, order):
    return sum(G.token_logp(lm, w, [BOS] + list(y[:l]), V, order) for l, w in enumerate(list(y) + [EOS]))


PHRASES = {"plain": [(1, 2), (3, )], "nested": [(1, 2), (1, 2, 3, 1)], "overlap": [(1, 1, 2), (2, 3)], "inside": [(1, 2, 3, 1), (2, 3)]}


@pytest.mark.parametrize("w, b, cw", [(0.5, 0.5, 1.0), (0.0, 0.0, 1.0), (0.7, 0.0, 0.25), (0.0, 0.5, 2.0)])
@pytest.mark.parametrize("phrases", list(PHRASES))
@pytest.mark.parametrize("C", [2, 3])
def test_reference_against_enumeration(C, phrases, w, b, cw):
    """V = 4, T = 5, a beam so wide that nothing is pruned: every labelling is there and its final score is the brute force's CTC
    mass + lm_weight * LM + context_weight * ctx + bonus * length within 1e-9, ctx the automaton's count of the labelling"""
    V, T, order = 4, 5, 3
    logits = np.random.RandomState(50 + C).randn(T, V) * 2.0
    lm = G.lm_dict(V, order, 43, 0.4)
    auto = X.Automaton(PHRASES[phrases], V)
    want = R.brute_force(logits, C, 0)
    K = len(want) + 3
    hyps, _ = Z.beam_search(logits, K, C, K, 0, lm, V, order, BOS, EOS, w, b, auto, cw)
    assert sorted(h[0] for h in hyps) == sorted(want)
    for y, final, ctc, lmv, ctx in hyps:
        assert ctx == auto.ctx(y) and abs(ctc - want[y]) <= 1e-9
        full = want[y] + (w * lm_sum(lm, y, V, order) if w else 0.0) + cw * auto.ctx(y) + b * len(y)
        assert abs(final - full) <= 1e-9, (y, final, full)
    assert all(hyps[i][1] >= hyps[i + 1][1] for i in range(len(hyps) - 1))


@pytest.mark.parametrize("name, w, b", F.PINNED[:6])
def test_zero_context_weight_is_the_lm_reference(name, w, b):
    c = F.CASES[name]
    x = F.case_logits(name, w, b)
    auto = X.Automaton([(1, 2)], c["V"])
    for u in range(c["B"]):
        args = (x[u, :min(c["in_len"][u], c["T"])], c["K"], c["C"], c["n_best"], Z.BLANK, F.case_lm(name), c["V"], c["order"], BOS, EOS, w, b)
        got, m1 = Z.beam_search(*args, auto, 0.0)
        ref, m2 = F.beam_search(*args)
        assert [h[:4] for h in got] == ref and m1 == m2 and all(h[4] == 0 for h in got)


def test_pinned_cases_are_decidable_and_biased():
    """the seeds are the first ones find_seed accepts; the context term counts on every case, and on some case the biased list is
    not the unbiased one"""
    changed = 0
    for name, w, b in Z.PINNED:
        res = Z.case_reference(name, w, b)
        assert min(m for _, m in res) >= Z.DECIDABLE and any(h[4] > 0 for hyps, _ in res for h in hyps), (name, w, b)
        c = Z.CASES[name]
        x = Z.case_logits(name, Z.SEEDS[(name, w, b)])
        plain = [F.beam_search(x[u, :min(c["in_len"][u], c["T"])], c["K"], c["C"], c["n_best"], Z.BLANK, F.case_lm(name), c["V"], c["order"], BOS,
                               EOS, w, b)[0] for u in range(c["B"])]
        changed += [[h[0] for h in hyps] for hyps, _ in res] != [[h[0] for h in hyps] for hyps in plain]
    assert len(Z.PINNED) == 8 and changed >= 1
    assert Z.find_seed("short", 0.5, 0.5) == Z.SEEDS[("short", 0.5, 0.5)] and Z.find_seed("identity_lm", 0.0, 0.0) == Z.SEEDS[("identity_lm", 0.0, 0.0)]


@pytest.mark.parametrize("K", Z.WINS_K)
def test_wins_inputs_hold_on_the_reference(K):
    """the biased best is absent from the CTC-only beam of K, holds a phrase, and is at least 4 tolerances ahead of the best that
    re-ranking that beam can give"""
    ok, biased, route, ctc_beam, phrases = Z.wins_reference(K)
    assert ok and phrases and biased[0][0] not in ctc_beam and biased[0][4] > 0
    assert Z._gap_units(biased[0][1], route[0][1]) >= Z.DECIDABLE
    assert K != 2 or Z.find_wins_seed(K) == Z.WINS_SEEDS[K]
