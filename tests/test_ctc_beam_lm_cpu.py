"""CPU: the float64 reference of CTC prefix beam search with the LM fused into the beam (tests/ctc_beam_lm_reference.py) against
brute-force enumeration and the rescore reference where nothing is pruned, against ctc_beam_reference at zero weights, the
decidability of every input the GPU tests (tests/test_hip_ctc_beam_lm.py) compare exactly on, and the inputs on which fusion wins."""
import numpy as np
import pytest

import ctc_beam_lm_reference as F
import ctc_beam_reference as R
import ngram_reference as G

BOS, EOS = F.BOS, F.EOS


def test_header_declares_the_entry_point():
    """js2t_ctc_beam_search's 20 parameters, the model's 5, bos / eos / lm_weight / length_bonus and the two further outputs"""
    from joeys2t_amd import _lib
    assert "js2t_ctc_beam_search_lm" in set(_lib.declared_symbols())
    restype, argtypes = _lib.FUNCTIONS["js2t_ctc_beam_search_lm"]
    assert len(argtypes) == 20 + 5 + 4 + 2 and restype is _lib.C.c_int
    assert argtypes.count(_lib.C.c_float) == 2


def unpruned(seed, T, C, order, w, b, V=4, blank=0):
    """(logits, lm, every labelling's brute-force CTC log-mass, the fused list with a beam wider than the number of labellings)"""
    logits = np.random.RandomState(seed).randn(T, V) * 2.0
    lm = G.lm_dict(V, order, 40 + order, 0.4)
    want = R.brute_force(logits, C, blank)
    K = len(want) + 3
    hyps, _ = F.beam_search(logits, K, C, K, blank, lm, V, order, BOS, EOS, w, b)
    return logits, lm, want, hyps


def lm_sum(lm, y, V, order):
    return sum(G.token_logp(lm, w, [BOS] + list(y[:l]), V, order) for l, w in enumerate(list(y) + [EOS]))


@pytest.mark.parametrize("w, b", [(0.5, 0.5), (0.5, 0.0), (0.7, 0.0), (0.0, 0.5)])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("C", [2, 3])
def test_reference_against_enumeration(C, order, w, b):
    """V = 4, T = 5, a beam so wide that nothing is pruned: every labelling is there and its final score is the brute force's CTC
    log-mass + lm_weight * (the LM sum with EOS) + the bonus"""
    V, T = 4, 5
    worst = 0.0
    for seed in range(3):
        logits, lm, want, hyps = unpruned(50 + seed, T, C, order, w, b)
        assert {h[0] for h in hyps} == set(want) and len(hyps) == len(want)
        assert [h[1] for h in hyps] == sorted((h[1] for h in hyps), reverse=True)
        for y, final, ctc, lms in hyps:
            s = lm_sum(lm, y, V, order) if w != 0 else 0.0
            worst = max(worst, abs(ctc - want[y]), abs(lms - s), abs(final - (want[y] + w * s + b * len(y))))
    print(f"C {C} order {order} weights {w} / {b}: worst |reference - enumeration| {worst:.2e}")
    assert worst <= 1e-9


@pytest.mark.parametrize("order", [1, 3, 4])
def test_unpruned_list_is_the_rescored_list(order):
    """nothing pruned: the fused list is ngram_reference.rescore over all labellings with base = the brute-force CTC log-mass, in
    its order"""
    V, T, C, w, b = 4, 5, 3, 0.5, 0.5
    logits, lm, want, hyps = unpruned(60, T, C, order, w, b)
    ys = sorted(want)
    ids = np.zeros((len(ys), T), dtype=np.int64)
    for i, y in enumerate(ys):
        ids[i, :len(y)] = y
    _, lms, score, od = G.rescore(ids, [len(y) for y in ys], [want[y] for y in ys], len(ys), T + 1, lm, V, order, BOS, EOS, w, b)
    assert G.margin(score) > 0  # no two labellings tie: the order is defined
    assert [h[0] for h in hyps] == [ys[i] for i in od[0]]
    assert all(abs(h[1] - score[i]) <= 1e-9 and abs(h[3] - lms[i]) <= 1e-9 for h, i in zip(hyps, od[0]))


@pytest.mark.parametrize("name", list(R.CASES))
def test_zero_weights_are_the_ctc_only_search(name):
    """both weights 0: the hypotheses, scores and margin of ctc_beam_reference.beam_search exactly; the model is not read"""
    c = R.CASES[name]
    x = R.case_logits(name)
    for u, (hyps, margin) in enumerate(R.case_reference(name)):
        got, m = F.beam_search(x[u, :min(c["in_len"][u], c["T"])], c["K"], c["C"], c["n_best"], R.BLANK, None, c["V"], 3, BOS, EOS, 0.0, 0.0)
        assert [(h[0], h[1]) for h in got] == [(y, s) for y, s in hyps] and m == margin
        assert all(h[2] == h[1] and h[3] == 0.0 for h in got)


def test_no_frames():
    lm = F.case_lm("k16")
    hyps, margin = F.beam_search(np.zeros((0, 37)), 4, 3, 2, 0, lm, 37, 3, BOS, EOS, 0.5, 0.5)
    eos = G.token_logp(lm, EOS, [BOS], 37, 3)
    assert hyps == [((), 0.5 * eos, 0.0, eos)] and margin == np.inf


def test_an_extension_the_lm_forbids_is_never_proposed():
    lm = dict(F.case_lm("short"))
    lm[(5, )] = (-np.inf, 0.0)
    x = F.case_logits("short", 0.5, 0.5)[0]
    assert 5 in [v for h in F.run_case("short", 0.5, 0.5)[0][0] for v in h[0]]  # (the label matters on this input)
    hyps, _ = F.beam_search(x, 4, 3, 4, 0, lm, 11, 1, BOS, EOS, 0.5, 0.5)
    assert hyps and all(5 not in h[0] and np.isfinite(h[1]) for h in hyps)


@pytest.mark.parametrize("name, w, b", F.PINNED)
def test_pinned_cases_are_decidable(name, w, b):
    res = F.case_reference(name, w, b)
    margin = min(m for _, m in res)
    print(f"{name} at {w} / {b}: seed {F.SEEDS[(name, w, b)]}, margin {margin:.1f}")
    assert margin >= F.DECIDABLE
    assert all(np.isfinite(h[1]) for hyps, _ in res for h in hyps)
    if name == "identity_lm":
        assert F.differs(res, F.run_case(name, w, b, identity="node"))


def test_what_is_pinned():
    """every shape of ctc_beam_reference but its V = 3 identity case (eos = 3 lies outside that vocabulary; identity_lm replaces it) at
    (0.5, 0.5), and at (0.5, 0) except k32; orders 1, 3 and 4 occur and the order-4 model holds 4-grams"""
    names = set(R.CASES) - {"identity"} | {"identity_lm"}
    assert {k[0] for k in F.PINNED if k[1:] == (0.5, 0.5)} == names
    assert {k[0] for k in F.PINNED if k[1:] == (0.5, 0.0)} == names - {"k32"}
    assert {F.CASES[n]["order"] for n in names} == {1, 3, 4}
    assert all(G.lm_order(F.case_lm(n)) == F.CASES[n]["order"] for n in names)
    assert F.CASES["long_k2"]["T"] > 64  # the beam's LM state crosses the 64-frame chunks


def test_the_pinned_seeds_are_the_first_decidable_ones():
    """find_seed reproduces SEEDS on the quick cases (the slow ones were found the same way)"""
    for name in ("short", "k8", "long_k1", "identity_lm"):
        for w, b in F.COMBOS:
            assert F.find_seed(name, w, b) == F.SEEDS[(name, w, b)]
    assert all(F.find_wins_seed(K) == F.WINS_SEEDS[K] for K in F.WINS_K)


@pytest.mark.parametrize("K", F.WINS_K)
def test_fusion_wins(K):
    """both routes decidable; the fused best hypothesis is not in the CTC-only beam of the same K, so no re-ranking of that beam can
    return it; and its final score is at least 4 tolerances above the best the rescore route returns"""
    ok, fused, route, ctc_beam = F.wins_reference(K)
    gap = F._gap_units(fused[0][1], route[0][1])
    print(f"K {K} seed {F.WINS_SEEDS[K]}: fused best {fused[0][0]} final {fused[0][1]:.4f}; rescore route best {route[0][0]} "
          f"score {route[0][1]:.4f}; gap {gap:.1f} tolerances")
    assert ok and fused[0][0] not in ctc_beam and gap >= F.DECIDABLE
    # the fused final IS the rescore rule's score of that labelling: base = its CTC log-mass
    y, final, ctc, lms = fused[0]
    w = F.WINS
    ids = np.array([list(y) + [0]], dtype=np.int64)
    _, rl, rs, _ = G.rescore(ids, [len(y)], [ctc], 1, len(y) + 1, F.wins_lm(), w["V"], w["order"], BOS, EOS, w["lm_weight"], w["length_bonus"])
    assert abs(rs[0] - final) <= 1e-9 and abs(rl[0] - lms) <= 1e-9
