"""CPU: the float64 reference of CTC prefix beam search (tests/ctc_beam_reference.py) against brute-force enumeration, the
known answer, and the decidability of every input the GPU tests (tests/test_hip_ctc_beam.py) compare exactly on."""
import numpy as np
import pytest

import ctc_beam_reference as R


@pytest.fixture(autouse=True, scope="module")
def contract_is_declared():
    """the reference restates the contract of include/joeys2t_hip.h: without the declaration there is nothing for it to pin"""
    from joeys2t_amd import _lib
    assert {"js2t_ctc_beam_search", "js2t_ctc_beam_workspace_bytes"} <= set(_lib.declared_symbols())


def test_header_declares_the_entry_points():
    from joeys2t_amd import _lib
    assert {"js2t_ctc_beam_search", "js2t_ctc_beam_workspace_bytes"} <= set(_lib.declared_symbols())
    restype, argtypes = _lib.FUNCTIONS["js2t_ctc_beam_search"]
    assert len(argtypes) == 20 and restype is _lib.C.c_int
    assert _lib.FUNCTIONS["js2t_ctc_beam_workspace_bytes"] == (_lib.C.c_int64, [_lib.C.c_int64, _lib.C.c_int64, _lib.C.c_int32])


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("T", [1, 3, 5])
def test_reference_against_enumeration(T, C):
    """V = 4, a beam so wide that nothing is pruned: every prefix's score is the log-sum over all V^T frame labellings that are
    admissible under the truncated distribution and collapse to it - and no other prefix exists"""
    V, blank = 4, 1
    worst = 0.0
    for seed in range(4):
        logits = np.random.RandomState(10 * T + seed).randn(T, V) * 2.0
        want = R.brute_force(logits, C, blank)
        K = len(want)
        hyps, _ = R.beam_search(logits, K + 3, C, K + 3, blank)
        assert {y for y, _ in hyps} == set(want) and len(hyps) == K
        assert [s for _, s in hyps] == sorted((s for _, s in hyps), reverse=True)
        worst = max(worst, max(abs(s - want[y]) for y, s in hyps))
        total = np.logaddexp.reduce(np.array([s for _, s in hyps]))  # all the mass the truncation leaves
        lp = R.log_softmax(logits)
        cand = R.candidates(logits, C, blank)
        kept = sum(np.logaddexp.reduce(np.append(lp[t, cand[t]], lp[t, blank])) for t in range(T))
        assert abs(total - kept) <= 1e-12
    print(f"T {T} C {C}: worst |reference - enumeration| {worst:.2e}")
    assert worst <= 1e-12


def test_known_answer():
    """two frames of blank 0.6 / a 0.4: the best path is (blank, blank), the best labelling is `a` with 1 - 0.36"""
    logits = np.log(np.array([[0.6, 0.4], [0.6, 0.4]]))
    hyps, margin = R.beam_search(logits, 2, 1, 2, 0)
    assert [y for y, _ in hyps] == [(1, ), ()]
    assert abs(hyps[0][1] - np.log(0.64)) <= 1e-14 and abs(hyps[1][1] - np.log(0.36)) <= 1e-14
    assert margin >= R.DECIDABLE


def test_candidates_order():
    logits = np.array([[5.0, 1.0, 3.0, 3.0, 0.0], [0.0, 2.0, 2.0, 9.0, 2.0]])
    assert R.candidates(logits, 3, 0).tolist() == [[2, 3, 1], [3, 1, 2]]
    assert R.candidates(logits, 2, 3).tolist() == [[0, 2], [1, 2]]


@pytest.mark.parametrize("name", list(R.CASES))
def test_pinned_cases_are_decidable(name):
    """the test that keeps the GPU tests from depending on luck: every input they compare exactly on has margin >= 4 in every
    utterance, and its seed is the first decidable one from the case's base"""
    res = R.case_reference(name)
    margins = [m for _, m in res]
    print(f"{name}: seed {R.SEEDS[name]} margins {['%.1f' % m for m in margins]}")
    assert min(margins) >= R.DECIDABLE
    assert R.find_seed(name) == R.SEEDS[name]
    c = R.CASES[name]
    for b, (hyps, _) in enumerate(res):
        assert len(hyps) == min(c["n_best"], len(hyps)) and all(len(y) <= min(c["in_len"][b], c["T"]) for y, _ in hyps)
        assert len({y for y, _ in hyps}) == len(hyps)


def test_identity_case_separates_the_node_variant():
    """a prefix is pruned while its child survives, is created again as a new trie node, and its extension then has to meet the
    surviving child: identity by (parent node, token) returns something else on the pinned identity case - and on a fair share of
    such inputs, while planted inputs at larger shapes never show it"""
    seq = R.case_reference("identity")
    node = R.run_case("identity", identity="node")
    assert R.differs(seq, node)
    base = R.CASES["identity"]["base"]
    n = sum(R.differs(R.run_case("identity", s), R.run_case("identity", s, "node")) for s in range(base, base + 200))
    print(f"node identity differs on {n} of 200 random inputs at V = 3, K = 3, C = 2, T = 10")
    assert n >= 1
    assert not R.differs(R.case_reference("k8"), R.run_case("k8", identity="node"))


def test_bf16_round():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.14159, 0.0], dtype=np.float32)  # 1 + 2^-8 ties to even (down), 1 + 3 * 2^-8 up
    assert R.bf16_round(x).tolist() == [1.0, 1.0, 1.015625, -3.140625, 0.0]
