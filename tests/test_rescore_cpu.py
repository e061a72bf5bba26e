"""CPU: the float64 reference of attention rescoring (tests/rescore_reference.py) against a known answer worked out by hand, its tie
and NaN rules, the decidability of every input the GPU tests (tests/test_hip_rescore.py) compare orders exactly on, and the argument
validation of search.ctc_attention_rescore that needs no device."""
import numpy as np
import pytest

import rescore_reference as R


def test_header_declares_the_entry_point():
    from joeys2t_amd import _lib
    assert "js2t_rescore" in _lib.declared_symbols()
    restype, argtypes = _lib.FUNCTIONS["js2t_rescore"]
    assert len(argtypes) == 17 and restype is _lib.C.c_int and argtypes[15] is _lib.C.c_float and argtypes[11] is _lib.C.c_int32


def known_answer_inputs():
    """two slots, V = 3, one label each (label 1, then EOS = 2).  Slot 0: P(label) = P(EOS | label) = 0.5, CTC probability 0.6;
    slot 1: 0.8 and 0.8, CTC probability 0.3.  CTC prefers slot 0 (0.6 > 0.3), attention slot 1 (0.64 > 0.25), and at w = 0.5 the
    geometric means are sqrt(0.6 * 0.25) = 0.387 < sqrt(0.3 * 0.64) = 0.438: slot 1 first"""
    p = np.array([[[0.25, 0.5, 0.25], [0.3, 0.2, 0.5]], [[0.1, 0.8, 0.1], [0.15, 0.05, 0.8]]])
    return np.log(p), np.array([[1, 0], [1, 0]]), np.array([1, 1]), np.log(np.array([0.6, 0.3]))


def test_known_answer():
    logits, ids, n, ctc = known_answer_inputs()
    tok, att, score, order = R.rescore(logits, ids, n, ctc, 2, 2, 0.5)
    assert np.allclose(tok, np.log([[0.5, 0.5], [0.8, 0.8]]), atol=1e-14)
    assert np.allclose(att, np.log([0.25, 0.64]), atol=1e-14)
    assert np.allclose(score, 0.5 * np.log([0.6 * 0.25, 0.3 * 0.64]), atol=1e-14)
    assert order.tolist() == [[1, 0]]
    _, _, s1, o1 = R.rescore(logits, ids, n, ctc, 2, 2, 1.0)
    assert o1.tolist() == [[0, 1]] and np.array_equal(s1, ctc)  # each head's own order, its own numbers
    _, a0, s0, o0 = R.rescore(logits, ids, n, ctc, 2, 2, 0.0)
    assert o0.tolist() == [[1, 0]] and np.array_equal(s0, a0)
    assert R.margin(score) >= R.DECIDABLE


def test_length_decides_not_the_id():
    """a label equal to EOS (or to anything else) is a label: with n = 2 the row scores ids[0], ids[1] and then EOS; whatever stands
    behind n - an id far outside the vocabulary, NaN logits - is not read"""
    rs = np.random.RandomState(0)
    logits = rs.randn(1, 4, 5)
    ids = np.array([[2, 2, 2**40 + 5]])
    logits[0, 3] = np.nan
    tok, att, score, order = R.rescore(logits, ids, np.array([2]), np.array([-1.0]), 1, 2, 0.3)
    lp = logits[0] - np.log(np.exp(logits[0]).sum(-1, keepdims=True))
    assert np.allclose(tok[0, :3], lp[[0, 1, 2], [2, 2, 2]], atol=1e-14) and tok[0, 3] == 0.0
    assert abs(att[0] - tok[0, :3].sum()) <= 1e-14 and abs(score[0] - (0.3 * -1.0 + 0.7 * att[0])) <= 1e-14
    tok2, att2, _, _ = R.rescore(logits, np.array([[2, 7, 0]]), np.array([2]), np.array([-1.0]), 1, 2, 0.3)
    assert tok2[0, 1] == -np.inf and att2[0] == -np.inf  # a label outside the vocabulary


def test_dead_slots_and_weights_of_zero():
    logits = np.random.RandomState(1).randn(4, 3, 6)
    logits[1:] = np.nan  # the dead slots' logits are not read
    ids = np.zeros((4, 2), dtype=np.int64)
    n = np.array([1, 1, 3, -1])
    ctc = np.array([-2.0, -np.inf, -1.0, -1.0])
    tok, att, score, order = R.rescore(logits, ids, n, ctc, 4, 2, 0.3)
    assert np.isfinite(score[0]) and (score[1:] == -np.inf).all() and (att[1:] == -np.inf).all() and (tok[1:] == 0).all()
    assert order.tolist() == [[0, 1, 2, 3]]  # the dead ones last, in slot order
    ids[0, 0] = 9  # att = -inf: w = 1 still returns the CTC score, w = 0.3 gives -inf and not NaN
    assert R.rescore(logits, ids, n, ctc, 4, 2, 1.0)[2][0] == -2.0
    assert R.rescore(logits, ids, n, ctc, 4, 2, 0.3)[2][0] == -np.inf


def test_tie_and_nan_rules():
    assert R.rank([-1.0, -3.0, -1.0, -2.0, -3.0]) == [0, 2, 3, 1, 4]  # equal scores keep slot order
    assert R.rank([np.nan, -5.0, -np.inf, np.nan, -1.0]) == [4, 1, 0, 2, 3]  # NaN ranks as -inf, in slot order among them
    assert sorted(R.rank([np.nan] * 7)) == list(range(7))
    assert R.margin([-1.0, -np.inf, np.nan]) == np.inf and abs(R.margin([-10.0, -10.5, -np.inf, -30.0]) - 0.5 / R.bound(10.5)) <= 1e-9


@pytest.mark.parametrize("name", list(R.CASES))
def test_pinned_cases_are_decidable(name):
    """a condition on the INPUTS, checked here so that the GPU test may compare orders exactly: every utterance of every pinned case
    has margin >= 4 at every weight it is used with, and the seed is the first such one from the case's base"""
    margins = {w: R.case_margin(name, w) for w in R.WEIGHTS}
    print(f"{name}: seed {R.SEEDS[name]} margins {({w: round(m, 1) for w, m in margins.items()})}")
    assert min(margins.values()) >= R.DECIDABLE
    assert R.find_seed(name) == R.SEEDS[name]
    c = R.CASES[name]
    x = R.case_inputs(name)
    assert x["logits"].shape == (c["B"] * c["N"], c["Lp"], c["V"]) and x["logits"].dtype == np.float32 and x["ids"].shape[2] >= c["Lp"] - 1
    if c.get("bf16"):
        assert np.array_equal(R.bf16_round(x["logits"]), x["logits"])
    for w in R.WEIGHTS:
        assert all(sorted(o) == list(range(c["N"])) for o in R.case_reference(name, w)[3].tolist())


def test_the_planted_case_has_what_it_says():
    c, x = R.CASES["ragged"], R.case_inputs("ragged")
    dead = R.dead_slots(x["n"].reshape(-1), x["ctc"].reshape(-1), c["Lp"]).reshape(c["B"], c["N"])
    assert x["n"][0, 0] == c["Lp"] - 1 and x["n"][0, 1] == 0 and c["B"] == 3
    assert dead[0].tolist() == [False, False, True, True, False] and x["ctc"][0, 2] == -np.inf and x["n"][0, 3] == c["Lp"]
    assert dead[1].tolist() == [False, False, True, False, False] and not dead[2].any()
    order = R.case_reference("ragged", 0.3)[3]
    assert order[0, 3:].tolist() == [2, 3] and order[1, 4] == 2


# ---------------------------------------------------------------- search-level argument validation (no device)
@pytest.mark.parametrize("kw, what", [
    (dict(beam_size=4, n_best=5), "n_best 5"),
    (dict(beam_size=4, n_best=1, n_rescore=5), "n_rescore 5"),
    (dict(beam_size=4, n_best=3, n_rescore=2), "n_best 3"),
    (dict(beam_size=33, n_best=1), "beam_size 33"),
    (dict(beam_size=4, n_best=0), "n_best 0"),
    (dict(beam_size=4, ctc_weight=1.5), "ctc_weight 1.5"),
    (dict(beam_size=4, ctc_weight=float("nan")), "ctc_weight nan"),
])
def test_search_argument_validation(kw, what):
    """the sizes are refused before the model or the batch is touched"""
    from joeys2t_amd.search import ctc_attention_rescore
    with pytest.raises(ValueError, match=what):
        ctc_attention_rescore(None, None, **kw)


def test_predict_names_its_decoders():
    from joeys2t_amd.prediction import predict
    with pytest.raises(ValueError, match="decoder.*attention.*ctc.*ctc-attention"):
        predict(None, [], decoder="rnn")
