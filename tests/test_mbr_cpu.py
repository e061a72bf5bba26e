"""CPU: the reference of minimum-Bayes-risk ranking (tests/mbr_reference.py) against the host Levenshtein of joeys2t_amd.metrics, known
answers and the metric axioms; the decidability of every input the GPU tests (tests/test_hip_mbr.py) compare orders exactly on; and
what needs no device of the feature itself: the declarations, the limits of the two entry points (refused before a launch) and the
argument validation of the decoders."""
import ctypes
import math

import numpy as np
import pytest

import mbr_reference as M


# ---------------------------------------------------------------- the reference
def test_edit_distance_equals_the_host_metric():
    from joeys2t_amd.metrics import edit_distance
    rs = np.random.RandomState(0)
    for it in range(200):
        a = rs.randint(0, 4, size=rs.randint(0, 20)).tolist()
        b = M.variant(rs, a, int(rs.randint(0, 5))) if it % 2 else rs.randint(0, 4, size=rs.randint(0, 20)).tolist()
        assert M.edit_distance(a, b) == edit_distance(a, b), (a, b)


def test_known_answers():
    k, s = [ord(c) for c in "kitten"], [ord(c) for c in "sitting"]
    assert M.edit_distance(k, s) == 3 and M.edit_distance(s, k) == 3
    assert M.edit_distance([], []) == 0 and M.edit_distance([], k) == 6 and M.edit_distance(s, []) == 7
    assert M.edit_distance([5], [2**40 + 5]) == 1 and M.edit_distance([2**40 + 5], [2**40 + 5]) == 0  # full 64-bit ids


def test_metric_axioms():
    rs = np.random.RandomState(1)
    for _ in range(100):
        a, b, c = (rs.randint(0, 3, size=rs.randint(0, 12)).tolist() for _ in range(3))
        ab, bc, ac = M.edit_distance(a, b), M.edit_distance(b, c), M.edit_distance(a, c)
        assert ab == M.edit_distance(b, a)
        assert abs(len(a) - len(b)) <= ab <= max(len(a), len(b))
        assert ac <= ab + bc
        assert M.edit_distance(a, a) == 0


def test_posterior_and_the_two_slot_risks():
    ids = np.array([[1, 2, 3, 4], [1, 5, 3, 0]])
    n, score = np.array([4, 3]), np.array([-1.0, -2.0])
    dist, post, risk, order = M.mbr(ids, n, score, 2, 5, 1.0)
    d = M.edit_distance([1, 2, 3, 4], [1, 5, 3])
    assert d == 2 and dist.tolist() == [[[0, 2], [2, 0]]]
    assert abs(post.sum() - 1.0) <= 1e-15 and abs(post[0] - 1 / (1 + math.exp(-1.0))) <= 1e-15
    assert risk[0] == post[1] * d and risk[1] == post[0] * d  # at N = 2 the risks are p_1 d and p_0 d
    assert order.tolist() == [[0, 1]]  # the likelier one has the smaller risk
    for name in M.CASES:
        for s in M.SCALES:
            post = M.case_reference(name, s)[1].reshape(M.CASES[name]["B"], -1)
            assert all(abs(p.sum() - 1.0) <= 1e-12 or p.sum() == 0.0 for p in post), name


def test_rank_and_margin_rules():
    assert M.rank([1.0, 3.0, 1.0, np.inf, 2.0, np.inf]) == [0, 2, 4, 1, 3, 5]  # equal risks keep slot order, dead slots last
    assert M.margin([1.0, np.inf]) == np.inf and M.margin([2.0, 2.0, np.inf]) == np.inf
    assert abs(M.margin([10.0, 10.5, np.inf, 30.0]) - 0.5 / M.bound(10.5)) <= 1e-9


@pytest.mark.parametrize("name", list(M.CASES))
def test_pinned_cases_are_decidable(name):
    """a condition on the INPUTS, checked here so that the GPU test may compare orders exactly: every utterance of every pinned case
    has margin >= 4 at both scales, and the seed is the first such one from the case's base"""
    margins = {s: M.case_margin(name, s) for s in M.SCALES}
    print(f"{name}: seed {M.SEEDS[name]} margins {({s: round(m, 1) for s, m in margins.items()})}")
    assert min(margins.values()) >= M.DECIDABLE
    assert M.find_seed(name) == M.SEEDS[name]
    c, x = M.CASES[name], M.case_inputs(name)
    assert x["ids"].shape == (c["B"], c["N"], c["T"]) and x["ids"].dtype == np.int64 and x["n"].dtype == np.int32 and x["score"].dtype == np.float32
    for s in M.SCALES:
        assert all(sorted(o) == list(range(c["N"])) for o in M.case_reference(name, s)[3].tolist())


def test_the_planted_cases_have_what_they_say():
    c, x = M.CASES["ragged"], M.case_inputs("ragged")
    dead = M.dead_slots(x["n"].reshape(-1), x["score"].reshape(-1), c["T"] + 1).reshape(c["B"], c["N"])
    assert dead[0].tolist() == [False, False, True, True, False] and x["score"][0, 2] == -np.inf and x["n"][0, 3] == c["T"] + 1
    assert dead[1, 1] and x["n"][1, 1] == -1 and dead[1, 3] and np.isnan(x["score"][1, 3]) and dead[1, 4] and x["score"][1, 4] == np.inf
    assert dead[2].all() and dead[3].tolist() == [True, True, False, True, True]
    dist, post, risk, order = M.case_reference("ragged", 1.0)
    assert order[2].tolist() == [0, 1, 2, 3, 4] and order[3, 0] == 2 and post[3 * 5 + 2] == 1.0 and risk[3 * 5 + 2] == 0.0
    assert (dist[2] == -1).all() and (dist[0, 2] == -1).all() and (dist[0, :, 3] == -1).all() and dist[0, 0, 0] == 0
    assert np.isinf(risk[dead.reshape(-1)]).all() and (post[dead.reshape(-1)] == 0).all()
    x = M.case_inputs("edges")
    assert set(x["n"].reshape(-1).tolist()) <= set(M.EDGE_LENGTHS) and x["n"].max() > 64
    x = M.case_inputs("long")
    assert x["n"].reshape(-1).tolist() == [M.EDIT_MAX_LEN, M.EDIT_MAX_LEN - 1, M.EDIT_MAX_LEN]
    x = M.case_inputs("hi_bits")
    assert np.array_equal(x["ids"][0, :, :6] % M.HI, np.broadcast_to(x["ids"][0, 0, :6], (4, 6))) and (x["n"] == 6).all()
    assert M.case_reference("hi_bits", 1.0)[0][0, 0].tolist() == [0, 1, 2, 3]


def test_consensus_mbr_top_is_not_the_map_top():
    x = M.case_inputs("consensus")
    assert int(np.argmax(x["score"][0])) == 0
    for s in M.SCALES:
        dist, post, risk, order = M.case_reference("consensus", s)
        assert order[0, 0] != 0 and order[0, 0] in (1, 2, 3) and int(np.argmax(post)) == 0


# ---------------------------------------------------------------- the feature, as far as no device is needed
def test_header_declares_and_library_exports_the_entry_points():
    from joeys2t_amd import _lib
    for name in ("js2t_edit_distance", "js2t_mbr_rescore", "js2t_edit_max_len"):
        assert name in _lib.declared_symbols()
        assert hasattr(_lib.lib(), name)
    restype, argtypes = _lib.FUNCTIONS["js2t_mbr_rescore"]
    assert len(argtypes) == 13 and restype is _lib.C.c_int and argtypes[11] is _lib.C.c_float and argtypes[9] is _lib.C.c_int32
    assert len(_lib.FUNCTIONS["js2t_edit_distance"][1]) == 12
    limit = _lib.lib().js2t_edit_max_len()
    assert limit == M.EDIT_MAX_LEN and limit >= 1024
    assert f"#define JS2T_EDIT_MAX_LEN {limit}\n" in _lib.HEADER_PATH.read_text()


def _refused(rc, *words):
    from joeys2t_amd import _lib
    msg = _lib.lib().js2t_last_error()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


def test_limits_are_refused_before_anything_is_launched():
    """every limit with NULL pointers: a launch would fault; the checks come first (as test_abi.py does for js2t_comm_*)"""
    from joeys2t_amd import _lib
    L = _lib.lib()
    big = M.EDIT_MAX_LEN

    def mbr(B=1, N=4, Lp=9, scale=1.0, stride=8):
        return L.js2t_mbr_rescore(None, stride, None, None, None, None, None, None, B, N, Lp, scale, None)

    _refused(mbr(N=0), b"N 0")
    _refused(mbr(N=33), b"N 33")
    _refused(mbr(Lp=0), b"Lp 0")
    _refused(mbr(Lp=big + 2, stride=big + 1), b"Lp - 1", str(big).encode())
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        _refused(mbr(scale=scale), b"scale")
    _refused(mbr(stride=7), b"ids_stride 7")
    _refused(mbr(B=2**31 // 16), b"B * N * N")
    _refused(mbr(), b"null pointer")  # (the limits hold: only now are the pointers looked at)
    assert mbr(B=0) == 0
    assert mbr(B=0, Lp=big + 1, stride=big) == 0 and mbr(B=0, N=33) != 0  # the limits are checked whatever B is

    def ed(R=1, group=1, a_max=8, b_max=8):
        return L.js2t_edit_distance(None, 8, None, None, 8, None, None, R, group, a_max, b_max, None)

    _refused(ed(group=0), b"group 0")
    _refused(ed(a_max=big + 1), b"a_max")
    _refused(ed(b_max=big + 1), b"b_max")
    _refused(ed(a_max=-1), b"a_max")
    _refused(ed(R=-1), b"R -1")
    _refused(ed(), b"null pointer")
    assert ed(R=0) == 0 and ed(R=0, group=0) != 0
    with pytest.raises(ctypes.ArgumentError):
        L.js2t_mbr_rescore(None, 8, None, None, None, None, None, None, 1, 4.5, 9, 1.0, None)


@pytest.mark.parametrize("kw, what", [
    (dict(decision="x"), "decision 'x'"),
    (dict(decision="mbr", mbr_scale=0), "mbr_scale 0"),
    (dict(decision="mbr", mbr_scale=-1.0), "mbr_scale -1"),
    (dict(decision="mbr", mbr_scale=float("nan")), "mbr_scale nan"),
    (dict(decision="mbr", mbr_scale=float("inf")), "mbr_scale inf"),
    (dict(mbr_scale=2), "mbr_scale 2.0 with decision='map'"),
    (dict(decision="map", mbr_scale=2), "mbr_scale 2.0 with decision='map'"),
])
def test_decision_options_are_refused_before_the_model_is_touched(kw, what):
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    for fn in (ctc_beam_search, ctc_attention_rescore):
        with pytest.raises(ValueError, match=what):
            fn(None, None, beam_size=4, **kw)
    for decoder in ("ctc", "ctc-attention", "attention"):
        with pytest.raises(ValueError, match=what):
            predict(None, [None], decoder=decoder, **kw)


def test_the_attention_decoder_refuses_mbr_and_sizes_are_checked():
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import ctc_beam_search
    with pytest.raises(ValueError, match="decision='mbr'.*decoder='attention'"):
        predict(None, [None], decoder="attention", decision="mbr")
    with pytest.raises(ValueError, match="n_rescore 5"):  # accepted without an LM now, and still bounded by the beam
        ctc_beam_search(None, None, beam_size=4, n_best=1, n_rescore=5, decision="mbr")
    with pytest.raises(ValueError, match="n_best 3"):
        ctc_beam_search(None, None, beam_size=4, n_best=3, n_rescore=2, decision="mbr")
    with pytest.raises(ValueError, match="n_rescore without an lm"):  # decision="map" is as it was
        ctc_beam_search(None, None, beam_size=4, n_best=1, n_rescore=2)
    with pytest.raises((AttributeError, TypeError)):  # valid options get as far as the model
        ctc_beam_search(None, None, beam_size=4, n_best=1, n_rescore=2, decision="mbr", mbr_scale=0.5)
