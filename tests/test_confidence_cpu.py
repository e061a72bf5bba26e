"""No GPU: the reference of the token confidence (tests/confidence_reference.py) pinned on the examples the header gives and on every
pair of short rows, word_confidence, the header's declaration and the refusals of the decoders' confidence options."""
import ctypes
import itertools

import numpy as np
import pytest

import confidence_reference as CR
import mbr_reference as M


# ---------------------------------------------------------------- the reference
def test_the_headers_three_examples():
    assert CR.flags([0, 0], [0]) == [0, 1]                 # the rule ...
    assert CR.flags_prefix_trimmed([0, 0], [0]) == [1, 0]  # ... and what a trimmed prefix would give instead
    assert CR.flags([0, 1, 0], [1, 0, 1]) == [1, 1, 0]     # a as the pivot
    assert sorted(y for _, y in CR.trace([1, 0, 1], [0, 1, 0])[0]) == [1, 2]  # a as the other row: it gets [0, 1, 1]
    assert CR.flags_suffix_trimmed([0, 0], [0]) == [0, 1] and CR.flags_suffix_trimmed([0, 1, 0], [1, 0, 1]) == [1, 1, 0]


def _rows(V, max_len):
    return [list(r) for L in range(max_len + 1) for r in itertools.product(range(V), repeat=L)]


def test_every_pair_of_short_rows():
    """V = 3, lengths <= 5: the matched pairs are strictly increasing and equal-labelled, the path costs the distance, equal rows are
    fully matched, and trimming the common suffix leaves the flags as they are"""
    rows = _rows(3, 5)
    assert len(rows) == 364
    prefix_differs = 0
    for a in rows:
        for b in rows:
            pairs, cost = CR.trace(a, b)
            back = pairs[::-1]
            assert all(p[0] < q[0] and p[1] < q[1] for p, q in zip(back, back[1:])), (a, b)
            assert all(a[x] == b[y] for x, y in pairs), (a, b)
            assert cost == M.edit_distance(a, b), (a, b)
            f = CR.flags(a, b)
            if a == b:
                assert f == [1] * len(a)
            assert CR.flags_suffix_trimmed(a, b) == f, (a, b)
            prefix_differs += CR.flags_prefix_trimmed(a, b) != f
    assert prefix_differs > 0  # the prefix may not be trimmed


def test_confidence_of_a_small_list():
    """two utterances by hand: a dead slot, a dead pivot, the pivot's own vote"""
    ids = np.array([[[5, 6, 7], [5, 9, 7], [1, 1, 1]], [[2, 3, 0], [2, 0, 0], [4, 4, 4]]], dtype=np.int64)
    n = np.array([[3, 3, 3], [2, 1, 3]], dtype=np.int32)
    score = np.array([[-1.0, -1.0, -np.inf], [-1.0, -1.0, -1.0]], dtype=np.float32)
    pivot = np.array([[0, 2], [1, 3]], dtype=np.int32)
    post, conf, hyp, match = CR.confidence(ids, n, score, 3, pivot, 4, 1.0)
    assert np.allclose(post, [0.5, 0.5, 0.0, 1 / 3, 1 / 3, 1 / 3])
    assert match[0, 0].tolist() == [[1, 1, 1], [1, 0, 1], [0, 0, 0]] and np.allclose(conf[0, 0], [1.0, 0.5, 1.0])
    assert not match[0, 1].any() and not conf[0, 1].any() and hyp[0, 1] == 0.0  # slot 2 is dead: a dead pivot
    assert match[1, 0].tolist() == [[1, 0, 0], [1, 0, 0], [0, 0, 0]] and np.allclose(conf[1, 0], [2 / 3, 0.0, 0.0])
    assert not match[1, 1].any() and hyp[1, 1] == 0.0 and np.allclose(hyp[:, 0], [0.5, 1 / 3])  # pivot 3 is outside the list


# ---------------------------------------------------------------- word_confidence
def test_word_confidence():
    from joeys2t_amd.alignment import WORD_MARKER as W
    from joeys2t_amd.confidence import word_confidence
    pieces = ["he", "llo", W + "wor", "ld", W, W + "a"]  # the first piece without a marker; a marker-only piece
    conf = np.array([0.5, 0.25, 1.0, 0.5, 0.75, 0.125, 0.9, 0.9], dtype=np.float32)  # more values than pieces: EOS, padding
    assert word_confidence(pieces, conf) == [("hello", 0.25), ("world", 0.5), ("", 0.75), ("a", 0.125)]
    assert word_confidence(pieces, conf, how="mean") == [("hello", 0.375), ("world", 0.75), ("", 0.75), ("a", 0.125)]
    assert word_confidence(pieces, conf, how="prod") == [("hello", 0.125), ("world", 0.5), ("", 0.75), ("a", 0.125)]
    assert word_confidence([], conf) == []
    with pytest.raises(ValueError, match="how 'max'"):
        word_confidence(pieces, conf, how="max")
    with pytest.raises(ValueError, match="6 pieces for 2"):
        word_confidence(pieces, conf[:2])


# ---------------------------------------------------------------- the declaration and the refusals
def test_the_header_declares_the_entry_points():
    from joeys2t_amd import _lib
    assert _lib.FUNCTIONS["js2t_nbest_confidence_workspace"] == (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64])
    restype, argtypes = _lib.FUNCTIONS["js2t_nbest_confidence"]
    assert restype is ctypes.c_int and len(argtypes) == 17
    assert argtypes[8] is ctypes.c_void_p and argtypes[10] is ctypes.c_int64 and argtypes[15] is ctypes.c_float  # uint8_t* match; bytes; scale


def _refused(rc, *words):
    from joeys2t_amd import _lib
    msg = _lib.lib().js2t_last_error()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


def test_limits_are_refused_before_anything_is_launched():
    """every limit with NULL pointers: a launch would fault; the checks come first (as test_mbr_cpu.py does for js2t_mbr_rescore)"""
    from joeys2t_amd import _lib
    L = _lib.lib()
    big = M.EDIT_MAX_LEN

    def size(B=1, P=2, N=4, Lp=9):
        return L.js2t_nbest_confidence_workspace(B, P, N, Lp)

    def conf(B=1, N=4, P=2, Lp=9, scale=1.0, stride=8, ws=None):
        ws = max(size(B, P, N, Lp), 0) if ws is None else ws
        return L.js2t_nbest_confidence(None, stride, None, None, None, None, None, None, None, None, ws, B, N, P, Lp, scale, None)

    # masks: 8 pairs * 1 word; codes: 8 pairs * 1 tile * 1 block of 16 rows * 64 lanes, 4 bytes each
    assert size() == 8 * (1 + 64) * 4 and size(Lp=1) == 0 and size(B=0) == 0
    assert size(Lp=66) == 8 * (3 + 2 * 5 * 64) * 4  # 65 labels: 3 mask words, 2 tiles of 5 blocks
    assert size(N=0) == size(N=33) == size(P=0) == size(P=5) == size(Lp=0) == size(Lp=big + 2) == size(B=-1) == -1
    _refused(conf(N=0), b"N 0")
    _refused(conf(N=33), b"N 33")
    _refused(conf(P=0), b"P 0")
    _refused(conf(P=5), b"P 5")
    _refused(conf(Lp=0), b"Lp 0")
    _refused(conf(Lp=big + 2, stride=big + 1), b"Lp - 1", str(big).encode())
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        _refused(conf(scale=scale), b"scale")
    _refused(conf(stride=7), b"ids_stride 7")
    _refused(conf(B=2**31 // 16), b"B * N * N")
    _refused(conf(ws=size() - 1), b"workspace of 2079 bytes below the 2080")
    _refused(conf(), b"null pointer")  # (the limits hold: only now are the pointers looked at)
    assert conf(B=0) == 0 and conf(B=0, N=33) != 0  # the limits are checked whatever B is
    with pytest.raises(ctypes.ArgumentError):
        L.js2t_nbest_confidence(None, 8, None, None, None, None, None, None, None, None, 0, 1, 4.5, 2, 9, 1.0, None)


@pytest.mark.parametrize("scale, what", [(0.0, "confidence_scale 0.0 not finite and above 0"), (-1.0, "confidence_scale -1.0 not finite and above 0"),
                                         (float("nan"), "confidence_scale nan not finite and above 0"),
                                         (float("inf"), "confidence_scale inf not finite and above 0")])
def test_a_bad_scale_is_refused_before_the_model_is_touched(scale, what):
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    for fn in (ctc_beam_search, ctc_attention_rescore):
        with pytest.raises(ValueError, match=fn.__name__ + ": " + what):
            fn(None, None, beam_size=4, confidence=True, confidence_scale=scale)
    for decoder in ("ctc", "ctc-attention", "attention"):
        with pytest.raises(ValueError, match="predict: " + what):
            predict(None, [None], decoder=decoder, confidence=True, confidence_scale=scale)


def test_a_scale_without_confidence_and_the_attention_decoder():
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    for fn in (ctc_beam_search, ctc_attention_rescore):
        with pytest.raises(ValueError, match=fn.__name__ + r": confidence_scale 2.0 without confidence=True"):
            fn(None, None, beam_size=4, confidence_scale=2.0)
    with pytest.raises(ValueError, match=r"predict: confidence_scale 2.0 without confidence=True"):
        predict(None, [None], decoder="ctc", confidence_scale=2.0)
    with pytest.raises(ValueError, match="confidence=True.*decoder='attention' has no such list"):
        predict(None, [None], decoder="attention", confidence=True)
    with pytest.raises(ValueError, match="return_prob='ref'"):
        predict(None, [None], decoder="ctc", confidence=True, return_prob="ref")
    with pytest.raises(ValueError, match="n_rescore 5"):  # accepted without an LM with confidence=True, and still bounded by the beam
        ctc_beam_search(None, None, beam_size=4, n_best=1, n_rescore=5, confidence=True)
    with pytest.raises(ValueError, match="n_rescore without an lm"):  # without it the call is as it was
        ctc_beam_search(None, None, beam_size=4, n_best=1, n_rescore=2)
    with pytest.raises((AttributeError, TypeError)):  # valid options get as far as the model
        ctc_beam_search(None, None, beam_size=4, n_best=1, n_rescore=2, confidence=True, confidence_scale=0.5)
