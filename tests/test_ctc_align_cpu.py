"""CPU: the float64 reference of CTC forced alignment (tests/ctc_align_reference.py) pinned by brute-force enumeration of frame
labellings and by a hand-checked known answer that exercises the tie rule; the host-side parts of joeys2t_amd.alignment; the C ABI
declares the aligner."""
import itertools

import numpy as np
import pytest

import ctc_align_reference as R
from joeys2t_amd import alignment
from joeys2t_amd._lib import declared_symbols

KNOWN_TARGET = [2, 3, 3, 4]
KNOWN_PATH_10 = [1, 3, 4, 5, 7, 8, 8, 8, 8, 8]


def test_header_declares_the_aligner():
    names = declared_symbols()
    assert "js2t_ctc_align" in names and "js2t_ctc_align_workspace_bytes" in names


@pytest.mark.parametrize("target", [[], [1], [2], [1, 2], [2, 1], [1, 1], [2, 2]])
def test_reference_against_enumeration(target):
    """V = 3, blank 0, T <= 6: every one of the V^T frame labellings that collapses to the target is a path; the largest of their
    scores is the reference's score and the reference's path is one of the maximisers (random logits: no exact ties expected, but the
    check does not rely on that)."""
    V, blank = 3, 0
    rs = np.random.RandomState(17 + 31 * len(target) + sum(target))
    for T in range(1, 7):
        logp = R.log_softmax(rs.randn(T, V) * 2.0)
        scores = {lab: float(logp[np.arange(T), list(lab)].sum()) for lab in itertools.product(range(V), repeat=T)
                  if R.collapse(lab, blank) == target}
        got = R.align(logp, target, blank)
        if not scores:
            assert got["path"] is None and got["score"] == -np.inf, (T, target)
            continue
        best = max(scores.values())
        assert abs(got["score"] - best) <= 1e-12 * max(1.0, abs(best)), (T, target, got["score"], best)
        R.check_path(got["path"], target, blank)
        labels = tuple(int(v) for v in R.extended(target, blank)[got["path"]])
        assert scores[labels] >= best - 1e-12 * max(1.0, abs(best))
        assert abs(R.path_score(logp, target, blank, got["path"]) - got["score"]) <= 1e-12 * max(1.0, abs(best))
        assert np.allclose(got["frame_logp"].sum(), got["score"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_known_answer(dtype):
    """uniform logits: every complete path ties, so the answer is the tie rule's - end in S-1, stay as long as staying is possible"""
    V, blank = 6, 0
    got = R.align(R.log_softmax(np.zeros((10, V)), dtype), KNOWN_TARGET, blank, dtype)
    assert got["path"].tolist() == KNOWN_PATH_10
    assert got["tok_start"].tolist() == [0, 1, 3, 4] and got["tok_end"].tolist() == [1, 2, 4, 5]
    assert abs(float(got["score"]) + 10 * np.log(6.0)) <= 1e-5
    got = R.align(R.log_softmax(np.zeros((5, V)), dtype), KNOWN_TARGET, blank, dtype)
    assert got["path"].tolist() == [1, 3, 4, 5, 7]
    got = R.align(R.log_softmax(np.zeros((4, V)), dtype), KNOWN_TARGET, blank, dtype)
    assert got["path"] is None and got["score"] == -np.inf


def test_reference_label_outside_the_vocabulary_and_no_frames():
    logp = R.log_softmax(np.random.RandomState(0).randn(6, 5))
    assert R.align(logp, [1, 7], 0)["score"] == -np.inf
    assert R.align(logp[:0], [], 0)["score"] == -np.inf
    got = R.align(logp, [], 0)  # no labels: the all-blank path
    assert got["path"].tolist() == [0] * 6 and abs(got["score"] - logp[:, 0].sum()) < 1e-12


def test_hypothesis_lengths():
    ids = np.array([[5, 6, 3, 1, 1], [5, 3, 7, 3, 1], [1, 1, 1, 1, 1], [5, 6, 7, 8, 9], [5, 1, 3, 1, 1]])
    assert alignment.hypothesis_lengths(ids, eos_index=3, pad_index=1).tolist() == [3, 2, 0, 5, 1]


def test_word_segments_known_answer():
    a = alignment.Alignment(tokens=[10, 11, 12, 13, 3], start_frame=[1, 3, 4, 9, 12], end_frame=[3, 4, 6, 10, 13],
                            start=[0.04, 0.12, 0.16, 0.36, 0.48], end=[0.12, 0.16, 0.24, 0.40, 0.52],
                            logp=[-0.5, -1.0, -0.25, -2.0, -0.1], score=-7.0)
    words = alignment.word_segments(["▁he", "llo", "▁wor", "ld"], a)  # the EOS has no piece
    assert [w[0] for w in words] == ["hello", "world"]
    assert [(w[1], w[2]) for w in words] == [(0.04, 0.16), (0.16, 0.40)]
    assert words[0][3] == pytest.approx((-0.5 * 2 - 1.0 * 1) / 3) and words[1][3] == pytest.approx((-0.25 * 2 - 2.0 * 1) / 3)
    assert alignment.word_segments(["he", "▁", "▁x"], a)[1][0] == ""  # a bare marker is a word of its own
    with pytest.raises(ValueError):
        alignment.word_segments(["a"] * 6, a)
