"""CPU: the host side of phrase spotting (joeys2t_amd.spotting) - the piece lookup, and the refusals that are raised before the
device is touched.  The kernel and the end-to-end path are in test_hip_ctc_spot.py."""
import pytest


def test_find_phrases_refusals_touch_no_device():
    """every ValueError of spotting.find_phrases is raised before a tensor is looked at: the stream here is not even one"""
    from joeys2t_amd import spotting
    for phrases, word in (([[]], "empty"), ([[5], list(range(1, 34))], "more than 32"), ([[[5, 6]]], "1-d integer"), ([[5.0]], "1-d integer")):
        with pytest.raises(ValueError, match=word):
            spotting.find_phrases(None, phrases, 0, 0.04)
    for threshold in (0.0, 1.5, float("nan"), -1.0):
        with pytest.raises(ValueError, match="threshold"):
            spotting.find_phrases(None, [[5]], 0, 0.04, threshold=threshold)
    with pytest.raises(ValueError, match="max_hits"):
        spotting.find_phrases(None, [[5]], 0, 0.04, max_hits=0)
    with pytest.raises(ValueError, match="stream"):
        spotting.find_phrases(None, [[5]], 0, 0.04)


def test_phrases_from_text():
    from joeys2t_amd import spotting
    from joeys2t_amd.biasing import ContextGraph
    from joeys2t_amd.vocabulary import Vocabulary
    vocab = Vocabulary.synthetic(20)
    toks = ["tok1", "tok2", "tok3"]  # ids 5, 6, 7 behind the four specials
    given = [" ".join(toks), [toks[0], toks[2]], toks[1] + " no-such-piece", toks[2]]
    ids, dropped = spotting.phrases_from_text(given, vocab)
    assert dropped == 1 and ids == [[5, 6, 7], [5, 7], [7]]
    assert ContextGraph.from_text(given, vocab).dropped == dropped  # (the same dropping rule)


def test_spot_long_is_exported():
    import joeys2t_amd
    from joeys2t_amd import long_form
    assert joeys2t_amd.spot_long is long_form.spot_long and "spot_long" in joeys2t_amd.__all__
