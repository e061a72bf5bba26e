"""CPU: the contextual-biasing options of search.ctc_beam_search, search.ctc_attention_rescore and prediction.predict are refused
before the model is touched (the model here is None), and the defaults leave the three signatures as they were."""
import inspect

import pytest

from joeys2t_amd.biasing import ContextGraph

GRAPH = ContextGraph.from_phrases([(5, 6)], 20)


@pytest.mark.parametrize("kw, what", [
    (dict(context_weight=1.0), "context_weight 1.0 without a context graph"),
    (dict(context_weight=-0.5), "context_weight -0.5 without a context graph"),
    (dict(context=GRAPH, context_weight=float("nan")), "context_weight nan not finite"),
    (dict(context=GRAPH, context_weight=float("inf")), "context_weight inf not finite"),
    (dict(context_weight=float("-inf")), "context_weight -inf not finite"),
])
def test_refused_before_the_model_is_touched(kw, what):
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    for fn in (ctc_beam_search, ctc_attention_rescore):
        with pytest.raises(ValueError, match=f"{fn.__name__}: {what}"):
            fn(None, None, beam_size=4, **kw)
    for decoder in ("ctc", "ctc-attention", "attention"):
        with pytest.raises(ValueError, match=f"predict: {what}"):
            predict(None, [None], decoder=decoder, **kw)


def test_the_attention_decoder_refuses_a_graph():
    from joeys2t_amd.prediction import predict
    with pytest.raises(ValueError, match="context / context_weight bias the CTC beam.*decoder='attention' has none"):
        predict(None, [None], decoder="attention", context=GRAPH, context_weight=1.0)
    with pytest.raises(ValueError, match="decoder='attention' has none"):
        predict(None, [None], decoder="attention", context=GRAPH)


def test_the_other_refusals_still_come_first_and_valid_options_reach_the_model():
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    with pytest.raises(ValueError, match="lm_weight 0.5 without an lm"):
        ctc_beam_search(None, None, beam_size=4, lm_weight=0.5, context=GRAPH, context_weight=1.0)
    with pytest.raises(ValueError, match="n_rescore without an lm or a length_bonus"):  # biasing alone makes no list to re-rank
        ctc_beam_search(None, None, beam_size=4, n_rescore=2, context=GRAPH, context_weight=1.0)
    with pytest.raises(ValueError, match="lm_fusion='search' without an lm or a length_bonus"):  # and is no LM
        ctc_beam_search(None, None, beam_size=4, lm_fusion="search", context=GRAPH, context_weight=1.0)
    for fn in (ctc_beam_search, ctc_attention_rescore):
        with pytest.raises((AttributeError, TypeError)):  # valid options get as far as the model
            fn(None, None, beam_size=4, context=GRAPH, context_weight=1.0)
        with pytest.raises((AttributeError, TypeError)):  # a graph with weight 0 is no biasing and no error
            fn(None, None, beam_size=4, context=GRAPH)


def test_defaults_and_positions():
    """the new options are keyword arguments at the end, off by default: no existing call changes"""
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    for fn in (ctc_beam_search, ctc_attention_rescore, predict):
        p = inspect.signature(fn).parameters
        assert list(p)[-2:] == ["context", "context_weight"] and p["context"].default is None and p["context_weight"].default == 0.0
