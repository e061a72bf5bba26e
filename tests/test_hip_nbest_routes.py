"""GPU: the COMBINATIONS of the n-best stages of the two CTC decoders, bit for bit against tests/golden/nbest_routes.npz - the output
of the same calls recorded (tools/record_nbest_routes.py, which takes the grid from here) before the decoders were written as one
stage chain.  The neighbours check each stage against its own reference; this file pins what the chain owns: which stages run, in
which order, on which base score and which Lp, and which parts come back.  Exact comparison is sound because the kernels are
deterministic by construction (no atomics, fixed summation orders) and the fixture was recorded twice, in two processes, with equal
bits in every field.

The grid, per golden model: route {ctc_beam_search, ctc_attention_rescore at ctc_weight 0.3} x LM {none, lm_fusion "rescore", "search"}
x context {none, the graph at weight 1.0} x decision {map, mbr} x confidence {off, on}, every call with return_parts=True, beam_size 6
and n_best 4 - and four edge rows per route: a list of one slot (beam_size = n_best = 1 under decision="mbr" with confidence: no
pairs, an empty MBR pair launch), n_rescore = 5 between n_best and the beam, a length_bonus alone without an LM, and
return_parts=False.  The models, the LM and the graph are those of test_hip_confidence.py, test_hip_ngram.py and
test_hip_ctc_beam_ctx.py, at their weights."""
import functools
import itertools
import json
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = Path(__file__).resolve().parent / "golden" / "nbest_routes.npz"
MODELS = ["model_pre", "model_post", "model_deepnet"]
SET = dict(beam_size=6, n_best=4)
CTCW, LMW, MODEL_CW, BONUS = 0.3, 0.5, 1.0, 0.5
ROUTES = ["ctc", "att"]


def grid():
    """[(call id, route, spec)]: spec holds the decoder's keyword arguments, with lm=True / context=True standing for the shared
    LM and the model's graph (`keywords` puts them in)"""
    calls = []
    for route in ROUTES:
        for lm, ctx, decision, conf in itertools.product((None, "rescore", "search"), (False, True), ("map", "mbr"), (False, True)):
            spec = dict(SET, return_parts=True, decision=decision, confidence=conf)
            if lm:
                spec.update(lm=True, lm_weight=LMW, lm_fusion=lm)
            if ctx:
                spec.update(context=True, context_weight=MODEL_CW)
            calls.append((f"{route}-lm_{lm or 'none'}-ctx_{int(ctx)}-{decision}-conf_{int(conf)}", route, spec))
        calls += [(f"{route}-one_slot", route, dict(beam_size=1, n_best=1, return_parts=True, decision="mbr", confidence=True)),
                  (f"{route}-n_rescore_5", route, dict(SET, n_rescore=5, return_parts=True, lm=True, lm_weight=LMW, decision="mbr", confidence=True)),
                  (f"{route}-bonus_alone", route, dict(SET, return_parts=True, length_bonus=BONUS)),
                  (f"{route}-no_parts", route, dict(SET, return_parts=False))]
    return calls


GRID = grid()
assert len(GRID) == 56 and len({c[0] for c in GRID}) == 56


@functools.lru_cache(maxsize=None)
def golden(name):
    """(model, golden arrays, the model's graph), once per process: do not modify"""
    from test_hip_ctc_beam_ctx import graph, model_phrases
    from test_hip_model import build
    model, g = build(name, torch.device("cuda:0"))
    model.eval()
    return model, g, graph(model_phrases(name), len(model.trg_vocab))


def keywords(name, spec):
    from test_hip_ngram import model_lm
    kw = dict(spec)
    if kw.get("lm"):
        kw["lm"] = model_lm()
    if kw.get("context"):
        kw["context"] = golden(name)[2]
    return kw


def decode(name, route, spec):
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    from test_hip_model import batch_kwargs
    model, g, _ = golden(name)
    batch = batch_kwargs(g, torch.device("cuda:0"))
    if route == "ctc":
        return ctc_beam_search(model, batch, **keywords(name, spec))
    return ctc_attention_rescore(model, batch, ctc_weight=CTCW, **keywords(name, spec))


def as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def fields(result):
    """{field: integer array} of a decoder's return value: ids, lengths, the scores' bit patterns, every part as bit patterns under
    "parts.<key>", a ragged list of arrays concatenated with its lengths under "parts.<key>.lengths"; sorted by name"""
    out = {"ids": result[0], "scores": as_bits(result[1]), "lengths": result[2]}
    assert len(result) in (3, 4)
    for key, val in (result[3] if len(result) == 4 else {}).items():
        if isinstance(val, list):
            out[f"parts.{key}.lengths"] = np.array([len(v) for v in val], dtype=np.int64)
            val = np.concatenate(val) if val else np.zeros((0, ), dtype=np.float32)
        out[f"parts.{key}"] = as_bits(val)
    assert all(v.dtype.kind == "i" for v in out.values()), {k: v.dtype for k, v in out.items()}
    return dict(sorted(out.items()))


def pack(results):
    """{(model, call id): fields} -> the arrays of the .npz: per call ONE i64 vector (every field flattened, in name order) and, once,
    the layout as JSON: {"model/call": [[field, dtype, shape], ...]}"""
    arrays, layout = {}, {}
    for (name, call), f in results.items():
        layout[f"{name}/{call}"] = [[k, v.dtype.str, list(v.shape)] for k, v in f.items()]
        arrays[f"{name}/{call}"] = np.concatenate([v.reshape(-1).astype(np.int64) for v in f.values()])
    arrays["layout"] = np.array(json.dumps(layout))
    return arrays


@functools.lru_cache(maxsize=None)
def recorded():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}, json.loads(str(z["layout"]))


def differences(f, blob, layout):
    """the fields of `f` that are not the recorded ones: a list of descriptions, empty when every key, dtype, shape and bit is"""
    if [k for k, _, _ in layout] != list(f):
        return [f"keys {list(f)} against the recorded {[k for k, _, _ in layout]}"]
    bad, at = [], 0
    for k, dtype, shape in layout:
        size = int(np.prod(shape))
        want = blob[at:at + size].astype(np.dtype(dtype)).reshape(shape)
        at += size
        if f[k].dtype.str != dtype or list(f[k].shape) != shape:
            bad.append(f"{k}: {f[k].dtype.str} {list(f[k].shape)} against the recorded {dtype} {shape}")
        elif not np.array_equal(f[k], want):
            bad.append(f"{k}: {int((f[k] != want).sum())} of {size} values differ, first at {np.argwhere(f[k] != want)[0].tolist()}")
    assert at == blob.size
    return bad


def test_the_fixture_holds_the_whole_grid():
    arrays, layout = recorded()
    assert sorted(layout) == sorted(f"{name}/{call}" for name in MODELS for call, _, _ in GRID) and len(arrays) == len(layout) + 1


@pytest.mark.parametrize("call", [c[0] for c in GRID])
@pytest.mark.parametrize("name", MODELS)
def test_route_gives_the_recorded_bits(device, name, call):
    arrays, layout = recorded()
    _, route, spec = next(c for c in GRID if c[0] == call)
    f = fields(decode(name, route, spec))
    assert ("parts.map_rank" in f) == (spec["return_parts"] and (route == "ctc" or spec.get("decision") == "mbr"))  # the parts did come back
    assert not differences(f, arrays[f"{name}/{call}"], layout[f"{name}/{call}"]), (name, call)
