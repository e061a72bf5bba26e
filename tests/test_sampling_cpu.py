"""Sampling from the attention decoder, as far as no device is needed: the float64 reference pinned by enumeration, the truncations'
algebra, the pinned cases' decidability, the header / library binding, and every refusal that must fire before a launch or before the
model is touched."""
import ctypes
import inspect

import numpy as np
import pytest

import sampling_reference as S


def _row(seed, V=6, scale=2.0):
    return (scale * np.random.RandomState(seed).randn(V)).astype(np.float32)


GRID = 2000
SETTINGS = [dict(T=1.0, k=0, p=1.0, eps=0.0), dict(T=0.7, k=4, p=1.0, eps=0.0), dict(T=1.0, k=0, p=0.8, eps=0.0),
            dict(T=1.3, k=0, p=1.0, eps=0.1), dict(T=0.8, k=5, p=0.85, eps=0.03)]


@pytest.mark.parametrize("kw", SETTINGS)
def test_the_reference_partitions_the_unit_interval(kw):
    """V = 6, a grid of 2000 values of u: the drawn ids cut [0, 1) into intervals of width q_v in id order, dropped tokens get measure
    0, and the kept set is the brute-force "sort, renormalise, cut" """
    for seed in range(5):
        row, forbid = _row(seed), (seed % 6, )
        kept = S.brute_force_kept(row, kw["T"], kw["k"], kw["p"], kw["eps"], forbid)
        one = S.ref(row, 0.5, forbid=forbid, **kw)
        assert sorted(one["order"].tolist()) == sorted(kept) and one["order"].tolist() == kept and one["kept"] == len(kept)
        z = row.astype(np.float64) / kw["T"]
        mass = {v: np.exp(z[v] - z[kept[0]]) for v in kept}
        W = sum(mass.values())
        ids = [S.ref(row, (i + 0.5) / GRID, forbid=forbid, **kw)["id"] for i in range(GRID)]
        assert ids == sorted(ids) and set(ids) <= set(kept)  # id order; nothing dropped is ever drawn
        for v in range(6):
            want = mass[v] / W if v in mass else 0.0
            got = ids.count(v) / GRID
            assert abs(got - want) <= 1.0 / GRID + 1e-12, (v, got, want)
            if v not in mass:
                assert got == 0
        for i in (0, GRID // 3, GRID - 1):
            r = S.ref(row, (i + 0.5) / GRID, forbid=forbid, **kw)
            assert r["cdf"][0] <= (i + 0.5) / GRID < r["cdf"][1]
            assert abs(np.exp(r["q"]) - (r["cdf"][1] - r["cdf"][0])) < 1e-12
            lse = np.log(np.exp(row.astype(np.float64)).sum())
            assert abs(r["logp"] - (float(row[r["id"]]) - lse)) < 1e-12  # the model's log-probability: forbidden ids stay in the sum


def test_truncations_are_prefixes_of_one_order_and_commute():
    for seed in range(8):
        row = _row(seed, V=23, scale=3.0)
        full = S.ref(row, 0.3)["order"].tolist()
        assert len(full) == 23 and all(row[a] > row[b] or (row[a] == row[b] and a < b) for a, b in zip(full, full[1:]))
        for kw in (dict(k=7), dict(p=0.7), dict(eps=0.05), dict(T=0.5, k=9, p=0.9, eps=0.01), dict(T=2.0, p=0.5, eps=0.02)):
            got = S.ref(row, 0.3, **kw)
            assert got["order"].tolist() == full[:got["kept"]]  # a prefix of the one order, whatever the temperature
            assert got["n0"] == min(got["n_eps"], got["n_k"])
        # the switches are identities
        base = S.ref(row, 0.3, T=0.9, k=6, p=0.8, eps=0.02)
        assert S.ref(row, 0.3, T=0.9, k=0, p=1.0, eps=0.0)["kept"] == 23
        assert S.ref(row, 0.3, T=0.9, k=23, p=0.8, eps=0.02)["kept"] == S.ref(row, 0.3, T=0.9, k=0, p=0.8, eps=0.02)["kept"]
        only_k = S.ref(row, 0.3, T=0.9, k=6)
        only_e = S.ref(row, 0.3, T=0.9, eps=0.02)
        assert S.ref(row, 0.3, T=0.9, k=6, eps=0.02)["kept"] == min(only_k["kept"], only_e["kept"])  # top-k and epsilon commute
        assert base["kept"] <= min(only_k["kept"], only_e["kept"])  # the nucleus is taken of what they leave
    tie = np.array([1.0, 3.0, 3.0, 0.0, 3.0], np.float32)
    assert S.ref(tie, 0.1, k=2)["order"].tolist() == [1, 2]  # equal logits across the boundary enter in id order
    assert S.ref(tie, 0.999, k=2)["id"] == 2 and S.ref(tie, 0.0, k=2)["id"] == 1


def test_edge_rules_of_the_reference():
    row = np.array([0.5, np.nan, -np.inf, 2.0, 1.0], np.float32)
    assert S.ref(row, 0.5)["n_a"] == 3
    r = S.ref(row, 0.5, forbid=(0, 3, 4))
    assert r["id"] is None and r["logp"] == -np.inf and r["kept"] == 0 and r["cdf"] == (0.0, 0.0)
    assert S.ref(row, 0.5, forbid=(0, 3))["id"] == 4  # all but one forbidden
    assert S.ref(row, np.nan)["id"] == S.ref(row, 0.0)["id"] == 0 and S.ref(row, 7.0)["id"] == S.ref(row, S.U_MAX)["id"] == 4
    assert S.ref(row, 0.9, eps=0.999)["kept"] == 1  # epsilon keeps at least one


@pytest.mark.parametrize("name", list(S.CASES))
def test_pinned_cases_are_decidable(name):
    c = S.CASES[name]
    assert 2 <= c["V"] <= S.MAX_V and 0 <= c["n_forbid"] <= 3
    assert S.find_seed(name) == S.SEEDS[name]  # the first decidable seed from the base
    rows = S.case_reference(name)
    live = [r for r in rows if r is not None]
    assert all(S.decidable(r) for r in live) and len(live) == c["rows"] - (len(S.FINISHED_ROWS) if c.get("special") else 0)
    inp = S.case_inputs(name)
    assert all(r["id"] not in inp["forbid"] for r in live) and all(0 <= r["id"] < c["V"] for r in live)
    if c.get("special"):
        assert np.isnan(inp["logits"][list(S.FINISHED_ROWS)]).all() and np.isinf(inp["logits"][1]).any() and np.isnan(inp["logits"][5]).any()
    print(name, "seed", S.SEEDS[name], "kept", min(r["kept"] for r in live), "..", max(r["kept"] for r in live),
          "least u margin / TAU_MASS", round(min(r["u_margin"] for r in live) / S.TAU_MASS, 1))


# ---------------------------------------------------------------- the feature, as far as no device is needed
def test_header_declares_and_library_exports_the_entry_point():
    from joeys2t_amd import _lib
    assert "js2t_sample_step" in _lib.declared_symbols() and hasattr(_lib.lib(), "js2t_sample_step")
    restype, argtypes = _lib.FUNCTIONS["js2t_sample_step"]
    assert restype is _lib.C.c_int and len(argtypes) == 24
    assert argtypes[1] is _lib.C.c_int64 and argtypes[6] is _lib.C.c_int32 and argtypes[17] is _lib.C.c_float and argtypes[18] is _lib.C.c_int32
    from joeys2t_amd import ops, search
    assert callable(ops.sample_step) and callable(search.sample_search) and ops.SAMPLE_MAX_V == S.MAX_V


def _refused(rc, *words):
    from joeys2t_amd import _lib
    msg = _lib.lib().js2t_last_error()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


def test_limits_are_refused_before_anything_is_launched():
    """every limit with NULL pointers: a launch would fault; the checks come first"""
    from joeys2t_amd import _lib
    L = _lib.lib()

    def call(rows=1, V=11, ids_ld=4, step=0, n_forbid=0, T=1.0, k=0, p=1.0, eps=0.0, eos=2, pad=1):
        return L.js2t_sample_step(None, V, None, None, None, ids_ld, step, None, None, None, None, None, None, rows, V, None, n_forbid, T, k,
                                  p, eps, eos, pad, None)

    _refused(call(V=1), b"vocabulary 1")
    _refused(call(V=65537), b"vocabulary 65537")
    _refused(call(n_forbid=17), b"forbidden")
    _refused(call(n_forbid=-1), b"forbidden")
    for T in (0.0, -1.0, float("nan"), float("inf")):
        _refused(call(T=T), b"temperature")
    _refused(call(k=-1), b"top_k -1")
    for p in (0.0, -0.5, 1.5, float("nan")):
        _refused(call(p=p), b"top_p")
    for eps in (-0.1, 1.0, float("nan")):
        _refused(call(eps=eps), b"epsilon")
    _refused(call(step=-1), b"step -1")
    _refused(call(step=4), b"step 4")
    _refused(call(eos=11), b"eos 11")
    _refused(call(eos=-1), b"eos -1")
    _refused(call(pad=11), b"pad 11")
    _refused(call(rows=-1), b"row count -1")
    _refused(call(), b"null pointer")  # (the limits hold: only now are the pointers looked at)
    assert call(rows=0) == 0 and call(rows=0, V=65536, k=10**6) == 0
    assert call(rows=0, V=1) != 0 and call(rows=0, p=0.0) != 0  # the limits are checked whatever the row count is
    with pytest.raises(ctypes.ArgumentError):
        call(k=1.5)


BAD = [(dict(n_samples=0), "n_samples 0"), (dict(temperature=0.0), "temperature 0.0"), (dict(temperature=float("nan")), "temperature nan"),
       (dict(temperature=float("inf")), "temperature inf"), (dict(top_k=-1), "top_k -1"), (dict(top_k=2.5), "top_k 2.5"),
       (dict(top_p=0.0), "top_p 0.0"), (dict(top_p=1.01), "top_p 1.01"), (dict(epsilon=1.0), "epsilon 1.0"),
       (dict(epsilon=-0.1), "epsilon -0.1")]


@pytest.mark.parametrize("kw, what", BAD)
def test_sampling_options_are_refused_before_the_model_is_touched(kw, what):
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import sample_search
    with pytest.raises(ValueError, match="sample_search: " + what):
        sample_search(None, None, **kw)
    with pytest.raises(ValueError, match="predict: " + what):
        predict(None, [None], decoder="sample", **kw)


def test_sample_search_refusals():
    from joeys2t_amd.search import sample_search

    class Prompted:
        trg_prompt_mask = object()

    class NoTransformer:
        class decoder:
            pass

    for kw, what in [(dict(decision="map"), "decision 'map'"), (dict(n_samples=4, n_best=5), "n_best 5"), (dict(n_samples=4, n_best=0), "n_best 0"),
                     (dict(n_samples=4, n_best=2), "n_best 2 with decision='none'"), (dict(n_samples=1, decision="mbr"), "decision='mbr' ranks 2..32 samples"),
                     (dict(n_samples=33, decision="mbr"), "decision='mbr' ranks 2..32 samples")]:
        with pytest.raises(ValueError, match="sample_search: " + what):
            sample_search(None, None, **kw)
    with pytest.raises(ValueError, match="sample_search: a prompted batch"):
        sample_search(None, Prompted(), n_samples=2)
    with pytest.raises(ValueError, match="sample_search: .*no Transformer decoder"):
        sample_search(NoTransformer(), None, n_samples=2)
    with pytest.raises((AttributeError, TypeError)):  # valid options get as far as the model
        sample_search(None, None, n_samples=8, temperature=0.8, top_k=10, top_p=0.9, epsilon=0.01, decision="mbr", n_best=3)


def test_predict_takes_the_sample_decoder_and_refuses_what_does_not_belong():
    from joeys2t_amd.prediction import predict
    params = inspect.signature(predict).parameters
    assert list(params)[-2:] == ["context", "context_weight"]
    want = dict(n_samples=1, temperature=1.0, top_k=0, top_p=1.0, epsilon=0.0, seed=0)
    assert {k: params[k].default for k in want} == want
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in want)
    for decoder in ("attention", "ctc", "ctc-attention"):  # the six options belong to decoder="sample"
        for kw in (dict(n_samples=2), dict(temperature=0.5), dict(top_k=3), dict(top_p=0.9), dict(epsilon=0.01), dict(seed=1)):
            with pytest.raises(ValueError, match="belong to decoder='sample'"):
                predict(None, [None], decoder=decoder, **kw)
    for kw, what in [(dict(lm_weight=0.5), "lm / lm_weight"), (dict(length_bonus=0.1), "lm / lm_weight"), (dict(context=object(), context_weight=1.0), "context"),
                     (dict(confidence=True), "confidence"), (dict(ctc_candidates=4), "ctc_candidates"), (dict(ctc_weight=0.5), "ctc_candidates / ctc_weight"),
                     (dict(beam_alpha=1.0), "beam_alpha"), (dict(repetition_penalty=1.2), "repetition_penalty"),
                     (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"), (dict(return_attention=True), "return_attention"),
                     (dict(decision="mbr", mbr_scale=2.0, n_samples=4), "mbr_scale")]:
        with pytest.raises(ValueError, match="predict: " + what):
            predict(None, [None], decoder="sample", **kw)
    with pytest.raises(ValueError, match="lm_fusion"):
        predict(None, [None], decoder="sample", lm_fusion="search")
    with pytest.raises(ValueError, match="n_best 1 must equal n_samples 4"):
        predict(None, [None], decoder="sample", n_samples=4)
    with pytest.raises(ValueError, match="decision='mbr' ranks 2..32 samples"):
        predict(None, [None], decoder="sample", decision="mbr")
    with pytest.raises(ValueError, match="decision='mbr' ranks 2..32 samples"):
        predict(None, [None], decoder="sample", decision="mbr", n_samples=4, n_best=5)
    with pytest.raises(ValueError, match="decoder 'x' is none of"):
        predict(None, [None], decoder="x")
    with pytest.raises((AttributeError, TypeError)):  # valid options get as far as the model
        predict(None, [None], decoder="sample", decision="mbr", n_samples=8, n_best=3, temperature=0.9, epsilon=0.02, seed=3)
    with pytest.raises((AttributeError, TypeError)):
        predict(None, [None], decoder="sample", n_samples=4, n_best=4, top_k=10)
