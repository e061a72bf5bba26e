"""CPU: the n-gram LM's host side (joeys2t_amd/lm.py: ARPA reader, table builder, save / load) and the float64 reference of
js2t_ngram_rescore (tests/ngram_reference.py), pinned by a property a wrong back-off rule cannot satisfy: a normalised back-off LM
scored by the reference sums to 1 over the vocabulary for EVERY context.  Also the decidability of every input the GPU tests
(tests/test_hip_ngram.py) compare orders exactly on, and the argument validation that needs no device."""
import itertools
import math
from pathlib import Path

import numpy as np
import pytest

import ngram_reference as G

ARPA = Path(__file__).resolve().parent / "golden" / "tiny_lm.arpa"
LN10 = math.log(10.0)


def test_header_declares_the_entry_point():
    from joeys2t_amd import _lib
    C = _lib.C
    assert "js2t_ngram_rescore" in _lib.declared_symbols()
    restype, argtypes = _lib.FUNCTIONS["js2t_ngram_rescore"]
    p, i64, i32, f = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    assert restype is C.c_int
    assert argtypes == [p, i64, p, p, p, p, i64, i32, i32, p, p, p, p, i64, i32, i64, i64, i64, i64, f, f, p]


# ---------------------------------------------------------------- the pin
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_the_reference_is_normalised_for_every_context(order):
    """V = 6: for every context of length 0 .. order - 1, stored or not, sum_w p(w | ctx) = 1 to 1e-12.  Back-off taken from the
    wrong gram, added after a hit, or a missing context treated as -inf all break this."""
    V = 6
    lm = G.make_lm(V, order, 10 + order, 0.6)
    assert G.lm_order(lm) == order and all((w, ) in lm for w in range(V))
    stored = unstored = 0
    worst = 0.0
    for k in range(order):
        for ctx in itertools.product(range(V), repeat=k):
            total = sum(math.exp(G.token_logp(lm, w, ctx, V, order)) for w in range(V))
            worst = max(worst, abs(total - 1.0))
            stored += ctx in lm or k == 0
            unstored += k > 0 and ctx not in lm
    print(f"order {order}: {len(lm)} n-grams, {stored} stored and {unstored} missing contexts, worst |sum - 1| {worst:.2e}")
    assert worst <= 1e-12
    assert order < 3 or (stored > V + 1 and unstored > 0)  # both kinds were seen
    # a longer history than the order gives what its last order - 1 tokens give, and an id outside the vocabulary cuts the context
    assert G.token_logp(lm, 1, (0, 1, 2, 3, 4), V, order) == G.token_logp(lm, 1, (0, 1, 2, 3, 4)[6 - order:], V, order)
    assert G.token_logp(lm, 1, (2, V + 5, 4), V, order) == G.token_logp(lm, 1, (4, )[:order - 1], V, order)
    assert G.token_logp(lm, V, (1, ), V, order) == -np.inf and G.token_logp(lm, -1, (1, ), V, order) == -np.inf


def test_known_answer_of_the_back_off_rule():
    """worked by hand: bigram (0, 1) stored, context 1 has back-off -0.5, context (0, 1) has -0.25"""
    lm = {(0, ): (-1.0, -0.125), (1, ): (-2.0, -0.5), (2, ): (-3.0, 0.0), (0, 1): (-0.75, -0.25), (1, 2): (-0.3, 0.0)}
    assert G.token_logp(lm, 1, (0, ), 3, 3) == -0.75                   # a hit: no back-off is added
    assert G.token_logp(lm, 2, (0, 1), 3, 3) == -0.25 + -0.3           # (0, 1, 2) missing: back-off of (0, 1), then the hit (1, 2)
    assert G.token_logp(lm, 0, (0, 1), 3, 3) == -0.25 + -0.5 + -1.0    # down to the unigram
    assert G.token_logp(lm, 0, (2, 2), 3, 3) == 0.0 + 0.0 + -1.0       # context (2, 2) not stored: back-off 0, not -inf
    assert G.token_logp(lm, 2, (0, 1), 3, 2) == -0.3                   # order 2 sees one token of context
    assert G.token_logp(lm, 2, (0, 1), 3, 1) == -3.0
    ids, n, base = np.array([[1, 2, 9], [1, 0, 0]]), np.array([2, 1]), np.array([-1.0, -2.0])
    tok, lms, score, order = G.rescore(ids, n, base, 2, 3, lm, 3, 3, 0, 2, 0.5, 0.25)
    # slot 0: p(1 | 0) p(2 | 0 1) p(eos = 2 | 1 2): the last one backs off from (1, 2) [0] and from (2) [0] to the unigram
    assert np.allclose(tok[0], [-0.75, -0.55, -3.0], atol=1e-15) and np.allclose(tok[1], [-0.75, -0.55, 0.0], atol=1e-15)
    assert np.allclose(lms, [-4.3, -1.3], atol=1e-15)
    assert np.allclose(score, [-1.0 + 0.5 * -4.3 + 0.5, -2.0 + 0.5 * -1.3 + 0.25], atol=1e-15) and order.tolist() == [[1, 0]]


def test_dead_slots_and_weights_of_zero():
    lm = G.make_lm(6, 3, 3, 0.5)
    ids = np.full((4, 3), 2**40 + 5, dtype=np.int64)  # whatever is not read
    ids[0, 0] = 4
    n, base = np.array([1, 1, 3, -1]), np.array([-2.0, -np.inf, -1.0, -1.0])
    tok, lms, score, order = G.rescore(ids, n, base, 4, 3, lm, 6, 3, G.BOS, G.EOS, 0.5, 0.0)
    assert np.isfinite(score[0]) and (score[1:] == -np.inf).all() and (lms[1:] == -np.inf).all() and (tok[1:] == 0).all()
    assert order.tolist() == [[0, 1, 2, 3]]  # the dead ones last, in slot order
    ids[0, 0] = 9  # outside the vocabulary: -inf at any weight but 0
    assert G.rescore(ids, n, base, 4, 3, lm, 6, 3, G.BOS, G.EOS, 0.5, 0.0)[2][0] == -np.inf
    tok0, lm0, s0, _ = G.rescore(ids, n, base, 4, 3, lm, 6, 3, G.BOS, G.EOS, 0.0, 0.0)
    assert s0[0] == -2.0 and lm0[0] == 0.0 and not tok0.any()  # the model is left out, base's own number comes back
    assert G.rescore(ids, n, base, 4, 3, lm, 6, 3, G.BOS, G.EOS, 0.0, 0.5)[2][0] == -2.0 + 0.5 * 1


# ---------------------------------------------------------------- ARPA
def vocab():
    from joeys2t_amd.vocabulary import Vocabulary
    return Vocabulary(["a", "b", "c"])  # <unk> 0 <pad> 1 <s> 2 </s> 3 a 4 b 5 c 6


def test_read_arpa_and_from_arpa():
    from joeys2t_amd.lm import NGramLM, read_arpa
    arpa = read_arpa(ARPA)
    assert arpa.order == 3 and arpa.counts == {1: 7, 2: 8, 3: 4} and len(arpa.ngrams) == 19
    assert arpa.ngrams[("<s>", )] == (-99.0, -0.5) and arpa.ngrams[("c", )] == (-0.9, 0.0)  # a missing back-off is 0
    assert arpa.ngrams[("<unk>", "a")] == (-1.1, 0.0) and arpa.ngrams[("a", "b", "</s>")] == (-0.45, 0.0)  # space separated lines
    assert read_arpa(ARPA.read_text().splitlines()).ngrams == arpa.ngrams
    lm = NGramLM.from_arpa(ARPA, vocab())
    U, P, S, E, a, b, c = range(7)
    want = {(S, ): (-99, -0.5), (E, ): (-1.0, 0), (U, ): (-1.5, -0.25), (a, ): (-0.6, -0.4), (b, ): (-0.7, -0.3), (c, ): (-0.9, 0),
            (P, ): (-1.5, 0),  # no unigram in the file: <unk>'s log-probability, back-off 0
            (S, a): (-0.3, -0.2), (S, b): (-0.5, 0), (a, b): (-0.4, -0.15), (a, E): (-0.8, 0), (b, a): (-0.35, -0.1), (b, E): (-0.6, 0),
            (U, a): (-1.1, 0), (S, a, b): (-0.2, 0), (a, b, a): (-0.25, 0), (a, b, E): (-0.45, 0)}
    assert lm.order == 3 and lm.V == 7 and lm.n_entries == 10 and lm.dropped == 3 and lm.dropped_tokens == ("zz", )
    assert lm.capacity == 32 and lm.capacity * 0.5 >= lm.n_entries and 1 <= lm.max_probe <= lm.capacity
    for g, (lp, bo) in want.items():
        lp32, bo32 = np.float32(lp * LN10), np.float32(bo * LN10)  # converted in float64, rounded to f32 once
        if len(g) == 1:
            assert lm.uni[g[0], 0] == lp32 and lm.uni[g[0], 1] == bo32, g
        else:
            assert G.table_lookup(lm, g)[:2] == (float(lp32), float(bo32)), g
    assert int((lm.table["key"] != 0).sum()) == 10
    for g in [(a, a), (a, c), (S, a, a), (b, a, b), (c, c, c)]:
        assert G.table_lookup(lm, g)[0] is None
    # scoring "a b" after <s>: the trigram, then </s> by the trigram (a b </s>)
    assert abs(G.table_token_logp(lm, b, [S, a], 7, 3) - -0.2 * LN10) < 1e-6
    assert abs(G.table_token_logp(lm, c, [S, a], 7, 3) - (-0.2 - 0.4 - 0.9) * LN10) < 1e-6  # back-offs of (<s> a) and (a), then c
    no_unk = [ln for ln in ARPA.read_text().splitlines() if "<unk>" not in ln]
    no_unk = [ln.replace("ngram 1=7", "ngram 1=6").replace("ngram 2=8", "ngram 2=7") for ln in no_unk]
    lm2 = NGramLM.from_arpa(no_unk, vocab(), oov_log10=-7.0)
    assert lm2.uni[P, 0] == np.float32(-7.0 * LN10) and lm2.uni[U, 0] == np.float32(-7.0 * LN10) and lm2.uni[U, 1] == 0


@pytest.mark.parametrize("edit, what", [
    (lambda t: t.replace("ngram 2=8", "ngram 2=9"), r"line 5.*ngram 2=9.*holds 8"),
    (lambda t: t.replace("-0.9\tc\n", "-0.9\n"), r"line 14.*fields"),
    (lambda t: t.replace("-0.5\t<s> b\n", "-0.5\tb\n"), r"line 19.*fields"),
    (lambda t: t.replace("\\end\\", ""), r"without \\end\\"),
    (lambda t: t.replace("\\3-grams:", "\\4-grams:"), r"line 27.*not announced"),
    (lambda t: t.replace("-0.6\ta\t-0.4", "x\ta\t-0.4"), r"line 12.*bad number"),
])
def test_malformed_arpa_files_raise(edit, what):
    from joeys2t_amd.lm import read_arpa
    text = edit(ARPA.read_text())
    assert text != ARPA.read_text()
    with pytest.raises(ValueError, match=what):
        read_arpa(text.splitlines())


# ---------------------------------------------------------------- the builder
def check_table(t, grams, lp, bo, absent):
    from joeys2t_amd.lm import fmix
    cap = t.capacity
    assert cap & (cap - 1) == 0 and t.n_entries == len(grams) < cap and int((t.table["key"] != 0).sum()) == len(grams)
    far = 0
    for g, a, b in zip(grams, lp, bo):
        got = G.table_lookup(t, tuple(g))
        assert got[:2] == (float(a), float(b)) and got[2] <= t.max_probe, g
        far = max(far, got[2])
    assert far == t.max_probe  # the largest distance of a stored key from its home, plus 1: not an over-estimate
    assert np.array_equal((fmix(np.array([G.key_of(g) for g in grams], dtype=np.uint64)) & np.uint64(cap - 1)).astype(np.int64),
                          np.array([G.fmix_py(G.key_of(g)) & (cap - 1) for g in grams]))
    full = 0
    for g in absent:
        got = G.table_lookup(t, tuple(g))
        assert got[0] is None
        full += got[2] == t.max_probe and all(int(t.table[(G.fmix_py(G.key_of(g)) + i) & (cap - 1)]["key"]) for i in range(t.max_probe))
    return full


@pytest.mark.parametrize("pin, want", [(G.BUILDER_WRAP, "wrap"), (G.BUILDER_PROBE4, "probe4")])
def test_builder_pinned_tables(pin, want):
    from joeys2t_amd.lm import NGramLM, fmix
    assert G.find_builder_seed(pin["count"], pin["max_load"], want) == pin["seed"]
    ids, lp, bo = G.builder_grams(pin["seed"], pin["count"])
    t = NGramLM.from_arrays(np.zeros((50, 2), dtype=np.float32), {3: (ids, lp, bo)}, max_load=pin["max_load"])
    assert t.capacity == 64 and t.order == 3
    have = {tuple(g) for g in ids.tolist()}
    absent = [g for g in itertools.product(range(50), repeat=3) if g not in have][::7] + [g[:2] for g in ids.tolist()]
    full = check_table(t, ids.tolist(), lp, bo, absent)
    stored = np.nonzero(t.table["key"])[0]
    home = (fmix(t.table["key"][stored]) & np.uint64(63)).astype(np.int64)
    wrapped = int((stored < home).sum())
    print(f"{want}: capacity {t.capacity}, {t.n_entries} entries, max_probe {t.max_probe}, {wrapped} wrapped, "
          f"{full} absent keys whose chain is full up to max_probe")
    if want == "wrap":
        assert wrapped >= 1 and t.n_entries > 0.95 * t.capacity and full >= 1
    else:
        assert t.max_probe >= 4


def test_builder_refuses_what_it_cannot_store():
    from joeys2t_amd.lm import NGramLM, build_table
    with pytest.raises(ValueError, match="distinct"):
        build_table(np.array([5, 5], dtype=np.uint64), [0, 0], [0, 0])
    with pytest.raises(ValueError, match="outside 0"):
        NGramLM.from_ngrams({(0, ): (0.0, 0.0), (0, 7): (0.0, 0.0)}, 7)
    with pytest.raises(ValueError, match="longer than 4"):
        NGramLM.from_ngrams({(0, 1, 2, 3, 4): (0.0, 0.0)}, 7)
    with pytest.raises(ValueError, match="V"):
        NGramLM(np.zeros((70000, 2), dtype=np.float32), np.zeros(0, dtype=[("key", "<u8"), ("logp", "<f4"), ("backoff", "<f4")]), 1, 0, 1)
    uni_only = NGramLM.from_ngrams({(w, ): (-1.0, 0.0) for w in range(5)}, 5)
    assert uni_only.order == 1 and uni_only.capacity == 0 and uni_only.n_entries == 0


@pytest.mark.parametrize("name", ["o3", "o4", "big", "big_full"])
def test_the_table_scorer_equals_the_dict_scorer(name):
    """the emulated probe rule over the built table against the dict, on the case's hypotheses and on random ones; values agree to
    the f32 rounding of the stored numbers"""
    from joeys2t_amd.lm import NGramLM
    c, lm = G.CASES[name], G.case_lm(name)
    t = NGramLM.from_ngrams(lm, c["V"], max_load=c.get("max_load", 0.5))
    grams = [g for g in lm if len(g) > 1]
    assert t.n_entries == len(grams) and t.order == c["order"] and t.n_entries <= c.get("max_load", 0.5) * t.capacity
    if name.startswith("big"):
        assert t.capacity == (16384 if name == "big_full" else 32768) and (name == "big" or t.max_probe >= 8)
    check_table(t, grams, [np.float32(lm[g][0]) for g in grams], [np.float32(lm[g][1]) for g in grams],
                [g[:-1] + ((g[-1] + 1) % c["V"], ) for g in grams[::17] if g[:-1] + ((g[-1] + 1) % c["V"], ) not in lm])
    rs = np.random.RandomState(5)
    hits = 0
    for _ in range(40):
        y = G.sample_labels(lm, c["V"], c["order"], rs, 12)
        if rs.uniform() < 0.3:
            y[rs.randint(12)] = c["V"] + 3  # an id outside the vocabulary: -inf there, the following contexts cut
        for l in range(13):
            w, hist = (y[l] if l < 12 else G.EOS), [G.BOS] + y[:l]
            a, b = G.token_logp(lm, w, hist, c["V"], c["order"]), G.table_token_logp(t, w, hist, c["V"], c["order"])
            assert (a == b == -np.inf) or abs(a - b) <= 1e-6 * max(1.0, abs(a)), (name, y, l, a, b)
            hits += any(tuple(hist[-k:]) + (w, ) in lm for k in range(1, c["order"]))
    assert hits > 40 or c["order"] == 1


def test_save_and_load_round_trip(tmp_path):
    from joeys2t_amd.lm import NGramLM
    lm = NGramLM.from_arpa(ARPA, vocab())
    lm.save(tmp_path / "lm.npz")
    back = NGramLM.load(tmp_path / "lm.npz")
    assert back.uni.dtype == lm.uni.dtype and np.array_equal(back.uni.view(np.int32), lm.uni.view(np.int32))
    assert back.table.dtype == lm.table.dtype and back.table.tobytes() == lm.table.tobytes()
    assert (back.order, back.n_entries, back.capacity, back.max_probe, back.dropped, back.dropped_tokens) == \
        (lm.order, lm.n_entries, lm.capacity, lm.max_probe, lm.dropped, lm.dropped_tokens)
    one = NGramLM.from_ngrams({(w, ): (-1.0, 0.0) for w in range(5)}, 5)
    one.save(tmp_path / "one.npz")
    assert NGramLM.load(tmp_path / "one.npz").capacity == 0


# ---------------------------------------------------------------- the inputs of the GPU tests
@pytest.mark.parametrize("name", list(G.CASES))
def test_pinned_cases_are_decidable(name):
    """a condition on the INPUTS, checked here so that the GPU test may compare orders exactly: every utterance of every pinned case
    has margin >= 4 at every (lm_weight, length_bonus) it is used with, and the seed is the first such one from the case's base"""
    margins = {wb: G.case_margin(name, *wb) for wb in G.COMBOS}
    print(f"{name}: seed {G.SEEDS[name]} margins {({wb: round(m, 1) for wb, m in margins.items()})}")
    assert min(margins.values()) >= G.DECIDABLE
    assert G.find_seed(name) == G.SEEDS[name]
    c, x = G.CASES[name], G.case_inputs(name)
    assert x["ids"].shape == (c["B"], c["N"], c["Lp"] + 1) and x["n"].dtype == np.int32 and x["base"].dtype == np.float32
    assert G.lm_order(G.case_lm(name)) == c["order"]
    for wb in G.COMBOS:
        assert all(sorted(o) == list(range(c["N"])) for o in G.case_reference(name, *wb)[3].tolist())


def test_the_planted_case_has_what_it_says():
    c, x = G.CASES["ragged"], G.case_inputs("ragged")
    dead = G.dead_slots(x["n"].reshape(-1), x["base"].reshape(-1), c["Lp"]).reshape(c["B"], c["N"])
    assert x["n"][0, 0] == c["Lp"] - 1 and x["n"][0, 1] == 0 and c["B"] == 3
    assert dead[0].tolist() == [False, False, True, True, False] and x["base"][0, 2] == -np.inf and x["n"][0, 3] == c["Lp"]
    assert dead[1].tolist() == [False, False, True, False, False] and not dead[2].any()
    order = G.case_reference("ragged", 0.3, 0.0)[3]
    assert order[0, 3:].tolist() == [2, 3] and order[1, 4] == 2


def test_the_cases_use_the_whole_vocabulary():
    """labels are drawn from every id, bos, eos and pad included, and the hypotheses meet stored n-grams of every order"""
    seen, orders = set(), set()
    for name in ("o4", "n32", "ragged"):
        c, x, lm = G.CASES[name], G.case_inputs(name), G.case_lm(name)
        for y, m in zip(x["ids"].reshape(-1, c["Lp"] + 1), x["n"].reshape(-1)):
            y = [int(v) for v in y[:max(int(m), 0)]] if m <= c["Lp"] - 1 else []
            seen |= set(y)
            hist = [G.BOS] + y + [G.EOS]
            orders |= {k for k in range(2, c["order"] + 1) for i in range(len(hist) - k + 1) if tuple(hist[i:i + k]) in lm}
    assert {G.PAD, G.BOS, G.EOS} <= seen and orders == {2, 3, 4}


# ---------------------------------------------------------------- search-level argument validation (no device)
@pytest.mark.parametrize("fn", ["ctc_beam_search", "ctc_attention_rescore"])
@pytest.mark.parametrize("kw, what", [
    (dict(lm_weight=0.5), "lm_weight 0.5 without an lm"),
    (dict(length_bonus=float("nan")), "not finite"),
    (dict(length_bonus=float("inf")), "not finite"),
])
def test_search_argument_validation(fn, kw, what):
    """refused before the model or the batch is touched"""
    from joeys2t_amd import search
    with pytest.raises(ValueError, match=what):
        getattr(search, fn)(None, None, beam_size=4, **kw)


def test_search_sizes_with_an_lm():
    from joeys2t_amd.search import ctc_beam_search
    with pytest.raises(ValueError, match="n_rescore 5"):
        ctc_beam_search(None, None, beam_size=4, n_best=1, n_rescore=5, length_bonus=0.5)
    with pytest.raises(ValueError, match="n_rescore 1"):
        ctc_beam_search(None, None, beam_size=4, n_best=2, n_rescore=1, length_bonus=0.5)
    with pytest.raises(ValueError, match="n_rescore without"):
        ctc_beam_search(None, None, beam_size=4, n_best=2, n_rescore=3)


def test_predict_refuses_an_lm_for_the_attention_decoder():
    from joeys2t_amd.prediction import predict
    with pytest.raises(ValueError, match="lm / lm_weight / length_bonus"):
        predict(None, [], lm=object(), lm_weight=0.5)
    with pytest.raises(ValueError, match="lm / lm_weight / length_bonus"):
        predict(None, [], decoder="attention", length_bonus=0.5)
