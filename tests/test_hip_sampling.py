"""js2t_sample_step against the float64 restatement of its rule (tests/sampling_reference.py), and `sample_search` / `predict` on the
three golden models.  Every test here fails without the feature: the symbol, the op and the decoder do not exist there."""
import functools

import numpy as np
import pytest
import torch

import sampling_reference as S

pytestmark = pytest.mark.gpu
WORST = {}  # case -> worst (log-prob err / bound, cdf err / TAU_MASS) seen
DEV = "cuda:0"


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return all((x is None and y is None) or torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def launch(logits, u, forbid, T=1.0, k=0, p=1.0, eps=0.0, finished=None, score=None, length=None, step=1, width=3, eos=S.EOS, pad=S.PAD,
           want=("q", "kept", "cdf"), ids=None):
    """one launch with garbage pre-filled in every output: -> (ids table, logp, q, kept, cdf, finished, score, length)"""
    from joeys2t_amd import ops
    rows = logits.shape[0]
    ids = torch.full((rows, width), -77, dtype=torch.int64, device=logits.device) if ids is None else ids
    out = (torch.full((rows, ), 7.5, device=logits.device), torch.full((rows, ), 7.5, device=logits.device) if "q" in want else None,
           torch.full((rows, ), -9, dtype=torch.int32, device=logits.device) if "kept" in want else None,
           torch.full((rows, 2), 7.5, device=logits.device) if "cdf" in want else None)
    ops.sample_step(logits, u, ids, step, forbid, eos, pad, temperature=T, top_k=k, top_p=p, epsilon=eps, finished=finished, score=score,
                    length=length, out=out)
    return (ids, *out, finished, score, length)


@functools.lru_cache(maxsize=None)
def on_device(name):
    """the pinned case's inputs on the device, uploaded once: do not modify"""
    c = S.case_inputs(name)
    return c, {k: torch.from_numpy(c[k]).to(DEV) for k in ("logits", "u", "finished", "score", "length")}


def run_case(name, **over):
    c, d = on_device(name)
    kw = dict(finished=d["finished"].clone(), score=d["score"].clone(), length=d["length"].clone())
    kw.update(over)
    return launch(d["logits"], d["u"], c["forbid"], c["T"], c["k"], c["p"], c["eps"], **kw)


@pytest.mark.parametrize("name", list(S.CASES))
def test_pinned_cases_against_the_reference(device, name):
    c, _ = on_device(name)
    ids, logp, q, kept, cdf, fin, score, length = (t.cpu().numpy() for t in run_case(name))
    ref = S.case_reference(name)
    worst_lp = worst_cdf = 0.0
    assert (ids[:, 0] == -77).all() and (ids[:, 2] == -77).all()  # only column `step` is written
    for r, want in enumerate(ref):
        if want is None:  # a finished row
            assert ids[r, 1] == S.PAD and logp[r] == 0 and q[r] == 0 and kept[r] == 0 and (cdf[r] == 0).all() and fin[r] == 1
            assert score[r].view(np.int32) == c["score"][r].view(np.int32) and length[r] == c["length"][r]
            continue
        assert ids[r, 1] == want["id"] and kept[r] == want["kept"], (name, r, ids[r, 1], want["id"], kept[r], want["kept"])
        e_lp = max(abs(logp[r] - want["logp"]) / S.bound(want["logp"]), abs(q[r] - want["q"]) / S.bound(want["q"]))
        e_cdf = max(abs(cdf[r, 0] - want["cdf"][0]), abs(cdf[r, 1] - want["cdf"][1])) / S.TAU_MASS
        worst_lp, worst_cdf = max(worst_lp, e_lp), max(worst_cdf, e_cdf)
        assert e_lp <= 1.0 and e_cdf <= 1.0, (name, r, e_lp, e_cdf)
        assert fin[r] == (1 if want["id"] == S.EOS else 0) and length[r] == c["length"][r] + (want["id"] != S.EOS)
        assert score[r].view(np.int32) == np.float32(c["score"][r] + logp[r]).view(np.int32)  # ONE f32 addition
    WORST[name] = (worst_lp, worst_cdf)
    print(f"{name}: worst log-prob err / bound {worst_lp:.4f}, worst cdf err / TAU_MASS {worst_cdf:.4f}")


@pytest.mark.parametrize("kw", [dict(), dict(k=5, p=0.9)])
def test_stratified_grid_reproduces_the_distribution(device, kw):
    """one V = 11 row R = 4096 times with u_r = (r + 0.5) / R: every token's count is within 1 + 2 R TAU_MASS of R q_v, exactly 0 for a
    dropped token - a deterministic distribution test, not a statistical one.  Forbidden ids are never returned."""
    R, forbid = 4096, [4]
    row = (2.0 * np.random.RandomState(5).randn(11)).astype(np.float32)
    logits = torch.from_numpy(row).to(DEV).repeat(R, 1)
    u = ((torch.arange(R, dtype=torch.float64) + 0.5) / R).float().to(DEV)
    ids = launch(logits, u, forbid, **kw)[0][:, 1].cpu().numpy()
    one = S.ref(row, 0.5, forbid=forbid, **kw)
    z = row.astype(np.float64)
    mass = {int(v): np.exp(z[v]) for v in one["order"]}
    W = sum(mass.values())
    worst = 0.0
    for v in range(11):
        got, want = int((ids == v).sum()), R * mass.get(v, 0.0) / W
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= 1 + 2 * R * S.TAU_MASS and (v in mass or got == 0), (v, got, want)
    assert (ids != 4).all() and (np.diff(ids) >= 0).all()
    print(f"grid {kw}: worst |count - R q| {worst:.3f} (bound {1 + 2 * R * S.TAU_MASS:.3f})")


def test_the_ends_of_the_unit_interval(device):
    c, d = on_device("v5000_p")
    rows = c["rows"]
    ref = [S.ref(c["logits"][r], 0.5, c["T"], c["k"], c["p"], c["eps"], c["forbid"]) for r in range(rows)]
    for uval, pick in ((0.0, min), (float(np.nextafter(np.float32(1), np.float32(0))), max), (float("nan"), min), (5.0, max), (-3.0, min)):
        u = torch.full((rows, ), uval, device=DEV)
        ids = launch(d["logits"], u, c["forbid"], c["T"], c["k"], c["p"], c["eps"])[0][:, 1].cpu().numpy()
        assert ids.tolist() == [pick(r["order"].tolist()) for r in ref], uval


@pytest.mark.parametrize("kw", [dict(k=1), dict(k=1, T=1e-3)])
def test_top1_is_the_greedy_step(device, kw):
    from joeys2t_amd import ops
    c, d = on_device("v5000")
    rows = c["rows"]
    scores, gids, _ = ops.beam_step(d["logits"], torch.zeros(rows, device=DEV), rows, 1, c["forbid"], 0.0)
    ids, logp, q, kept, *_ = launch(d["logits"], d["u"], c["forbid"], **kw)
    assert torch.equal(ids[:, 1], gids[:, 0])
    err = (logp - scores[:, 0]).abs().cpu().numpy()
    assert all(e <= S.bound(s) for e, s in zip(err, scores[:, 0].cpu().numpy()))
    if "k" in kw:
        assert (kept == 1).all() and (q == 0).all()


def test_forbidden_ids_and_the_empty_set(device):
    V, rows = 11, 8
    logits = torch.from_numpy((2.0 * np.random.RandomState(3).randn(rows, V)).astype(np.float32)).to(DEV)
    u = torch.rand(rows, device=DEV)
    only = 6
    ids, logp, q, kept, cdf, *_ = launch(logits, u, [v for v in range(V) if v != only])
    assert (ids[:, 1] == only).all() and (kept == 1).all() and (q == 0).all() and (cdf[:, 0] == 0).all() and (cdf[:, 1] == 1).all()
    lse = torch.logsumexp(logits.double(), 1)
    assert ((logp.double() - (logits[:, only].double() - lse)).abs() <= 1e-4 * (logits[:, only].double() - lse).abs().clamp(min=1)).all()
    fin, score, length = torch.zeros(rows, dtype=torch.uint8, device=DEV), torch.zeros(rows, device=DEV), torch.full((rows, ), 3, dtype=torch.int32, device=DEV)
    ids, logp, q, kept, cdf, fin, score, length = launch(logits, u, list(range(V)), finished=fin, score=score, length=length)
    assert (ids[:, 1] == S.EOS).all() and torch.isneginf(logp).all() and (q == 0).all() and (kept == 0).all() and (cdf == 0).all()
    assert (fin == 1).all() and torch.isneginf(score).all() and (length == 3).all()
    dead = torch.full_like(logits, float("-inf"))
    dead[0, 2] = float("nan")
    ids, logp, *_ = launch(dead, u, [])
    assert (ids[:, 1] == S.EOS).all() and torch.isneginf(logp).all()


def test_rows_are_independent_and_poison_is_not_read(device):
    """every row alone equals itself in the batch, bit for bit; finished rows carry NaN logits and NaN u (the case's), every output is
    pre-filled with garbage"""
    for name in ("tiny_all", "v5003_all"):
        c, d = on_device(name)
        whole = run_case(name)
        for r in (0, 1, 3, 5, 7, 10, c["rows"] - 1):
            one = launch(d["logits"][r:r + 1], d["u"][r:r + 1], c["forbid"], c["T"], c["k"], c["p"], c["eps"], finished=d["finished"][r:r + 1].clone(),
                         score=d["score"][r:r + 1].clone(), length=d["length"][r:r + 1].clone())
            assert same_bits(one, [t[r:r + 1] for t in whole]), (name, r)


def test_a_view_equals_its_contiguous_copy(device):
    """rows at an odd element offset, V = 5003 (no multiple of four), a row distance that is no multiple of four"""
    c, d = on_device("v5003_all")
    rows, V = c["rows"], c["V"]
    buf = torch.full((rows * (V + 6) + 8, ), float("nan"), device=DEV)
    view = buf[2:2 + rows * (V + 6)].view(rows, V + 6)[:, 1:1 + V]  # element offset 3, rows 5009 apart
    view.copy_(d["logits"])
    assert view.data_ptr() % 16 != 0 and view.stride(0) == V + 6
    got = launch(view, d["u"], c["forbid"], c["T"], c["k"], c["p"], c["eps"], finished=d["finished"].clone(), score=d["score"].clone(),
                 length=d["length"].clone())
    assert same_bits(got, run_case("v5003_all"))
    # and the ids table as a strided view
    table = torch.full((rows, 9), -77, dtype=torch.int64, device=DEV)
    got = launch(d["logits"], d["u"], c["forbid"], c["T"], c["k"], c["p"], c["eps"], finished=d["finished"].clone(), score=d["score"].clone(),
                 length=d["length"].clone(), ids=table[:, 2:5])
    assert torch.equal(got[0][:, 1], run_case("v5003_all")[0][:, 1]) and (table[:, [0, 1, 2, 4, 5, 6, 7, 8]] == -77).all()


def test_optional_outputs_may_be_absent(device):
    name = "tiny_all"
    full = run_case(name)
    for drop in ("q", "kept", "cdf"):
        got = run_case(name, want=tuple(w for w in ("q", "kept", "cdf") if w != drop))
        k = {"q": 2, "kept": 3, "cdf": 4}[drop]
        assert got[k] is None and same_bits([t for i, t in enumerate(got) if i != k], [t for i, t in enumerate(full) if i != k])
    for drop, k in (("finished", 5), ("score", 6), ("length", 7)):
        c, d = on_device("tiny")  # (no finished rows: without the flags every row is live)
        base = run_case("tiny")
        got = run_case("tiny", **{drop: None})
        assert got[k] is None and same_bits([t for i, t in enumerate(got) if i != k], [t for i, t in enumerate(base) if i != k])


def test_a_captured_launch_replays_the_same_bits(device):
    from joeys2t_amd import ops
    name = "v5003_all"
    c, d = on_device(name)
    clean = run_case(name)
    rows = c["rows"]
    ids = torch.full((rows, 3), -77, dtype=torch.int64, device=DEV)
    out = (torch.empty(rows, device=DEV), torch.empty(rows, device=DEV), torch.empty(rows, dtype=torch.int32, device=DEV), torch.empty((rows, 2), device=DEV))
    fin, score, length = d["finished"].clone(), d["score"].clone(), d["length"].clone()

    def call():
        ops.sample_step(d["logits"], d["u"], ids, 1, c["forbid"], S.EOS, S.PAD, temperature=c["T"], top_k=c["k"], top_p=c["p"], epsilon=c["eps"],
                        finished=fin, score=score, length=length, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # first launch outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for fill in (7, 11):
        ids.fill_(-77)
        for o in out:
            o.fill_(fill)
        fin.copy_(d["finished"]), score.copy_(d["score"]), length.copy_(d["length"])
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits((ids, *out, fin, score, length), clean)


def test_the_op_refuses_what_the_library_refuses(device):
    from joeys2t_amd import ops
    logits, u = torch.zeros((2, 11), device=DEV), torch.zeros(2, device=DEV)
    ids = torch.zeros((2, 3), dtype=torch.int64, device=DEV)
    ok = dict(temperature=1.0, top_k=0, top_p=1.0, epsilon=0.0)
    for kw in (dict(temperature=0.0), dict(temperature=float("inf")), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(epsilon=1.0), dict(epsilon=-0.5)):
        with pytest.raises(ops.Js2tError):
            ops.sample_step(logits, u, ids, 0, [], S.EOS, S.PAD, **dict(ok, **kw))
    for bad in (lambda: ops.sample_step(logits, u, ids, 3, [], S.EOS, S.PAD), lambda: ops.sample_step(logits, u, ids, 0, [], 11, S.PAD),
                lambda: ops.sample_step(logits, u, ids, 0, list(range(17)), S.EOS, S.PAD), lambda: ops.sample_step(logits.double(), u, ids, 0, [], S.EOS, S.PAD),
                lambda: ops.sample_step(logits, u, ids.int(), 0, [], S.EOS, S.PAD), lambda: ops.sample_step(logits, u[:1], ids, 0, [], S.EOS, S.PAD),
                lambda: ops.sample_step(logits[:, :1], u, ids, 0, [], 0, 0), lambda: ops.sample_step(logits.cpu(), u, ids, 0, [], S.EOS, S.PAD),
                lambda: ops.sample_step(logits, u, ids, 0, [], S.EOS, S.PAD, finished=torch.zeros(2, dtype=torch.bool, device=DEV))):
        with pytest.raises(ops.Js2tError):
            bad()
    assert (ids == 0).all()  # nothing ran


def test_kernel_summary(device):
    """the worst measured error / tolerance per case (runs the cases if run alone)"""
    for name in S.CASES:
        if name not in WORST:
            test_pinned_cases_against_the_reference(device, name)
    print("worst (log-prob err / bound, cdf err / TAU_MASS):", {k: (round(a, 4), round(b, 4)) for k, (a, b) in WORST.items()})
    assert len(WORST) == len(S.CASES) and all(a <= 1 and b <= 1 for a, b in WORST.values())


# ---------------------------------------------------------------- model level
MODELS = ["model_pre", "model_post", "model_deepnet"]
MAX_LEN = 12
DISTINCT = {}  # model -> utterances with two different samples
EOS_ROWS = {}  # model -> (rows that drew EOS, rows)


@functools.lru_cache(maxsize=None)
def golden(name):
    """(model, golden arrays), built once per process: do not modify"""
    from test_hip_model import build
    model, g = build(name, torch.device(DEV))
    model.eval()
    return model, g


def draw(name, **kw):
    from joeys2t_amd.search import sample_search
    from test_hip_model import batch_kwargs
    model, g = golden(name)
    return sample_search(model, batch_kwargs(g, torch.device(DEV)), max_output_length=MAX_LEN, **kw)


@functools.lru_cache(maxsize=None)
def eight(name):
    """eight samples per utterance at temperature 1, seed 0, with parts: shared by the tests, do not modify"""
    return draw(name, n_samples=8, return_parts=True)


@pytest.mark.parametrize("name", MODELS)
def test_one_sample_with_top1_is_greedy(device, name):
    from joeys2t_amd.search import search
    from test_hip_model import batch_kwargs
    model, g = golden(name)
    gids, gscores, _ = search(model, batch_kwargs(g, device), max_output_length=MAX_LEN, beam_size=1, beam_alpha=-1.0, return_prob="hyp")
    ids, scores, lengths = draw(name, n_samples=1, top_k=1)
    eos = model.eos_index
    for b in range(gids.shape[0]):
        row = gids[b].tolist()
        n = row.index(eos) if eos in row else len(row)
        assert lengths[b] == n and ids[b, :n].tolist() == row[:n], (name, b)  # ids up to EOS; the sampler does not store it
        total = float(gscores[b, :n + (eos in row)].sum())
        assert abs(float(scores[b, 0]) - total) <= S.bound(total)


@pytest.mark.parametrize("name", MODELS)
def test_samples_carry_the_models_log_probability(device, name):
    """every sample that drew EOS: its score is the CPU oracle's teacher-forced log-probability of that sample, EOS included, within
    the per-row bound of test_hip_rescore.oracle_attention (which scores labels + EOS: a row that reached the length limit without EOS
    has no such term and is checked for its length only).  Checks the N-rows-per-utterance cache path and that the log-probability
    belongs to the token returned."""
    from test_hip_rescore import oracle_attention
    model, g = golden(name)
    ids, scores, lengths, parts = eight(name)
    B = g["src"].shape[0]
    assert ids.dtype == np.int64 and scores.dtype == np.float32 and lengths.dtype == np.int64
    assert ids.shape == (B * 8, max(int(lengths.max()), 1)) and scores.shape == (B * 8, 1) and parts["slot"].tolist() == list(range(8)) * B
    assert all((ids[r, lengths[r]:] == model.pad_index).all() and (ids[r, :lengths[r]] != model.eos_index).all() for r in range(B * 8))
    assert (lengths <= MAX_LEN).all()
    # the distribution drawn from is the model's renormalised over the ids that are not forbidden: never less likely than the model's
    assert all(q >= p - S.bound(p) and np.isfinite(q) for q, p in zip(parts["sampling_log_prob"].tolist(), scores[:, 0].tolist()))
    ref = oracle_attention(name, g, ids, lengths)
    ended = 0
    for r, (want, hb) in enumerate(ref):
        if lengths[r] == MAX_LEN:
            continue  # twelve labels fill the table: the row reached the limit without EOS (a shorter row always drew it)
        ended += 1
        print(f"{name} row {r}: n {lengths[r]} score {scores[r, 0]:.6f} oracle {want:.6f} err / bound {abs(float(scores[r, 0]) - want) / hb:.4f}")
        assert abs(float(scores[r, 0]) - want) <= hb, (name, r, scores[r, 0], want, hb)
    EOS_ROWS[name] = (ended, B * 8)
    groups = [set(tuple(ids[r, :lengths[r]].tolist()) for r in range(b * 8, b * 8 + 8)) for b in range(B)]
    DISTINCT[name] = sum(len(s) > 1 for s in groups)
    print(f"{name}: {ended} of {B * 8} rows match the oracle with EOS, {DISTINCT[name]} of {B} utterances have two different samples")
    assert ended >= 1


def test_model_level_counts(device):
    for name in MODELS:
        if name not in DISTINCT:
            test_samples_carry_the_models_log_probability(device, name)
    print("utterances with different samples:", DISTINCT, "rows checked with EOS:", EOS_ROWS)
    assert sum(DISTINCT.values()) >= 1 and sum(e for e, _ in EOS_ROWS.values()) >= 1


def test_seeds(device):
    name = MODELS[0]
    a, b, c = draw(name, n_samples=4, seed=11), draw(name, n_samples=4, seed=11), draw(name, n_samples=4, seed=12)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    assert a[0].shape != c[0].shape or not np.array_equal(a[0], c[0])


@pytest.mark.parametrize("name", MODELS)
def test_lengths_and_minimum_length(device, name):
    model, g = golden(name)
    ids, scores, lengths = draw(name, n_samples=5, min_output_length=3, seed=4)
    assert (lengths >= 3).all() and (lengths <= MAX_LEN).all() and np.isfinite(scores).all()
    assert all((ids[r, lengths[r]:] == model.pad_index).all() for r in range(len(lengths)))


@pytest.mark.parametrize("name", MODELS)
def test_sampled_mbr(device, name):
    import mbr_reference as M
    model, g = golden(name)
    ids, scores, lengths, parts = eight(name)
    mids, mscores, mlen, mparts = draw(name, n_samples=8, decision="mbr", n_best=3, return_parts=True)
    B = g["src"].shape[0]
    assert mids.shape[0] == B * 3 and mparts["slot"].shape == (B * 3, )
    T = ids.shape[1]
    _, _, risk, order = M.mbr(ids.reshape(B, 8, T), lengths.reshape(B, 8).astype(np.int32), np.zeros((B, 8), np.float32), 8, T + 1, 1.0)
    risk = np.asarray(risk, dtype=np.float64).reshape(B, 8)
    for b in range(B):
        slots = mparts["slot"][b * 3:b * 3 + 3].tolist()
        assert len(set(slots)) == 3
        for i, s in enumerate(slots):
            r, src = b * 3 + i, b * 8 + s
            assert mscores[r, 0].view(np.int32) == scores[src, 0].view(np.int32) and mlen[r] == lengths[src]
            assert mids[r, :mlen[r]].tolist() == ids[src, :lengths[src]].tolist()
            assert abs(float(mparts["risk"][r]) - risk[b, s]) <= M.bound(risk[b, s])
        for i, (s, t) in enumerate(zip(slots, slots[1:])):
            gap, tol = risk[b, t] - risk[b, s], max(M.bound(risk[b, s]), M.bound(risk[b, t]))
            assert gap > 0 if abs(gap) >= 4 * tol else gap >= -2 * tol, (name, b, slots)
            if mparts["risk"][b * 3 + i].view(np.int32) == mparts["risk"][b * 3 + i + 1].view(np.int32):
                assert s < t  # ties in draw order
        rest = [s for s in range(8) if s not in slots]
        assert all(risk[b, s] >= risk[b, slots[-1]] - 2 * max(M.bound(risk[b, s]), M.bound(risk[b, slots[-1]])) for s in rest)


def test_predict_with_the_sample_decoder(device):
    """predict sorts a batch by source length, draws, and puts the rows back: the rows are sample_search's on the sorted batch, in
    the original order; one generator runs through the batches, so the second of two equal batches draws something else"""
    from joeys2t_amd.helpers import expand_reverse_index
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import sample_search
    from test_hip_model import batch_kwargs
    name = MODELS[0]
    model, g = golden(name)
    B = g["src"].shape[0]
    kw = dict(decoder="sample", n_samples=8, max_output_length=MAX_LEN, return_prob="hyp")
    for decision, nb in (("none", 8), ("mbr", 3)):
        batch = batch_kwargs(g, device)
        back = expand_reverse_index(batch.sort_by_src_length(), nb)
        ids, scores, lengths = sample_search(model, batch, n_samples=8, max_output_length=MAX_LEN, decision=decision, n_best=nb)
        out_ids, _, out_scores = predict(model, [batch_kwargs(g, device)], n_best=nb, decision="mbr" if decision == "mbr" else "map", **kw)
        assert len(out_ids) == B * nb == len(out_scores)
        for r, src in enumerate(back):
            assert out_ids[r][:lengths[src]].tolist() == ids[src, :lengths[src]].tolist()
            assert np.asarray(out_scores[r]).view(np.int32)[0] == scores[src, 0].view(np.int32)
    two_ids, _, two_scores = predict(model, [batch_kwargs(g, device), batch_kwargs(g, device)], n_best=8, **kw)
    assert len(two_ids) == 2 * B * 8
    first, second = np.asarray([s[0] for s in two_scores[:B * 8]]), np.asarray([s[0] for s in two_scores[B * 8:]])
    again = np.asarray([s[0] for s in predict(model, [batch_kwargs(g, device)], n_best=8, **kw)[2]])
    assert np.array_equal(first.view(np.int32), again.view(np.int32)) and not np.array_equal(first, second)
