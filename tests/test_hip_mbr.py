"""GPU: js2t_edit_distance and js2t_mbr_rescore against the reference of tests/mbr_reference.py - distances and orders exactly on
inputs that test_mbr_cpu.py shows to be decidable, posterior and risk within the project's tolerance (ctc_beam_reference.bound) -
their exactness, poison, batching, replay and tie properties, their composition with the beam kernel's list, metrics.token_errors,
and decision="mbr" of the two CTC decoders and of predict on the golden models against the same lists ranked on the host."""
import functools

import numpy as np
import pytest
import torch

import mbr_reference as M

pytestmark = pytest.mark.gpu

WORST = {}  # (what, scale) -> worst err / tolerance seen
HI = 2**40 + 5


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def on_device(name, device=None):
    device = device or torch.device("cuda:0")
    x = M.case_inputs(name)
    return tuple(torch.from_numpy(x[k]).to(device) for k in ("ids", "n", "score"))


def run(ids, n, score, N, scale, **kw):
    from joeys2t_amd import ops
    out = ops.mbr_rescore(ids, n, score, N, scale, **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def clean(name, scale):
    """the pinned case run once on the GPU and shared by the tests that compare against it: do not modify"""
    return run(*on_device(name), M.CASES[name]["N"], scale)


def garbage_outputs(like):
    return tuple(torch.full_like(t, 77) if t.dtype == torch.int32 else torch.full_like(t, float("nan")) for t in like)


def check_values(out, ref, dead, what, scale, exact_order=True):
    """the four outputs against the reference's: dist exact, posterior and risk in tolerance, dead slots as stated, the order exact
    (or, without exact_order, consistent with the reference's risks within two tolerances)"""
    dist, post, risk, order = (o.cpu().numpy() for o in out)
    rdist, rpost, rrisk, rorder = ref
    B, N = rorder.shape
    assert dist.shape == (B, N, N) and post.shape == risk.shape == (B * N, ) and order.shape == (B, N)
    assert dist.dtype == np.int32 and post.dtype == risk.dtype == np.float32 and order.dtype == np.int32
    assert np.array_equal(dist, rdist), (what, scale)
    assert np.array_equal(dist, dist.transpose(0, 2, 1))
    worst = 0.0
    for r in range(B * N):
        b, k = divmod(r, N)
        if dead[r]:
            assert post[r] == 0.0 and risk[r] == np.inf and (dist[b, k] == -1).all() and (dist[b, :, k] == -1).all(), (what, r)
            continue
        assert dist[b, k, k] == 0
        errs = [abs(float(post[r]) - rpost[r]) / M.bound(rpost[r]), abs(float(risk[r]) - rrisk[r]) / M.bound(rrisk[r])]
        worst = max(worst, max(errs))
        assert max(errs) <= 1.0, (what, scale, r, errs)
    print(f"{what} scale {scale}: worst err / tolerance {worst:.4f}")
    WORST[(what, scale)] = max(WORST.get((what, scale), 0.0), worst)
    for b in range(B):
        assert sorted(order[b].tolist()) == list(range(N))
        nd = int(dead[b * N:(b + 1) * N].sum())
        assert order[b, N - nd:].tolist() == [k for k in range(N) if dead[b * N + k]]  # dead slots last, in slot order
        if not exact_order:
            rr = rrisk[b * N:(b + 1) * N]
            for first, second in zip(order[b, :N - nd - 1], order[b, 1:N - nd]):
                assert rr[first] <= rr[second] + 2 * M.bound(rr[second]), (what, b, first, second)
    if exact_order:
        assert np.array_equal(order, rorder), (what, scale, order, rorder)


def case_dead(name):
    x = M.case_inputs(name)
    return M.dead_slots(x["n"].reshape(-1), x["score"].reshape(-1), M.CASES[name]["T"] + 1)


# ---------------------------------------------------------------- the pinned cases against the reference
@pytest.mark.parametrize("scale", M.SCALES)
@pytest.mark.parametrize("name", list(M.CASES))
def test_pinned_case_matches_reference(device, name, scale):
    check_values(clean(name, scale), M.case_reference(name, scale), case_dead(name), name, scale)


# ---------------------------------------------------------------- js2t_edit_distance
@functools.lru_cache(maxsize=None)
def length_pairs():
    """all 64 ordered pairs of the edge lengths: (a [64, 131], a_len, b [64, 131], b_len, the reference's distances), rows that are
    variants of one base row in the even pairs and unrelated in the odd ones: do not modify"""
    rs = np.random.RandomState(7)
    base = rs.randint(1, M.V, size=129).tolist()
    W = 131
    a, b = rs.randint(1, M.V, size=(64, W)).astype(np.int64), rs.randint(1, M.V, size=(64, W)).astype(np.int64)
    a_len, b_len, want = np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(64, np.int64)
    for p, (la, lb) in enumerate((x, y) for x in M.EDGE_LENGTHS for y in M.EDGE_LENGTHS):
        a_len[p], b_len[p] = la, lb
        if p % 2 == 0:
            a[p, :la] = M.variant(rs, base[:la], 2, la)
            b[p, :lb] = M.variant(rs, base[:lb], 3, lb)
        want[p] = M.edit_distance(a[p, :la], b[p, :lb])
    return a, a_len, b, b_len, want


def test_edit_distance_at_every_pair_of_edge_lengths(device):
    from joeys2t_amd import ops
    a, a_len, b, b_len, want = length_pairs()
    ta, tal, tb, tbl = (torch.from_numpy(x).to(device) for x in (a, a_len, b, b_len))
    d = ops.edit_distance(ta, tal, tb, tbl)
    assert d.dtype == torch.int32 and d.shape == (64, )
    assert d.cpu().numpy().tolist() == want.tolist()
    assert ops.edit_distance(tb, tbl, ta, tal).cpu().numpy().tolist() == want.tolist()  # symmetric
    assert not ops.edit_distance(ta, tal, ta, tal).any()  # a against itself
    # a strided view at an odd base offset: the same rows inside a wider table
    wide = torch.full((64, 2 * 131 + 3), HI, dtype=torch.int64, device=device)
    wide[:, 3:3 + 131] = ta
    view = wide[:, 3:3 + 131]
    assert view.data_ptr() % 16 == 8 and not view.is_contiguous()
    out = torch.full((64, ), 77, dtype=torch.int32, device=device)
    assert ops.edit_distance(view, tal, tb, tbl, out=out) is out and out.cpu().numpy().tolist() == want.tolist()
    odd = torch.full((64 * 131 + 1, ), HI, dtype=torch.int64, device=device)
    odd[1:] = tb.reshape(-1)
    assert ops.edit_distance(ta, tal, odd[1:].view(64, 131), tbl).cpu().numpy().tolist() == want.tolist()


def test_edit_distance_groups_negative_lengths_and_poison(device):
    from joeys2t_amd import ops
    a, a_len, b, b_len, want = length_pairs()
    R, g = 20, 3  # rows of a against row r // 3 of b; the last group is short
    rb = [r // g for r in range(R)]
    want_g = [M.edit_distance(a[r, :a_len[r]], b[rb[r], :b_len[rb[r]]]) for r in range(R)]
    ta, tal = torch.from_numpy(a[:R]).to(device), torch.from_numpy(a_len[:R]).to(device)
    tb, tbl = torch.from_numpy(b[:7]).to(device), torch.from_numpy(b_len[:7]).to(device)
    assert ops.edit_distance(ta, tal, tb, tbl, group=g).cpu().numpy().tolist() == want_g
    # poison behind every length; a negative length on either side gives exactly -1
    ta, tb, tal, tbl = ta.clone(), tb.clone(), tal.clone(), tbl.clone()
    ta[torch.arange(131, device=device)[None, :] >= tal[:, None]] = HI
    tb[torch.arange(131, device=device)[None, :] >= tbl[:, None]] = HI
    tal[4], tbl[3] = -1, -5
    ta[4], tb[3] = HI, HI
    got = ops.edit_distance(ta, tal, tb, tbl, group=g).cpu().numpy().tolist()
    assert got == [-1 if r == 4 or rb[r] == 3 else want_g[r] for r in range(R)]
    with pytest.raises(ops.Js2tError, match="group 0"):
        ops.edit_distance(ta, tal, tb, tbl, group=0)
    with pytest.raises(ops.Js2tError, match="a_max"):
        ops.edit_distance(torch.zeros((1, M.EDIT_MAX_LEN + 1), dtype=torch.int64, device=device), tal[:1], tb[:1], tbl[:1])
    assert ops.edit_distance(ta[:0], tal[:0], tb[:0], tbl[:0]).shape == (0, )


def test_token_errors_equals_the_host_sum(device):
    from joeys2t_amd.metrics import edit_distance, token_errors
    a, a_len, b, b_len, _ = length_pairs()
    dev = [torch.from_numpy(x).to(device) for x in (a, a_len, b, b_len)]
    total = sum(edit_distance(a[r, :a_len[r]].tolist(), b[r, :b_len[r]].tolist()) for r in range(64))
    assert token_errors(*dev) == (total, int(b_len.sum()))
    g = 4
    per = [edit_distance(a[r, :a_len[r]].tolist(), b[r // g, :b_len[r // g]].tolist()) for r in range(64)]
    err, n_ref, d = token_errors(dev[0], dev[1], dev[2][:16], dev[3][:16], group=g, return_dist=True)
    assert (err, n_ref, d.tolist()) == (sum(per), g * int(b_len[:16].sum()), per)


# ---------------------------------------------------------------- exact without a tolerance
def test_a_one_hot_posterior_is_exact(device):
    """scale 1e4: every exp but the top's underflows to 0, so the posterior is exactly one-hot, risk[i] is (float)dist[i][top] bit
    for bit and the first of the order is the MAP slot (or a lower slot that holds the same labelling: equal risks keep slot order)"""
    name, N = "n5", 5
    ids, n, score = on_device(name)
    dist, post, risk, order = (o.cpu().numpy() for o in run(ids, n, score, N, 1e4))
    x = M.case_inputs(name)
    for b in range(M.CASES[name]["B"]):
        top = int(np.argmax(x["score"][b]))
        assert np.sort(x["score"][b])[-1] - np.sort(x["score"][b])[-2] > 0.02  # (the input: exp(-200) is 0 in f32)
        assert post[b * N:(b + 1) * N].tolist() == [1.0 if k == top else 0.0 for k in range(N)]
        assert np.array_equal(risk[b * N:(b + 1) * N].view(np.int32), dist[b, :, top].astype(np.float32).view(np.int32))
        same = [k for k in range(N) if dist[b, k, top] == 0]
        assert order[b, 0] == same[0] and top in same and dist[b, top, top] == 0
    assert order[0, 0] == int(np.argmax(x["score"][0]))  # (utterance 0 has no second copy of its top)


def test_equal_scores_give_the_mean_distance(device):
    name, N = "ragged", 5
    ids, n, score = on_device(name)
    score = torch.where(torch.isfinite(score), torch.full_like(score, -7.5), score)
    dist, post, risk, order = (o.cpu().numpy() for o in run(ids, n, score, N, 1.0))
    dead = case_dead(name)
    worst = 0.0
    for r in range(len(dead)):
        b, k = divmod(r, N)
        live = [j for j in range(N) if not dead[b * N + j]]
        if not dead[r]:
            mean = float(np.mean([dist[b, k, j] for j in live]))
            worst = max(worst, abs(float(risk[r]) - mean) / M.bound(mean))
            assert abs(float(post[r]) - 1.0 / len(live)) <= M.bound(1.0 / len(live))
    print(f"equal scores: worst err / tolerance {worst:.4f}")
    assert worst <= 1.0


# ---------------------------------------------------------------- poison, batching, replay, ties
@pytest.mark.parametrize("name", ["ragged", "edges", "n32"])
def test_poison_behind_the_lengths_and_in_dead_slots(device, name):
    """ids of 2^40 + 5 behind every n and throughout dead slots, the outputs pre-filled with NaN / 77: the bits of the clean run,
    which a second clean launch repeats"""
    N, T = M.CASES[name]["N"], M.CASES[name]["T"]
    ids, n, score = on_device(name)
    assert same_bits(run(ids, n, score, N, 0.3), clean(name, 0.3))
    ids = ids.clone()
    dead = torch.from_numpy(case_dead(name)).to(device).view(n.shape)
    ids[(torch.arange(T, device=device)[None, None, :] >= n[:, :, None]) | dead[:, :, None]] = HI
    out = garbage_outputs(clean(name, 0.3))
    got = run(ids, n, score, N, 0.3, out=out)
    assert all(g is o for g, o in zip(got, out)) and same_bits(out, clean(name, 0.3))


@pytest.mark.parametrize("name", ["ragged", "edges"])
def test_an_utterance_alone_and_in_a_batch(device, name):
    N = M.CASES[name]["N"]
    ids, n, score = on_device(name)
    for b in range(M.CASES[name]["B"]):
        alone = run(ids[b:b + 1].contiguous(), n[b:b + 1].contiguous(), score[b:b + 1].contiguous(), N, 0.3)
        dist, post, risk, order = clean(name, 0.3)
        assert same_bits(alone, (dist[b:b + 1], post[b * N:(b + 1) * N], risk[b * N:(b + 1) * N], order[b:b + 1])), (name, b)


def test_captured_launch_replays_the_same_bits(device):
    """the entry point allocates nothing and does not synchronise: captured in a graph and replayed twice, the outputs re-filled in
    between, it gives the clean bits"""
    from joeys2t_amd import ops
    name = "edges"
    N = M.CASES[name]["N"]
    ids, n, score = on_device(name)
    out = garbage_outputs(clean(name, 0.3))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.mbr_rescore(ids, n, score, N, 0.3, out=out)  # first launch outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.mbr_rescore(ids, n, score, N, 0.3, out=out)
    for fill in (7, 11):
        for o in out:
            o.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, clean(name, 0.3))


def test_identical_hypotheses_keep_slot_order(device):
    """two identical hypotheses with identical scores: distance 0 between them, the same risk bits, slot order kept"""
    name, N = "n5", 5
    ids, n, score = on_device(name)
    ids, n, score = ids.clone(), n.clone(), score.clone()
    ids[:, 3], n[:, 3], score[:, 3] = ids[:, 1], n[:, 1], score[:, 1]
    dist, post, risk, order = (o.cpu().numpy() for o in run(ids, n, score, N, 1.0))
    for b in range(M.CASES[name]["B"]):
        assert dist[b, 1, 3] == 0 and dist[b, 3, 1] == 0
        assert risk[b * N + 1].view(np.int32) == risk[b * N + 3].view(np.int32) and post[b * N + 1].view(np.int32) == post[b * N + 3].view(np.int32)
        o = order[b].tolist()
        assert o.index(3) == o.index(1) + 1


def test_argument_errors(device):
    from joeys2t_amd import ops
    ids, n, score = on_device("n5")
    for kw, what in ((dict(N=0), "N 0"), (dict(N=33), "multiple of N|N 33"), (dict(scale=0.0), "scale"), (dict(scale=float("nan")), "scale"),
                     (dict(Lp=0), "Lp 0"), (dict(Lp=10), "ids_stride 8"), (dict(Lp=M.EDIT_MAX_LEN + 2), "Lp - 1")):
        with pytest.raises(ops.Js2tError, match=what):
            ops.mbr_rescore(ids, n, score, **dict(dict(N=5, scale=1.0), **kw))
    with pytest.raises(ops.Js2tError, match="out ="):
        ops.mbr_rescore(ids, n, score, 5, out=tuple(o[:1] for o in clean("n5", 1.0)))
    with pytest.raises(ops.Js2tError, match="CPU tensor"):
        ops.mbr_rescore(ids.cpu(), n, score, 5)
    empty = ops.mbr_rescore(ids[:0], n[:0], score[:0], 5)
    assert [tuple(t.shape) for t in empty] == [(0, 5, 5), (0, ), (0, ), (0, 5)]


# ---------------------------------------------------------------- composition with the beam kernel's list
def test_the_beam_kernels_list_goes_straight_in(device):
    """ops.ctc_beam_search's [B, N, T] table as it is (ids_stride = T, Lp = T + 1) on the pinned `short` input of ctc_beam_reference:
    what the reference gives that list"""
    import ctc_beam_reference as CB
    from joeys2t_amd import ops
    c = CB.CASES["short"]
    lg = torch.as_tensor(CB.case_logits("short")).to(device).contiguous()
    B, T, V = lg.shape
    lse, _ = ops.row_lse(lg.view(-1, V))
    cand_id, cand_lp, _ = ops.ctc_beam_candidates(lg.view(-1, V), c["C"], CB.BLANK)
    ids, n, score = ops.ctc_beam_search(lg, lse, cand_id, cand_lp, torch.as_tensor(c["in_len"]).to(device), c["K"], c["n_best"], CB.BLANK, 1)
    N = c["n_best"]
    for scale in M.SCALES:
        out = run(ids, n, score, N, scale)
        hn, hs = n.cpu().numpy().reshape(-1), score.cpu().numpy().reshape(-1)
        ref = M.mbr(ids.cpu().numpy(), hn, hs, N, T + 1, scale)
        check_values(out, ref, M.dead_slots(hn, hs, T + 1), "beam list", scale, exact_order=False)
    assert int(n.max()) > 1


def test_worst_error_over_the_kernel_cases(device):
    for name in M.CASES:
        for scale in M.SCALES:
            if (name, scale) not in WORST:
                check_values(clean(name, scale), M.case_reference(name, scale), case_dead(name), name, scale)
    worst = max(WORST.values())
    print(f"worst err / tolerance over {len(WORST)} comparisons: {worst:.4f} at {max(WORST, key=WORST.get)}")
    assert worst <= 1.0


# ---------------------------------------------------------------- model level
MODELS = ["model_pre", "model_post", "model_deepnet"]
SET = dict(beam_size=6, n_best=4, n_rescore=4)
LMW, CTCW = 0.5, 0.3
ROUTES = ["ctc", "att", "att_lm"]
TOPS = {}  # (model, route) -> (utterances whose top changed, utterances)


@functools.lru_cache(maxsize=None)
def golden(name):
    from test_hip_model import build
    model, g = build(name, torch.device("cuda:0"))
    model.eval()
    return model, g


@functools.lru_cache(maxsize=None)
def decodes(name, route):
    """(the decision="mbr" call with its parts, the same call with decision="map"), once per process: do not modify"""
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    from test_hip_model import batch_kwargs
    from test_hip_ngram import model_lm
    model, g = golden(name)
    dev = torch.device("cuda:0")
    if route == "ctc":
        return (ctc_beam_search(model, batch_kwargs(g, dev), decision="mbr", return_parts=True, **SET),
                ctc_beam_search(model, batch_kwargs(g, dev), beam_size=SET["beam_size"], n_best=SET["n_best"], decision="map"))
    kw = dict(SET, ctc_weight=CTCW, **(dict(lm=model_lm(), lm_weight=LMW) if route == "att_lm" else {}))
    return (ctc_attention_rescore(model, batch_kwargs(g, dev), decision="mbr", return_parts=True, **kw),
            ctc_attention_rescore(model, batch_kwargs(g, dev), decision="map", **kw))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", MODELS)
def test_mbr_decision_on_a_golden_model(device, name, route):
    """decision="mbr" against the decision="map" list ranked on the host by the reference: no utterance is left out"""
    model, g = golden(name)
    (ids, scores, n, parts), (mids, mscores, mn) = decodes(name, route)
    nb = SET["n_best"]
    B = g["src"].shape[0]
    assert ids.shape == mids.shape and scores.shape == (B * nb, 1) and n.shape == (B * nb, )
    assert parts["risk"].shape == parts["posterior"].shape == parts["map_rank"].shape == (B * nb, )
    assert parts["risk"].dtype == parts["posterior"].dtype == np.float32 and parts["map_rank"].dtype == np.int64
    L = mids.shape[1]
    rdist, rpost, rrisk, rorder = M.mbr(mids, mn, mscores.reshape(-1), nb, L + 1, 1.0)
    worst, changed = 0.0, 0
    for u in range(B):
        free = list(range(u * nb, (u + 1) * nb))
        rows = []
        for r in range(u * nb, (u + 1) * nb):  # the returned rows are a permutation of the MAP call's rows, with their scores' bits
            q = next(q for q in free if n[r] == mn[q] and ids[r].tolist() == mids[q].tolist()
                     and scores[r].view(np.int32) == mscores[q].view(np.int32))
            free.remove(q)
            rows.append(q)
            assert parts["map_rank"][r] == q - u * nb
            if np.isfinite(rrisk[q]):
                errs = [abs(float(parts["risk"][r]) - rrisk[q]) / M.bound(rrisk[q]), abs(float(parts["posterior"][r]) - rpost[q]) / M.bound(rpost[q])]
                worst = max(worst, max(errs))
                assert max(errs) <= 1.0, (name, route, r, q, errs)
            else:
                assert parts["risk"][r] == np.inf and parts["posterior"][r] == 0.0
        for first, second in zip(rows, rows[1:]):  # the order is the reference's up to near-ties
            assert rrisk[first] <= rrisk[second] + 2 * M.bound(rrisk[second]) or not np.isfinite(rrisk[second]), (name, route, u, rows)
        changed += rows[0] != u * nb
    TOPS[(name, route)] = (changed, B)
    WORST[("model " + name + " " + route, 1.0)] = worst
    print(f"{name} {route}: worst err / tolerance {worst:.4f}; top changed in {changed} of {B} utterances")


@pytest.mark.parametrize("name", MODELS)
def test_predict_and_the_explicit_map_decision(device, name):
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    from test_hip_model import batch_kwargs
    model, g = golden(name)
    # n_rescore defaults to the beam in both: the 4 of least risk among the 6 best
    ids, _, _ = predict(model, [batch_kwargs(g, device)], beam_size=SET["beam_size"], n_best=SET["n_best"], decoder="ctc", decision="mbr")
    got = ctc_beam_search(model, batch_kwargs(g, device), beam_size=SET["beam_size"], n_best=SET["n_best"], decision="mbr")
    assert len(ids) == len(got[0]) == SET["n_best"] * g["src"].shape[0]
    for r in range(len(ids)):
        assert np.asarray(ids[r])[:got[2][r]].tolist() == got[0][r, :got[2][r]].tolist() and (np.asarray(ids[r])[got[2][r]:] == model.pad_index).all()
    # decision="map" given explicitly: the bits of the call without it
    for fn, kw in ((ctc_beam_search, dict(beam_size=6, n_best=4)), (ctc_attention_rescore, dict(SET, ctc_weight=CTCW))):
        a, b = fn(model, batch_kwargs(g, device), **kw), fn(model, batch_kwargs(g, device), decision="map", mbr_scale=1.0, **kw)
        assert all(np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
                   for x, y in zip(a, b))
    parts = ctc_beam_search(model, batch_kwargs(g, device), beam_size=6, n_best=4, return_parts=True)[3]
    assert sorted(parts) == ["map_rank"] and parts["map_rank"].tolist() == list(range(4)) * g["src"].shape[0]


def test_model_level_counts(device):
    for name in MODELS:
        for route in ROUTES:
            if (name, route) not in TOPS:
                test_mbr_decision_on_a_golden_model(device, name, route)
    print("top changed (utterances): " + ", ".join(f"{m} {r}: {c} of {b}" for (m, r), (c, b) in TOPS.items()))
    assert len(TOPS) == len(MODELS) * len(ROUTES)
