"""GPU: js2t_nbest_confidence against the reference of tests/confidence_reference.py - the votes (`match`) exactly, posterior, conf and
hyp_conf within the project's tolerance (ctc_beam_reference.bound) - its tie rule at the pinned pairs, poison, dead slots and dead
pivots, batching, replay, its composition with js2t_mbr_rescore's posterior and the beam kernel's list, and confidence=True of the
two CTC decoders and of predict on the golden models against the same lists voted on the host."""
import functools

import numpy as np
import pytest
import torch

import confidence_reference as CR
import mbr_reference as M

pytestmark = pytest.mark.gpu

WORST = {}  # what -> worst err / tolerance seen
HI = 2**40 + 5
DEV = "cuda:0"


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def run(ids, n, score, N, pivot, scale=1.0, want_match=True, **kw):
    from joeys2t_amd import ops
    out = ops.nbest_confidence(ids, n, score, N, pivot, scale, want_match=want_match, **kw)
    torch.cuda.synchronize()
    return out


def check(out, ref, what):
    """(posterior, conf, hyp_conf, match) against the reference's: the votes exact, the rest in tolerance, exact zeros where the
    reference has none"""
    post, conf, hyp, match = (o.cpu().numpy() for o in out)
    rpost, rconf, rhyp, rmatch = ref
    assert post.shape == rpost.shape and conf.shape == rconf.shape and hyp.shape == rhyp.shape and match.shape == rmatch.shape, what
    assert post.dtype == conf.dtype == hyp.dtype == np.float32 and match.dtype == np.uint8
    assert np.array_equal(match, rmatch), (what, np.argwhere(match != rmatch)[:8])
    worst = 0.0
    for got, want in ((post, rpost), (conf, rconf), (hyp, rhyp)):
        tol = np.vectorize(M.bound, otypes=[np.float64])(want)  # ctc_beam_reference.bound, elementwise
        if got.size:
            worst = max(worst, float((np.abs(got.astype(np.float64) - want) / tol).max()))
        assert (got[want == 0.0] == 0.0).all(), what
    print(f"{what}: worst err / tolerance {worst:.4f}")
    WORST[what] = max(WORST.get(what, 0.0), worst)
    assert worst <= 1.0, (what, worst)


# ---------------------------------------------------------------- the inputs
def all_pivots(B, N, seed):
    """i32 [B, N]: every slot of every utterance is pivot once, in a shuffled order"""
    rs = np.random.RandomState(seed)
    return np.stack([rs.permutation(N) for _ in range(B)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(ids, n, score, pivot, N, Lp) of a named case, NumPy: do not modify"""
    if name in M.CASES:
        x = dict(M.case_inputs(name))
        c = M.CASES[name]
        x.update(N=c["N"], Lp=c["T"] + 1, pivot=all_pivots(c["B"], c["N"], c["base"]))
        if name == "ragged":  # dead pivots among them: outside the list, and slots the case makes dead
            x["pivot"] = np.array([[0, 1, 2, 3, 4], [-1, 5, 0, 2, 1], [3, 0, 1, 2, 4], [2, 0, 77, -2**31, 4]], dtype=np.int32)
        return x
    rs = np.random.RandomState({"all_edges": 11, "tiles4": 12, "pins": 13, "same": 14, "lds_edge": 15}[name])
    if name == "all_edges":  # variants of one row at every edge length, cut from its front or its back, and an unrelated row
        B, N, T = 1, len(M.EDGE_LENGTHS) + 1, 131
        ids = rs.randint(1, M.V, size=(B, N, T)).astype(np.int64)
        n = np.zeros((B, N), dtype=np.int32)
        base = rs.randint(1, M.V, size=129).tolist()
        for k, length in enumerate(M.EDGE_LENGTHS):
            M._fill(ids, n, 0, k, M.variant(rs, base[:length] if k % 2 else base[len(base) - length:], 3, length))
        n[0, N - 1] = 129  # (the random row it was filled with)
    elif name == "tiles4":  # one pair of 200 / 199 labels: four tiles of columns either way round
        B, N, T = 1, 2, 200
        ids = rs.randint(1, M.V, size=(B, N, T)).astype(np.int64)
        n = np.zeros((B, N), dtype=np.int32)
        base = rs.randint(1, M.V, size=T).tolist()
        M._fill(ids, n, 0, 0, base)
        M._fill(ids, n, 0, 1, M.variant(rs, base, 6, T - 1))
    elif name == "lds_edge":  # either side of the sizes up to which a table's codes stay in LDS: 64 columns, 256 rows; no common suffix
        B, N, T = 1, 4, 257
        ids = rs.randint(1, M.V, size=(B, N, T)).astype(np.int64)
        n = np.zeros((B, N), dtype=np.int32)
        base = rs.randint(1, M.V, size=T).tolist()
        for k, length in enumerate((256, 257, 64, 65)):
            M._fill(ids, n, 0, k, M.variant(rs, base, 4, length - 1) + [100 + k])
    elif name == "pins":  # the header's two examples as two-slot lists
        B, N, T = 2, 2, 3
        ids = np.array([[[0, 0, 9], [0, 9, 9]], [[0, 1, 0], [1, 0, 1]]], dtype=np.int64)
        n = np.array([[2, 1], [3, 3]], dtype=np.int32)
    else:  # "same": every hypothesis of an utterance is the same row
        B, N, T = 2, 5, 8
        ids = np.repeat(rs.randint(1, M.V, size=(B, 1, T)), N, axis=1).astype(np.int64)
        n = np.repeat(np.array([[8], [5]], dtype=np.int32), N, axis=1)
    score = (-10.0 - rs.uniform(0.0, 3.0, size=(B, N))).astype(np.float32)
    return dict(ids=ids, n=n, score=score, pivot=all_pivots(B, N, 5), N=N, Lp=T + 1)


def on_device(name, P=None):
    x = inputs(name)
    t = [torch.from_numpy(x[k]).to(DEV) for k in ("ids", "n", "score")]
    pivot = torch.from_numpy(x["pivot"] if P is None else np.ascontiguousarray(x["pivot"][:, :P])).to(DEV)
    return (*t, x["N"], pivot)


@functools.lru_cache(maxsize=None)
def reference(name, scale, P=None):
    """the reference result of a case, computed once per process and shared: do not modify"""
    x = inputs(name)
    return CR.confidence(x["ids"], x["n"], x["score"], x["N"], x["pivot"] if P is None else x["pivot"][:, :P], x["Lp"], scale)


@functools.lru_cache(maxsize=None)
def clean(name, scale, P=None):
    """the case run once on the GPU and shared by the tests that compare against it: do not modify"""
    return run(*on_device(name, P), scale)


# ---------------------------------------------------------------- against the reference
@pytest.mark.parametrize("P", [1, None])
@pytest.mark.parametrize("name", ["n1", "n2", "n5", "n32"])
def test_sizes(device, name, P):
    """N = 1, 2, 5, 32 with lengths 0 .. 8, one pivot and every slot as a pivot"""
    check(clean(name, 1.0, P), reference(name, 1.0, P), f"{name} P={P or 'N'}")
    if name == "n1":  # the whole mass agrees: exact ones inside the length, exact zeros behind
        post, conf, hyp, _ = (o.cpu().numpy() for o in clean(name, 1.0, P))
        n = inputs(name)["n"]
        assert (post == 1.0).all() and (hyp == 1.0).all()
        assert all((conf[b, 0, :n[b, 0]] == 1.0).all() and (conf[b, 0, n[b, 0]:] == 0.0).all() for b in range(n.shape[0]))


@pytest.mark.parametrize("name", ["all_edges", "edges", "tiles4", "lds_edge", "hi_bits", "ragged"])
@pytest.mark.parametrize("scale", M.SCALES)
def test_case_matches_reference(device, name, scale):
    check(clean(name, scale), reference(name, scale), f"{name} scale {scale}")


def test_edges_cover_both_roles_and_every_length(device):
    x = inputs("all_edges")
    assert sorted(x["n"][0].tolist()) == sorted([*M.EDGE_LENGTHS, 129]) and sorted(x["pivot"][0].tolist()) == list(range(x["N"]))
    match = reference("all_edges", 1.0)[3]
    assert match.sum() > 1500  # the variants do agree: the DP is not trivially empty
    y = inputs("tiles4")
    assert y["n"][0].tolist() == [200, 199] and 150 < reference("tiles4", 1.0)[3][0, 0, 1].sum() < 200


def test_the_pinned_pairs(device):
    """a = [0, 0], b = [0] gives [0, 1] (a trimmed prefix would give [1, 0]); [0, 1, 0] gets [1, 1, 0] as the pivot of [1, 0, 1],
    which as a pivot gets its own path"""
    ids, n, score, N, _ = on_device("pins")
    pivot = torch.tensor([[0, 1], [0, 1]], dtype=torch.int32, device=DEV)
    out = run(ids, n, score, N, pivot)
    m = out[3].cpu().numpy()
    assert m[0, 0, 1].tolist() == [0, 1, 0] and m[0, 0, 0].tolist() == [1, 1, 0]
    assert m[1, 0, 1].tolist() == [1, 1, 0] and m[1, 1, 0].tolist() == CR.flags([1, 0, 1], [0, 1, 0])
    x = inputs("pins")
    check(out, CR.confidence(x["ids"], x["n"], x["score"], N, pivot.cpu().numpy(), x["Lp"], 1.0), "pins")


def test_rows_that_differ_above_bit_32_do_not_match(device):
    x = inputs("hi_bits")
    match = clean("hi_bits", 1.0)[3].cpu().numpy()
    low = x["ids"] & 0xFFFFFFFF
    assert all((low[0, k, :6] == low[0, 0, :6]).all() for k in range(4))  # equal in their low words ...
    for p, pv in enumerate(x["pivot"][0]):
        for j in range(4):
            assert match[0, p, j, :6].tolist() == (x["ids"][0, pv, :6] == x["ids"][0, j, :6]).astype(int).tolist()  # ... matched where all 64 bits agree
    assert match.sum() < 4 * 4 * 6


def test_identical_hypotheses_are_certain(device):
    post, conf, hyp, match = (o.cpu().numpy() for o in clean("same", 1.0))
    n = inputs("same")["n"]
    for b in range(2):
        assert (match[b, :, :, :n[b, 0]] == 1).all() and (match[b, :, :, n[b, 0]:] == 0).all()
        assert (np.abs(conf[b, :, :n[b, 0]] - 1.0) <= M.bound(1.0)).all() and (conf[b, :, n[b, 0]:] == 0.0).all()
    check(clean("same", 1.0), reference("same", 1.0), "same")


# ---------------------------------------------------------------- the posterior
@pytest.mark.parametrize("scale", M.SCALES)
@pytest.mark.parametrize("name", ["n5", "n32", "ragged", "hi_bits"])
def test_the_posterior_is_mbr_rescores_bit_for_bit(device, name, scale):
    from joeys2t_amd import ops
    ids, n, score, N, _ = on_device(name)
    want = ops.mbr_rescore(ids, n, score, N, scale)[1]
    assert torch.equal(bits(clean(name, scale)[0]), bits(want))
    post = clean(name, scale)[0]
    pivot = torch.from_numpy(inputs(name)["pivot"]).to(DEV).to(torch.int64)
    live = (pivot >= 0) & (pivot < N)
    rows = (pivot.clamp(0, N - 1) + torch.arange(pivot.shape[0], device=DEV)[:, None] * N)
    assert torch.equal(bits(clean(name, scale)[2]), bits(torch.where(live, post[rows], torch.zeros_like(post[rows]))))  # hyp_conf


@pytest.mark.parametrize("name", ["n5", "ragged"])
def test_a_one_hot_posterior_gives_the_votes_of_the_top_slot(device, name):
    """scale 1e4: all the mass on the best-scored live slot, so conf is (float)match against it, bit for bit"""
    x = inputs(name)
    post, conf, hyp, match = run(*on_device(name), 1e4)
    dead = M.dead_slots(x["n"].reshape(-1), x["score"].reshape(-1), x["Lp"]).reshape(x["n"].shape)
    for b in range(x["n"].shape[0]):
        if dead[b].all():
            assert not conf[b].any()
            continue
        top = int(np.argmax(np.where(dead[b], -np.inf, x["score"][b])))
        assert post[b * x["N"] + top] == 1.0
        assert torch.equal(bits(conf[b]), bits(match[b, :, top].float())), (name, b)


# ---------------------------------------------------------------- poison, batching, replay
def direct(ids, n, score, N, pivot, Lp, scale):
    """the entry point itself on outputs pre-filled with NaN / 77 and a workspace pre-filled with 0xAB"""
    from joeys2t_amd import _lib, ops
    B, P = pivot.shape
    out = [torch.full((B * N, ), float("nan"), device=DEV), torch.full((B, P, Lp - 1), float("nan"), device=DEV),
           torch.full((B, P), float("nan"), device=DEV), torch.full((B, P, N, Lp - 1), 77, dtype=torch.uint8, device=DEV)]
    ws = torch.full((_lib.lib().js2t_nbest_confidence_workspace(B, P, N, Lp), ), 0xAB, dtype=torch.uint8, device=DEV)
    rc = _lib.lib().js2t_nbest_confidence(ops._p(ids), ids.shape[-1], ops._p(n), ops._p(score), ops._p(pivot), *(ops._p(o) for o in out), ops._p(ws),
                                          ws.numel(), B, N, P, Lp, scale, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    return out


@pytest.mark.parametrize("name", ["ragged", "all_edges", "lds_edge", "n32"])
def test_poison_behind_the_lengths_and_in_dead_slots(device, name):
    """ids of 2^40 + 5 behind every n and throughout dead slots, the outputs pre-filled with NaN / 77, the workspace with 0xAB: the
    bits of the clean run, which a second clean launch repeats"""
    x = inputs(name)
    ids, n, score, N, pivot = on_device(name)
    assert same_bits(run(ids, n, score, N, pivot, 0.3), clean(name, 0.3))
    ids = ids.clone()
    T = ids.shape[-1]
    dead = torch.from_numpy(M.dead_slots(x["n"].reshape(-1), x["score"].reshape(-1), x["Lp"])).to(DEV).view(n.shape)
    ids[(torch.arange(T, device=DEV)[None, None, :] >= n[:, :, None]) | dead[:, :, None]] = HI
    assert same_bits(direct(ids, n, score, N, pivot, x["Lp"], 0.3), clean(name, 0.3))


@pytest.mark.parametrize("name", ["ragged", "n32"])
def test_an_utterance_alone_and_in_a_batch(device, name):
    ids, n, score, N, pivot = on_device(name)
    post, conf, hyp, match = clean(name, 0.3)
    for b in range(ids.shape[0]):
        alone = run(ids[b:b + 1].contiguous(), n[b:b + 1].contiguous(), score[b:b + 1].contiguous(), N, pivot[b:b + 1].contiguous(), 0.3)
        assert same_bits(alone, (post[b * N:(b + 1) * N], conf[b:b + 1], hyp[b:b + 1], match[b:b + 1])), (name, b)


def test_without_the_votes_the_same_bits(device):
    for name in ("all_edges", "ragged"):
        assert same_bits(run(*on_device(name), 0.3, want_match=False), clean(name, 0.3)[:3])


def test_captured_launch_replays_the_same_bits(device):
    """the entry point does not synchronise and allocates nothing itself: captured in a graph and replayed twice, the outputs
    re-filled in between, it gives the clean bits"""
    from joeys2t_amd import ops
    args = on_device("all_edges")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.nbest_confidence(*args, 0.3, want_match=True)  # first launch outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.nbest_confidence(*args, 0.3, want_match=True)
    for fill in (7, 11):
        for o in out:
            o.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, clean("all_edges", 0.3))


# ---------------------------------------------------------------- workspace, limits, composition
def test_argument_errors(device):
    from joeys2t_amd import _lib, ops
    ids, n, score, N, pivot = on_device("n5")
    for kw, what in ((dict(N=0), "N 0"), (dict(N=33), "multiple of N|N 33"), (dict(scale=0.0), "scale"), (dict(scale=float("nan")), "scale"),
                     (dict(Lp=0), "Lp 0"), (dict(Lp=10), "ids_stride 8"), (dict(Lp=M.EDIT_MAX_LEN + 2), "Lp - 1")):
        with pytest.raises(ops.Js2tError, match=what):
            ops.nbest_confidence(ids, n, score, **dict(dict(N=5, pivot=pivot, scale=1.0), **kw))
    with pytest.raises(ops.Js2tError, match="pivot = contiguous i32"):
        ops.nbest_confidence(ids, n, score, 5, pivot.to(torch.int64))
    with pytest.raises(ops.Js2tError, match="P 6"):
        ops.nbest_confidence(ids, n, score, 5, torch.zeros((ids.shape[0], 6), dtype=torch.int32, device=DEV))
    with pytest.raises(ops.Js2tError, match="CPU tensor"):
        ops.nbest_confidence(ids.cpu(), n, score, 5, pivot)
    with pytest.raises(ValueError, match=r"Lp 2048, P 32 and N 32"):
        ops.nbest_confidence(torch.zeros((4, 32, M.EDIT_MAX_LEN), dtype=torch.int64, device=DEV), torch.zeros((4, 32), dtype=torch.int32, device=DEV),
                             torch.zeros((4, 32), device=DEV), 32, torch.zeros((4, 32), dtype=torch.int32, device=DEV))  # (refused before a launch)
    empty = ops.nbest_confidence(ids[:0], n[:0], score[:0], 5, pivot[:0], want_match=True)
    assert [tuple(t.shape) for t in empty] == [(0, ), (0, 5, 8), (0, 5), (0, 5, 5, 8)]
    # the entry point itself: a workspace one byte short and every NULL are refused without a launch (the outputs keep their fill)
    L = _lib.lib()
    B, P, Lp = ids.shape[0], pivot.shape[1], 9
    need = L.js2t_nbest_confidence_workspace(B, P, N, Lp)
    out = [torch.full((B * N, ), 7.0, device=DEV), torch.full((B, P, Lp - 1), 7.0, device=DEV), torch.full((B, P), 7.0, device=DEV),
           torch.full((B, P, N, Lp - 1), 7, dtype=torch.uint8, device=DEV)]
    ws = torch.zeros((need, ), dtype=torch.uint8, device=DEV)
    ptrs = [ops._p(t) for t in (ids, n, score, pivot, *out, ws)]

    def call(ptrs, ws_bytes):
        return L.js2t_nbest_confidence(ptrs[0], 8, *ptrs[1:8], ptrs[8], ws_bytes, B, N, P, Lp, 1.0, ops._stream())

    assert call(ptrs, need - 1) != 0 and b"workspace" in L.js2t_last_error()
    for k in (0, 1, 2, 3, 4, 5, 6, 8):  # every pointer but `match` (7), which may be NULL
        assert call([None if i == k else p for i, p in enumerate(ptrs)], need) != 0 and b"null pointer" in L.js2t_last_error(), k
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in out)
    assert call(ptrs, need) == 0
    torch.cuda.synchronize()
    assert same_bits(out, clean("n5", 1.0))


def test_the_beam_kernels_list_goes_straight_in(device):
    """ops.ctc_beam_search's [B, N, T] table as it is (ids_stride = T, Lp = T + 1) on the pinned `short` input of ctc_beam_reference:
    what the reference gives that list, every slot a pivot"""
    import ctc_beam_reference as CB
    from joeys2t_amd import ops
    c = CB.CASES["short"]
    lg = torch.as_tensor(CB.case_logits("short")).to(DEV).contiguous()
    B, T, V = lg.shape
    lse, _ = ops.row_lse(lg.view(-1, V))
    cand_id, cand_lp, _ = ops.ctc_beam_candidates(lg.view(-1, V), c["C"], CB.BLANK)
    ids, n, score = ops.ctc_beam_search(lg, lse, cand_id, cand_lp, torch.as_tensor(c["in_len"]).to(DEV), c["K"], c["n_best"], CB.BLANK, 1)
    N = c["n_best"]
    pivot = torch.arange(N, dtype=torch.int32, device=DEV).expand(B, N).contiguous()
    for scale in M.SCALES:
        out = run(ids, n, score, N, pivot, scale)
        ref = CR.confidence(ids.cpu().numpy(), n.cpu().numpy(), score.cpu().numpy(), N, pivot.cpu().numpy(), T + 1, scale)
        check(out, ref, f"beam list scale {scale}")
    assert int(n.max()) > 1


# ---------------------------------------------------------------- model level
MODELS = ["model_pre", "model_post", "model_deepnet"]
SET = dict(beam_size=6, n_best=4)
CTCW = 0.3
ROUTES = ["ctc", "att"]
DECISIONS = ["map", "mbr"]


@functools.lru_cache(maxsize=None)
def golden(name):
    from test_hip_model import build
    model, g = build(name, torch.device(DEV))
    model.eval()
    return model, g


def decode(name, route, **kw):
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    from test_hip_model import batch_kwargs
    model, g = golden(name)
    if route == "ctc":
        return ctc_beam_search(model, batch_kwargs(g, torch.device(DEV)), **kw)
    return ctc_attention_rescore(model, batch_kwargs(g, torch.device(DEV)), ctc_weight=CTCW, **kw)


@functools.lru_cache(maxsize=None)
def whole_list(name, route):
    """the same search with n_best = n_rescore = the beam: the whole list with its scores, once per process: do not modify"""
    return decode(name, route, beam_size=SET["beam_size"], n_best=SET["beam_size"], **({} if route == "ctc" else dict(n_rescore=SET["beam_size"])))


@pytest.mark.parametrize("decision", DECISIONS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", MODELS)
def test_confidence_on_a_golden_model(device, name, route, decision):
    """confidence=True against the whole list voted on the host by the reference, no utterance left out; ids, scores and lengths
    are the bits of the call without it"""
    model, g = golden(name)
    ids, scores, n, parts = decode(name, route, decision=decision, confidence=True, **SET)
    pids, pscores, pn = decode(name, route, decision=decision, **SET)
    assert np.array_equal(ids, pids) and np.array_equal(scores.view(np.int32), pscores.view(np.int32)) and np.array_equal(n, pn)
    nb, N = SET["n_best"], SET["beam_size"]
    B = g["src"].shape[0]
    tok, hyp = parts["token_confidence"], parts["confidence"]
    assert tok.shape == ids.shape and tok.dtype == np.float32 and hyp.shape == (B * nb, ) and hyp.dtype == np.float32
    assert ("map_rank" in parts or (route, decision) == ("att", "map")) and (decision != "mbr" or "risk" in parts)  # the parts as ever
    fids, fscores, fn = whole_list(name, route)
    pivot = np.zeros((B, nb), dtype=np.int32)
    for u in range(B):  # the returned rows are rows of the whole list, with their scores' bits
        free = list(range(u * N, (u + 1) * N))
        for r in range(u * nb, (u + 1) * nb):
            q = next(q for q in free if n[r] == fn[q] and ids[r, :n[r]].tolist() == fids[q, :fn[q]].tolist()
                     and scores[r].view(np.int32) == fscores[q].view(np.int32))
            free.remove(q)
            pivot[u, r - u * nb] = q - u * N
    L = fids.shape[1]
    rpost, rconf, rhyp, _ = CR.confidence(fids, fn, fscores.reshape(-1), N, pivot, L + 1, 1.0)
    worst = 0.0
    for r in range(B * nb):
        u, p = divmod(r, nb)
        want = rconf[u, p, :ids.shape[1]]
        dead = not np.isfinite(scores[r, 0])
        assert (tok[r, n[r]:] == 0.0).all() and (not dead or (not tok[r].any() and hyp[r] == 0.0))
        errs = np.abs(tok[r].astype(np.float64) - want) / np.array([M.bound(w) for w in want])
        worst = max(worst, float(errs.max()), abs(float(hyp[r]) - rhyp[u, p]) / M.bound(rhyp[u, p]))
    WORST[f"model {name} {route} {decision}"] = worst
    print(f"{name} {route} {decision}: worst err / tolerance {worst:.4f}; mean token confidence {tok[tok > 0].mean():.3f}")
    assert worst <= 1.0 and tok.max() <= 1.0 + 1e-4 and (tok > 0).any()


@pytest.mark.parametrize("name", MODELS)
def test_predict_carries_the_same_values(device, name):
    from joeys2t_amd.prediction import predict
    from test_hip_model import batch_kwargs
    model, g = golden(name)
    out = predict(model, [batch_kwargs(g, device)], decoder="ctc", confidence=True, **SET)
    assert len(out) == 4 and sorted(out[3]) == ["hypothesis", "token"]
    ids, _, n, parts = decode(name, "ctc", confidence=True, **SET)
    assert len(out[0]) == len(out[3]["token"]) == len(ids) and out[3]["hypothesis"].dtype == np.float32
    assert np.array_equal(out[3]["hypothesis"].view(np.int32), parts["confidence"].view(np.int32))
    for r in range(len(ids)):
        assert np.asarray(out[0][r])[:n[r]].tolist() == ids[r, :n[r]].tolist()
        t = out[3]["token"][r]
        assert t.dtype == np.float32 and t.shape == (n[r], ) and np.array_equal(t.view(np.int32), parts["token_confidence"][r, :n[r]].view(np.int32))
    with pytest.raises(ValueError, match="no such list"):
        predict(model, [batch_kwargs(g, device)], decoder="attention", confidence=True)


def test_worst_error_over_the_cases(device):
    for name in ("all_edges", "tiles4", "lds_edge", "ragged", "hi_bits"):
        for scale in M.SCALES:
            if f"{name} scale {scale}" not in WORST:
                check(clean(name, scale), reference(name, scale), f"{name} scale {scale}")
    worst = max(WORST.values())
    print(f"worst err / tolerance over {len(WORST)} comparisons: {worst:.4f} at {max(WORST, key=WORST.get)}")
    assert worst <= 1.0
