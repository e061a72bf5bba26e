"""GPU: contextual biasing - js2t_context_rescore (ops.context_rescore) against tests/context_reference.py and
js2t_ctc_beam_search_ctx (ops.ctc_beam_search_ctx) against the float64 reference of tests/ctc_beam_ctx_reference.py; both are pinned
on the CPU by test_context_cpu.py and test_ctc_beam_ctx_cpu.py.

Exactness as in test_hip_ctc_beam_lm.py: ids, lengths, counts and orders are compared exactly on DECIDABLE inputs (margin >= 4
tolerances at every pruning step and between the returned scores), scores within 1e-4 max(1, |ref|).  Every comparison prints
err / tolerance.
"""
import functools

import numpy as np
import pytest
import torch

import context_reference as X
import ctc_beam_ctx_reference as Z
import ctc_beam_lm_reference as F
import ctc_beam_reference as R

pytestmark = pytest.mark.gpu

BLANK, BOS, EOS = Z.BLANK, Z.BOS, Z.EOS
PAD = -1
CW = Z.CTX_WEIGHT


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def graph(phrases, V, **kw):
    from joeys2t_amd.biasing import ContextGraph
    return ContextGraph.from_phrases(phrases, V, device="cuda:0", **kw)


# ================================================================ js2t_context_rescore
def rescore_input(seed, B, N, T, V, phrases, ragged=False, oov=False):
    """ids i64 [B, N, T], n i32 [B, N], base f32 [B, N]: hypotheses made of phrases, pieces of phrases and random ids; ragged: every
    kind of dead slot (base -inf, n < 0, n > Lp - 1 = T) and garbage ids behind the lengths; oov: ids outside 0 .. V-1 in between"""
    rs = np.random.RandomState(seed)
    ids = rs.randint(0, V, size=(B, N, T)).astype(np.int64)
    n = np.full((B, N), T, dtype=np.int32)
    for b in range(B):
        for k in range(N):
            y = []
            while len(y) < T:
                p = phrases[rs.randint(len(phrases))]
                r = rs.rand()
                y += list(p) if r < 0.5 else list(p[:max(len(p) - 1, 1)]) if r < 0.7 else [int(rs.randint(0, V))]
                if oov and rs.rand() < 0.15:
                    y.append(int(rs.choice([-1, V, V + 7, 2**40 + 1, -2**40])))
            ids[b, k] = y[:T]
            if ragged:
                n[b, k] = rs.randint(0, T + 1)
    base = rs.uniform(-30.0, -5.0, size=(B, N)).astype(np.float32)
    if ragged:
        kinds = rs.randint(0, 6, size=(B, N))
        base[kinds == 0] = -np.inf
        n[kinds == 1] = -1
        n[kinds == 2] = T + 1
        live = (kinds > 2)
        for b in range(B):
            for k in range(N):
                ids[b, k, max(int(n[b, k]), 0):] = 2**41 + 3 if live[b, k] else -5
    return ids, n, base


def decidable_rescore_input(auto, cw, *args, **kw):
    """the first seed (from 0) whose every utterance has its adjacent scores at least 4 tolerances apart under the reference"""
    for seed in range(64):
        ids, n, base = rescore_input(seed, *args, **kw)
        B, N, T = ids.shape
        ctx, score, order = X.rescore(ids, n, base, N, T + 1, auto, cw)
        if min(X.margin(score[b * N:(b + 1) * N]) for b in range(B)) >= X.DECIDABLE:
            return ids, n, base, ctx, score, order
    raise AssertionError("no decidable seed")


def check_rescore(device, phrases, V, cw, B, N, T, g=None, **kw):
    from joeys2t_amd import ops
    auto = X.Automaton(phrases, V)
    g = g or graph(phrases, V)
    ids, n, base, ctx, score, order = decidable_rescore_input(auto, cw, B, N, T, V, phrases, **kw)
    got_ctx, got_score, got_order = ops.context_rescore(torch.from_numpy(ids).to(device), torch.from_numpy(n).to(device),
                                                        torch.from_numpy(base).to(device), N, g, cw)
    torch.cuda.synchronize()
    got_ctx, got_score, got_order = got_ctx.cpu().numpy(), got_score.cpu().numpy(), got_order.cpu().numpy()
    assert got_ctx.dtype == np.int32 and got_ctx.shape == (B * N, ) and got_order.shape == (B, N)
    assert got_ctx.tolist() == ctx.tolist()
    assert got_order.tolist() == order.tolist()
    live = np.isfinite(score)
    assert (got_score[~live] == -np.inf).all() and (got_ctx[~live] == 0).all()
    err = max((abs(float(a) - b) / X.bound(b) for a, b in zip(got_score[live], score[live])), default=0.0)
    print(f"context_rescore B {B} N {N} T {T} V {V}: {int(live.sum())} live, ctx up to {int(ctx.max())}, worst err / tolerance {err:.4f}")
    assert err <= 1.0
    return ctx


SMALL = [(1, 2, 3), (3, 4), (1, 2), (5, 5, 6), (2, 3, 4, 5, 1)]


@pytest.mark.parametrize("N", [1, 32])
def test_rescore_matches_reference(device, N):
    assert check_rescore(device, SMALL, 8, 0.5, 3, N, 12).max() > 0


def test_rescore_lp_1_and_no_labels(device):
    """Lp = 1: only the empty hypothesis fits - ctx 0, score = base; a slot with a label is dead.  And T = 1 under the default Lp"""
    from joeys2t_amd import ops
    base = torch.tensor([[-3.0, -1.0, float("-inf"), -0.5]], device=device)
    n = torch.tensor([[0, 0, 0, 1]], dtype=torch.int32, device=device)
    ctx, score, order = ops.context_rescore(torch.full((1, 4, 1), 3, dtype=torch.int64, device=device), n, base, 4, graph([(3, )], 8), 0.5, Lp=1)
    assert ctx.tolist() == [0, 0, 0, 0] and score.tolist() == [-3.0, -1.0, float("-inf"), float("-inf")] and order.tolist() == [[1, 0, 2, 3]]
    assert check_rescore(device, [(3, ), (4, )], 8, 0.5, 2, 4, 1).max() == 1


def test_rescore_ragged_and_ids_outside_the_vocabulary(device):
    check_rescore(device, SMALL, 8, 0.5, 4, 8, 14, ragged=True)
    assert check_rescore(device, SMALL, 8, 0.75, 2, 6, 20, oov=True).max() > 0
    check_rescore(device, SMALL, 8, -0.5, 3, 5, 9, ragged=True, oov=True)  # a negative weight: phrases to avoid


def test_rescore_longest_phrase_and_chain(device):
    long = tuple(int(v) for v in np.random.RandomState(3).randint(0, 6, size=32))
    assert check_rescore(device, [long, long[:5], (1, 2)], 6, 0.25, 2, 4, 80).max() >= 32
    # the chain case: a a a a b against a a a a a a b, and 32 equal tokens (max_fail 32)
    from joeys2t_amd import ops
    g = graph([(0, 0, 0, 0, 1)], 2)
    ids = torch.tensor([[0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 1, 0, 0, 0]], device=device)
    ctx, _, _ = ops.context_rescore(ids, torch.tensor([7, 7], dtype=torch.int32, device=device), torch.zeros(2, device=device), 2, g, 1.0)
    assert g.max_fail == 4 and ctx.tolist() == [5, 0]
    g = graph([(1, ) * 32], 2)
    ids = torch.ones((1, 70), dtype=torch.int64, device=device)
    ctx, _, _ = ops.context_rescore(ids, torch.tensor([70], dtype=torch.int32, device=device), torch.zeros(1, device=device), 1, g, 1.0)
    assert g.max_fail == 32 and ctx.tolist() == [39 * 32]


@functools.lru_cache(maxsize=None)
def big_graph():
    """about 2000 phrases at V = 5000 at max_load 0.95, built once per process: do not modify"""
    phrases = X.random_phrases(np.random.RandomState(7), 5000, 2000, lengths=(2, 6), share=0.3)
    return phrases, graph(phrases, 5000, max_load=0.95)


def test_rescore_large_graph_at_high_load(device):
    phrases, g = big_graph()
    assert g.max_probe > 4 and g.n_nodes > 4000
    assert check_rescore(device, phrases, 5000, 0.5, 2, 8, 24, g=g).max() > 0


def test_rescore_weight_zero_reads_nothing(device):
    """NULL graph, a poisoned graph and NULL ids: base's bits, ctx 0, the order of the base scores"""
    from joeys2t_amd import ops
    from joeys2t_amd._lib import lib
    ids, n, base = (torch.from_numpy(a).to(device) for a in rescore_input(1, 2, 5, 9, 8, SMALL, ragged=True))
    none = ops.context_rescore(ids, n, base, 5, None, 0.0)
    bad = graph(SMALL, 8)
    bad.nodes_dev.fill_(-1)
    bad.edges_dev.fill_(-1)
    assert same_bits(ops.context_rescore(ids, n, base, 5, bad, 0.0), none)
    live = torch.from_numpy(np.isfinite(X.rescore(ids.cpu().numpy(), n.cpu().numpy(), base.cpu().numpy(), 5, 10, None, 0.0)[1])).to(device)
    assert 0 < int(live.sum()) < 10 and not none[0].any()
    assert same_bits([none[1]], [torch.where(live, base.view(-1), torch.full_like(base.view(-1), float("-inf")))])
    out = [torch.empty_like(t) for t in none]
    assert lib().js2t_context_rescore(None, 9, n.data_ptr(), base.data_ptr(), None, None, 0, 0, 0, 0, out[0].data_ptr(), out[1].data_ptr(),
                                      out[2].data_ptr(), 2, 5, 10, 8, 0.0, None) == 0
    torch.cuda.synchronize()
    assert same_bits(out, none)


def test_rescore_argument_errors(device):
    from joeys2t_amd import ops
    from joeys2t_amd._lib import lib
    g = graph(SMALL, 8)
    ids, n, base = (torch.from_numpy(a).to(device) for a in rescore_input(1, 2, 5, 9, 8, SMALL))
    ctx = torch.full((10, ), 77, dtype=torch.int32, device=device)
    score = torch.full((10, ), 77.0, device=device)
    order = torch.full((2, 5), 77, dtype=torch.int32, device=device)
    good = dict(ids=ids.data_ptr(), ids_stride=9, n=n.data_ptr(), base=base.data_ptr(), nodes=g.nodes_dev.data_ptr(), edges=g.edges_dev.data_ptr(),
                capacity=g.capacity, max_probe=g.max_probe, n_nodes=g.n_nodes, max_fail=g.max_fail, ctx=ctx.data_ptr(), score=score.data_ptr(),
                order=order.data_ptr(), B=2, N=5, Lp=10, V=8, context_weight=0.5, stream=None)

    def call(**change):
        return lib().js2t_context_rescore(*dict(good, **change).values())

    bad = [(dict(N=0), b"N 0 outside"), (dict(N=33), b"N 33 outside"), (dict(Lp=0), b"Lp 0 below"), (dict(ids_stride=8), b"ids_stride 8 below"),
           (dict(B=-1), b"bad shape"), (dict(context_weight=float("nan")), b"not finite"), (dict(context_weight=float("inf")), b"not finite"),
           (dict(nodes=None), b"null pointer (context graph"), (dict(edges=None), b"null pointer (context graph"), (dict(ids=None), b"null pointer (ids"),
           (dict(nodes=g.nodes_dev.data_ptr() + 8), b"not 16-byte aligned"), (dict(n_nodes=1), b"1 context nodes outside"),
           (dict(n_nodes=65536), b"65536 context nodes outside"), (dict(capacity=g.capacity + 1), b"is no power of two"),
           (dict(max_probe=0), b"max_probe 0 outside"), (dict(max_fail=0), b"max_fail 0 outside"), (dict(max_fail=33), b"max_fail 33 outside"),
           (dict(V=65536), b"V 65536 outside")]
    bad += [({k: None}, b"null pointer") for k in ("n", "base", "ctx", "score", "order")]
    for change, msg in bad:
        rc = call(**change)
        assert rc < 0 and msg in lib().js2t_last_error(), (change, rc, lib().js2t_last_error())
    torch.cuda.synchronize()
    assert (ctx == 77).all() and (score == 77.0).all() and (order == 77).all()  # nothing was launched
    assert call(B=0, n=None) == 0 and call() == 0
    torch.cuda.synchronize()
    from joeys2t_amd.biasing import ContextGraph
    with pytest.raises(ops.Js2tError, match="context_weight 0 expected"):
        ops.context_rescore(ids, n, base, 5, None, 0.5)
    with pytest.raises(ops.Js2tError, match="context.to"):
        ops.context_rescore(ids, n, base, 5, ContextGraph.from_phrases(SMALL, 8), 0.5)


# ================================================================ js2t_ctc_beam_search_ctx
def tables(device, logits, C, blank=BLANK):
    from joeys2t_amd import ops
    lg = torch.as_tensor(logits).to(device).contiguous()
    V = lg.shape[-1]
    lse, _ = ops.row_lse(lg.view(-1, V))
    cand_id, cand_lp, _ = ops.ctc_beam_candidates(lg.float().view(-1, V), C, blank)
    return lg, lse, cand_id, cand_lp


@functools.lru_cache(maxsize=None)
def device_lm(name):
    """the case's LM as a device table, built once per process and shared: do not modify"""
    from joeys2t_amd.lm import NGramLM
    return NGramLM.from_ngrams(F.case_lm(name), F.CASES[name]["V"], device="cuda:0")


@functools.lru_cache(maxsize=None)
def case_graph(name, w, b):
    """the pinned case's phrase graph on the device, built once per process and shared: do not modify"""
    return graph(Z.case_phrases(name, Z.SEEDS[(name, w, b)]), Z.CASES[name]["V"])


def run(device, logits, in_len, K, C, n_best, lm, w, b, g, cw, **kw):
    from joeys2t_amd import ops
    lg, lse, cand_id, cand_lp = tables(device, logits, C)
    out = ops.ctc_beam_search_ctx(lg, lse, cand_id, cand_lp, torch.as_tensor(in_len).to(device), K, n_best, BLANK, PAD, lm, BOS, EOS, w, b, g, cw, **kw)
    torch.cuda.synchronize()
    return out


def case_input(name, w, b):
    return torch.from_numpy(Z.case_logits(name, Z.SEEDS[(name, w, b)]))


@functools.lru_cache(maxsize=None)
def clean(name, w, b):
    """the pinned case run once on the GPU and shared by the tests that compare against it: do not modify"""
    c = Z.CASES[name]
    return run(torch.device("cuda:0"), case_input(name, w, b), c["in_len"], c["K"], c["C"], c["n_best"], device_lm(name) if w else None, w, b,
               case_graph(name, w, b), CW)


def check_utterance(out, u, hyps, n_best, what):
    """utterance u of (ids, lengths, final, ctc, lm, ctx) against the reference's hypotheses: exact ids, lengths, counts, pad fill,
    the three scores in tolerance; the slots without a prefix -inf / -inf / -inf, count 0, length 0, all pad"""
    ids, n, score, ctc, lms, ctx = (o[u].cpu().numpy() for o in out)
    assert ids.shape[0] == n.shape[0] == score.shape[0] == ctc.shape[0] == lms.shape[0] == ctx.shape[0] == n_best
    for i in range(n_best):
        if i < len(hyps):
            y, s, c, l, k = hyps[i]
            errs = [abs(float(score[i]) - s) / Z.bound(s), abs(float(ctc[i]) - c) / Z.bound(c), abs(float(lms[i]) - l) / Z.bound(l)]
            print(f"{what} utterance {u} slot {i}: len {n[i]} ctx {ctx[i]} final {score[i]:.6f} ref {s:.6f} err/tol {errs[0]:.3f}, ctc {errs[1]:.3f}, "
                  f"lm {errs[2]:.3f}")
            assert n[i] == len(y) and ids[i, :len(y)].tolist() == list(y), (what, u, i, ids[i, :n[i]].tolist(), y)
            assert (ids[i, len(y):] == PAD).all() and ctx[i] == k, (what, u, i, ctx[i], k)
            assert max(errs) <= 1.0, (what, u, i, (score[i], ctc[i], lms[i]), (s, c, l))
        else:
            assert score[i] == -np.inf and ctc[i] == -np.inf and lms[i] == -np.inf and n[i] == 0 and ctx[i] == 0 and (ids[i] == PAD).all(), (what, u, i)


@pytest.mark.parametrize("name, w, b", Z.PINNED)
def test_pinned_case_matches_reference(device, name, w, b):
    c = Z.CASES[name]
    out = clean(name, w, b)
    assert out[0].shape == (c["B"], c["n_best"], c["T"]) and out[0].dtype == torch.int64 and out[1].dtype == torch.int32
    assert all(o.shape == (c["B"], c["n_best"]) for o in out[2:]) and out[5].dtype == torch.int32
    for u, (hyps, margin) in enumerate(Z.case_reference(name, w, b)):
        assert margin >= Z.DECIDABLE
        check_utterance(out, u, hyps, c["n_best"], f"{name}@{w}+{b}")


@pytest.mark.parametrize("name, w, b", Z.PINNED)
def test_out_ctx_is_what_context_rescore_counts(device, name, w, b):
    from joeys2t_amd import ops
    c = Z.CASES[name]
    ids, n, score, ctc, lms, ctx = clean(name, w, b)
    got, sc, _ = ops.context_rescore(ids, n, ctc, c["n_best"], case_graph(name, w, b), CW)
    torch.cuda.synchronize()
    assert torch.equal(got.view_as(ctx), ctx) and ctx.max() > 0
    if w == 0 and b == 0:  # final = ctc + cw * ctx: the same two roundings in both kernels
        assert same_bits([sc.view_as(score)], [score])


@pytest.mark.parametrize("K", Z.WINS_K)
def test_biasing_returns_what_rescoring_cannot(device, K):
    """the kernel returns the reference's biased best, which holds a phrase; the CTC-only beam of the same K (ops.ctc_beam_search)
    does not hold that labelling, so ops.context_rescore over it cannot return it, and its best score is lower"""
    from joeys2t_amd import ops
    w = Z.WINS
    ok, biased, route, _, phrases = Z.wins_reference(K)
    assert ok
    g = graph(phrases, w["V"])
    x = torch.from_numpy(Z.wins_logits(K))
    out = run(device, x, [w["T"]], K, w["C"], 1, None, 0.0, 0.0, g, w["context_weight"])
    check_utterance(out, 0, biased[:1], 1, f"wins K {K}")
    assert int(out[5][0, 0]) > 0
    lg, lse, cand_id, cand_lp = tables(device, x, w["C"])
    ids, n, ctc = ops.ctc_beam_search(lg, lse, cand_id, cand_lp, torch.as_tensor([w["T"]]).to(device), K, K, BLANK, PAD)
    _, score, order = ops.context_rescore(ids, n, ctc, K, g, w["context_weight"])
    torch.cuda.synchronize()
    ids, n, score, order = ids[0].cpu().numpy(), n[0].cpu().numpy(), score.cpu().numpy(), order[0].cpu().numpy()
    kept = [tuple(ids[k, :n[k]].tolist()) for k in range(K)]
    assert biased[0][0] not in kept and kept[order[0]] == route[0][0]
    assert abs(float(score[order[0]]) - route[0][1]) <= Z.bound(route[0][1])
    assert float(out[2][0, 0]) >= float(score[order[0]]) + 4 * Z.bound(route[0][1])


# ---------------------------------------------------------------- weights of zero
@pytest.mark.parametrize("name, w, b", [p for p in F.PINNED if p[0] in ("short", "k8", "k32", "bf16", "identity_lm")])
def test_zero_context_weight_is_the_lm_search(device, name, w, b):
    """context_weight 0 with NULL graph pointers, and with a graph whose tables are poisoned: ids, lengths and the three scores are
    js2t_ctc_beam_search_lm's bits; out_ctx is 0"""
    from joeys2t_amd import ops
    c = F.CASES[name]
    x = torch.from_numpy(F.case_logits(name, w, b))
    x = x.to(torch.bfloat16) if c.get("bf16") else x
    lg, lse, cand_id, cand_lp = tables(device, x, c["C"])
    il = torch.as_tensor(c["in_len"]).to(device)
    args = (lg, lse, cand_id, cand_lp, il, c["K"], c["n_best"], BLANK, PAD, device_lm(name), BOS, EOS, w, b)
    want = ops.ctc_beam_search_lm(*args)
    none = ops.ctc_beam_search_ctx(*args, None, 0.0)
    bad = graph([(1, 2), (2, 3, 1)], c["V"])
    bad.nodes_dev.fill_(-1)
    bad.edges_dev.fill_(-1)
    poisoned = ops.ctc_beam_search_ctx(*args, bad, 0.0)
    torch.cuda.synchronize()
    assert same_bits(none[:5], want) and same_bits(poisoned, none) and not none[5].any()


@pytest.mark.parametrize("name", list(R.CASES))
def test_all_weights_zero_is_the_ctc_only_search(device, name):
    from joeys2t_amd import ops
    c = R.CASES[name]
    x = torch.from_numpy(R.case_logits(name))
    x = x.to(torch.bfloat16) if c.get("bf16") else x
    lg, lse, cand_id, cand_lp = tables(device, x, c["C"])
    il = torch.as_tensor(c["in_len"]).to(device)
    want = ops.ctc_beam_search(lg, lse, cand_id, cand_lp, il, c["K"], c["n_best"], BLANK, PAD)
    got = ops.ctc_beam_search_ctx(lg, lse, cand_id, cand_lp, il, c["K"], c["n_best"], BLANK, PAD, None, min(BOS, c["V"] - 1), min(EOS, c["V"] - 1),
                                  0.0, 0.0, None, 0.0)
    torch.cuda.synchronize()
    assert same_bits(got[:3], want) and same_bits(got[3:4], want[2:3]) and not got[5].any()


# ---------------------------------------------------------------- edges and invariants
SHORT = ("short", 0.5, 0.5)


def short_args():
    c = Z.CASES["short"]
    return c, (c["K"], c["C"], c["n_best"], device_lm("short"), 0.5, 0.5, case_graph(*SHORT), CW)


def test_no_frames_and_clamped_length(device):
    c, args = short_args()
    out = run(device, case_input(*SHORT), [c["T"] + 7, 0, 1], *args)
    ref = Z.case_reference(*SHORT)
    check_utterance(out, 0, ref[0][0], c["n_best"], "clamped")
    auto = X.Automaton(Z.case_phrases("short", Z.SEEDS[SHORT]), c["V"])
    empty, _ = Z.beam_search(np.zeros((0, c["V"])), c["K"], c["C"], c["n_best"], BLANK, F.case_lm("short"), c["V"], c["order"], BOS, EOS, 0.5, 0.5,
                             auto, CW)
    assert len(empty) == 1 and empty[0][0] == () and empty[0][4] == 0
    check_utterance(out, 1, empty, c["n_best"], "no frames")
    check_utterance(out, 2, ref[2][0], c["n_best"], "one frame")


def test_an_utterance_alone_and_in_a_batch(device):
    c, args = short_args()
    x = case_input(*SHORT)
    for u in range(c["B"]):
        one = run(device, x[u:u + 1], c["in_len"][u:u + 1], *args)
        assert same_bits(one, [o[u:u + 1] for o in clean(*SHORT)]), u


def test_garbage_behind_the_length_in_the_workspace_and_in_ignored_slots(device):
    from joeys2t_amd import ops
    c, _ = short_args()
    B, T, V = c["B"], c["T"], c["V"]
    lg, lse, cand_id, cand_lp = tables(device, case_input(*SHORT), c["C"])
    il = torch.as_tensor(c["in_len"]).to(device)
    args = (il, c["K"], c["n_best"], BLANK, PAD, device_lm("short"), BOS, EOS, 0.5, 0.5, case_graph(*SHORT), CW)
    again = ops.ctc_beam_search_ctx(lg, lse, cand_id, cand_lp, *args)
    rows = cand_id.shape[0]
    col = lambda v, dt: torch.full((rows, 1), v, dtype=dt, device=device)  # noqa: E731
    cand_id = torch.cat([col(BLANK, torch.int64), cand_id[:, :1], col(V, torch.int64), cand_id[:, 1:], col(5, torch.int64)], dim=1).contiguous()
    cand_lp = torch.cat([col(0.0, torch.float32), cand_lp[:, :1], col(0.0, torch.float32), cand_lp[:, 1:], col(float("-inf"), torch.float32)],
                        dim=1).contiguous()
    dead = (torch.arange(T)[None, :] >= torch.as_tensor(c["in_len"])[:, None]).to(device)
    lg, lse = lg.clone(), lse.clone()
    lg[dead] = float("nan")
    lse[dead.view(-1)] = float("nan")
    cand_lp[dead.view(-1)] = float("nan")
    cand_id[dead.view(-1)] = 2**40 + 5
    ws = torch.full((ops.ctc_beam_workspace_bytes(B, T, c["K"]) + 64, ), 0xFF, dtype=torch.uint8, device=device)
    out = ops.ctc_beam_search_ctx(lg, lse, cand_id, cand_lp, *args, workspace=ws)
    torch.cuda.synchronize()
    assert same_bits(again, clean(*SHORT)) and same_bits(out, clean(*SHORT))


def test_packed_rows_equal_padded(device):
    from joeys2t_amd import ops
    c, _ = short_args()
    B, T, V = c["B"], c["T"], c["V"]
    lg, lse, cand_id, cand_lp = tables(device, case_input(*SHORT), c["C"])
    pk = ops.PackedRows.from_lengths(list(c["in_len"]), T, device, round_to=16)
    live = (torch.arange(T)[None, :] < torch.as_tensor(c["in_len"])[:, None]).view(-1).to(device)
    n_live = int(sum(c["in_len"]))

    def packed(t, fill):
        out = torch.full((pk.rows, ) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=device)
        out[:n_live] = t[live]
        return out

    out = ops.ctc_beam_search_ctx(packed(lg.view(B * T, V), 0.0), packed(lse, 0.0), packed(cand_id, 0), packed(cand_lp, 0.0),
                                  torch.as_tensor(c["in_len"]).to(device), c["K"], c["n_best"], BLANK, PAD, device_lm("short"), BOS, EOS, 0.5, 0.5,
                                  case_graph(*SHORT), CW, pack=pk)
    torch.cuda.synchronize()
    assert same_bits(out, clean(*SHORT))


def test_large_graph_in_the_beam(device):
    """the graph of about 2000 phrases at load 0.95 under the search: logits peaked on a path made of its phrases"""
    phrases, g = big_graph()
    auto = X.Automaton(phrases, 5000)
    rs = np.random.RandomState(5)
    labels = [t for i in rs.randint(0, len(phrases), size=4) for t in phrases[i]][:10]
    path = np.array([v for lab in labels for v in (lab, BLANK, BLANK)])
    T = len(path)
    for seed in range(8):
        rs = np.random.RandomState(100 + seed)
        x = rs.randn(1, T, 5000)
        x[0, np.arange(T), path] += rs.uniform(6.0, 8.0, size=T)
        x = x.astype(np.float32)
        hyps, margin = Z.beam_search(x[0], 4, 3, 2, BLANK, None, 5000, 1, BOS, EOS, 0.0, 0.0, auto, 0.5)
        if margin >= Z.DECIDABLE:
            break
    assert margin >= Z.DECIDABLE and hyps[0][4] > 0
    out = run(device, torch.from_numpy(x), [T], 4, 3, 2, None, 0.0, 0.0, g, 0.5)
    check_utterance(out, 0, hyps, 2, "big graph")


def test_captured_launch_replays_the_same_bits(device):
    from joeys2t_amd import ops
    c, _ = short_args()
    lg, lse, cand_id, cand_lp = tables(device, case_input(*SHORT), c["C"])
    il = torch.as_tensor(c["in_len"]).to(device)
    ws = torch.empty((ops.ctc_beam_workspace_bytes(c["B"], c["T"], c["K"]), ), dtype=torch.uint8, device=device)
    args = (lg, lse, cand_id, cand_lp, il, c["K"], c["n_best"], BLANK, PAD, device_lm("short"), BOS, EOS, 0.5, 0.5, case_graph(*SHORT), CW)
    want = clean(*SHORT)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = ops.ctc_beam_search_ctx(*args, workspace=ws)  # first launch outside the capture
        rs = ops.context_rescore(first[0], first[1], first[3], c["n_best"], case_graph(*SHORT), CW)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want_rs = [t.clone() for t in rs]
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        out = ops.ctc_beam_search_ctx(*args, workspace=ws)
        rs = ops.context_rescore(out[0], out[1], out[3], c["n_best"], case_graph(*SHORT), CW)
    for _ in range(2):
        for o in (*out, *rs):
            o.fill_(7)
        ws.fill_(0x5A)
        graph_.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want) and same_bits(rs, want_rs)


def test_argument_errors(device):
    """every limit of the header: a negative return with a message, nothing launched (the outputs keep their fill)"""
    from joeys2t_amd import ops
    from joeys2t_amd._lib import lib
    name = "k8"
    c = Z.CASES[name]
    B, T, V = c["B"], c["T"], c["V"]
    lm, g = device_lm(name), case_graph(name, 0.5, 0.5)
    lg, lse, cand_id, cand_lp = tables(device, case_input(name, 0.5, 0.5), c["C"])
    il = torch.as_tensor(c["in_len"]).to(device)
    ids = torch.full((B, 1, T), 77, dtype=torch.int64, device=device)
    n, ctx = (torch.full((B, 1), 77, dtype=torch.int32, device=device) for _ in range(2))
    score, ctc, lms = (torch.full((B, 1), 77.0, dtype=torch.float32, device=device) for _ in range(3))
    ws = torch.empty((ops.ctc_beam_workspace_bytes(B, T, 4), ), dtype=torch.uint8, device=device)
    good = dict(logits=lg.data_ptr(), dt=0, lse=lse.data_ptr(), cand_id=cand_id.data_ptr(), cand_lp=cand_lp.data_ptr(), in_len=il.data_ptr(),
                uni=lm.uni_dev.data_ptr(), table=lm.table_dev.data_ptr(), capacity=lm.capacity, max_probe=lm.max_probe, lm_order=lm.order,
                nodes=g.nodes_dev.data_ptr(), edges=g.edges_dev.data_ptr(), ccap=g.capacity, cprobe=g.max_probe, n_nodes=g.n_nodes,
                max_fail=g.max_fail, out_ids=ids.data_ptr(), out_len=n.data_ptr(), out_score=score.data_ptr(), out_ctc=ctc.data_ptr(),
                out_lm=lms.data_ptr(), out_ctx=ctx.data_ptr(), workspace=ws.data_ptr(), B=B, T=T, V=V, beam=4, n_cand=c["C"], n_best=1,
                blank=BLANK, pad=PAD, bos=BOS, eos=EOS, lm_weight=0.5, context_weight=1.0, length_bonus=0.5, row_offsets=None, stream=None)
    assert len(good) == 39

    def call(**change):
        return lib().js2t_ctc_beam_search_ctx(*dict(good, **change).values())

    bad = [(dict(beam=0), b"beam 0 outside"), (dict(beam=33), b"beam 33 outside"), (dict(n_cand=9), b"9 candidates outside"),
           (dict(n_best=5), b"n_best 5 outside"), (dict(T=2**31 // 32), b"frames exceed"), (dict(blank=V), b"blank 37 outside"),
           (dict(dt=7), b"bad dtype"), (dict(T=0), b"bad shape"), (dict(V=65536), b"V 65536 outside"), (dict(bos=V), b"bos 37 outside"),
           (dict(lm_order=5), b"order 5 outside"), (dict(lm_weight=float("nan")), b"not finite"), (dict(uni=None), b"null pointer (uni"),
           (dict(context_weight=float("nan")), b"not finite"), (dict(context_weight=float("-inf")), b"not finite"),
           (dict(nodes=None), b"null pointer (context graph"), (dict(edges=None), b"null pointer (context graph"),
           (dict(edges=g.edges_dev.data_ptr() + 8), b"context graph not 16-byte aligned"), (dict(n_nodes=1), b"1 context nodes outside"),
           (dict(n_nodes=65536), b"65536 context nodes outside"), (dict(ccap=0), b"context capacity 0 is no power"),
           (dict(ccap=g.capacity - 1), b"is no power of two"), (dict(cprobe=0), b"context max_probe 0 outside"),
           (dict(cprobe=g.capacity + 1), b"context max_probe"), (dict(max_fail=0), b"max_fail 0 outside"), (dict(max_fail=33), b"max_fail 33 outside"),
           (dict(out_ctx=None), b"null pointer"), (dict(out_ctc=None), b"null pointer")]
    bad += [({k: None}, b"null pointer") for k in ("logits", "lse", "cand_id", "cand_lp", "in_len", "out_ids", "out_len", "out_score", "workspace")]
    for change, msg in bad:
        rc = call(**change)
        assert rc < 0 and msg in lib().js2t_last_error(), (change, rc, lib().js2t_last_error())
    torch.cuda.synchronize()
    assert (ids == 77).all() and (n == 77).all() and (ctx == 77).all() and all((t == 77.0).all() for t in (score, ctc, lms))
    assert call(B=0, logits=None, out_ctx=None) == 0
    # a weight of 0 leaves its model out: no LM, no graph, neither
    assert call(context_weight=0.0, nodes=None, edges=None, ccap=0, cprobe=0, n_nodes=0, max_fail=0) == 0
    assert call(lm_weight=0.0, uni=None, table=None, capacity=0, max_probe=0) == 0
    assert call() == 0
    torch.cuda.synchronize()
    args = (lg, lse, cand_id, cand_lp, il, 4, 1, BLANK, PAD, lm, BOS, EOS, 0.5, 0.0)
    from joeys2t_amd.biasing import ContextGraph
    with pytest.raises(ops.Js2tError, match="context_weight 0 expected"):
        ops.ctc_beam_search_ctx(*args, None, 1.0)
    with pytest.raises(ops.Js2tError, match="the context graph is over 11 ids"):
        ops.ctc_beam_search_ctx(*args, case_graph(*SHORT), 1.0)
    with pytest.raises(ops.Js2tError, match="context.to"):
        ops.ctc_beam_search_ctx(*args, ContextGraph.from_phrases([(1, 2)], V), 1.0)


# ================================================================ model level
MODELS = ["model_pre", "model_post", "model_deepnet"]
SET = dict(beam_size=6, n_best=4, candidates=8)
MODEL_CW, CTCW, LMW = 1.0, 0.3, 0.5
PHRASE_LEN = 3
COUNTS = {}  # model -> (utterances left out of the exact comparison, utterances whose best differs from the unbiased search's)


@functools.lru_cache(maxsize=None)
def model_phrases(name):
    """Chosen on the CPU from the ORACLE's CTC logits (tests/golden): per utterance and lower-ranked hypothesis of the unbiased
    reference search (beam 6, 8 candidates), the first window of PHRASE_LEN tokens that the best hypothesis does not contain.  With
    MODEL_CW = 1.0 the reference on those logits is decidable on all 9 utterances (the smallest margin is 7.7 tolerances) and the
    best hypothesis changes on all 9; windows of 2 tokens, or weights of 1.5 and 2.0, leave up to 3 undecidable."""
    from test_hip_model import load_golden
    g = load_golden(name)
    x = g["ctc_logits"]
    in_len = g["src_mask"].reshape(x.shape[0], -1).sum(1)
    out = set()
    for u in range(x.shape[0]):
        hyps, _ = R.beam_search(x[u, :in_len[u]], SET["beam_size"], SET["candidates"], SET["beam_size"], BOS)
        best = hyps[0][0]
        for y, _ in hyps[1:]:
            for i in range(len(y) - PHRASE_LEN + 1):
                w = tuple(int(v) for v in y[i:i + PHRASE_LEN])
                if not any(tuple(best[j:j + PHRASE_LEN]) == w for j in range(len(best) - PHRASE_LEN + 1)):
                    out.add(w)
                    break
    return sorted(out)


@functools.lru_cache(maxsize=None)
def golden(name):
    """(model, golden arrays, the graph, the biased search's result with parts, the unbiased search's), once per process: do not modify"""
    from joeys2t_amd.search import ctc_beam_search
    from test_hip_model import batch_kwargs, build
    dev = torch.device("cuda:0")
    model, g = build(name, dev)
    model.eval()
    gr = graph(model_phrases(name), len(model.trg_vocab))
    biased = ctc_beam_search(model, batch_kwargs(g, dev), context=gr, context_weight=MODEL_CW, return_parts=True, **SET)
    plain = ctc_beam_search(model, batch_kwargs(g, dev), **SET)
    return model, g, gr, biased, plain


def ctc_frames(model, batch):
    with torch.no_grad():
        enc, _, src_mask, _ = model(return_type="encode", **vars(batch))
        ctc_out = model.decoder.project(model.decoder.ctc_output_layer, enc, model.runtime.compute_dtype)
    return ctc_out.float().contiguous(), src_mask.squeeze(1).sum(dim=1)


@pytest.mark.parametrize("name", MODELS)
def test_biased_search_on_a_golden_model(device, name):
    """search.ctc_beam_search(context=...) against the reference run on the device's own CTC logits: ids, counts exact and scores in
    tolerance on the decidable utterances"""
    from test_hip_model import batch_kwargs
    model, g, gr, biased, plain = golden(name)
    assert (model.bos_index, model.eos_index) == (BOS, EOS) and len(model.trg_vocab) == 20
    nb, K, C = SET["n_best"], SET["beam_size"], SET["candidates"]
    ids, scores, n, parts = biased
    logits, in_len = ctc_frames(model, batch_kwargs(g, device))
    B = logits.shape[0]
    assert ids.shape == (B * nb, max(int(n.max()), 1)) and scores.shape == (B * nb, 1) and parts["context"].shape == (B * nb, )
    assert parts["context"].dtype == np.int32 and parts["map_rank"].tolist() == list(range(nb)) * B
    auto = X.Automaton(model_phrases(name), 20)
    x = logits.cpu().numpy()
    left_out = differs = 0
    worst = 0.0
    for u in range(B):
        rows = list(range(u * nb, (u + 1) * nb))
        assert all(scores[r, 0] >= scores[r + 1, 0] for r in rows[:-1])
        differs += ids[rows[0], :n[rows[0]]].tolist() != plain[0][rows[0], :plain[2][rows[0]]].tolist()
        ref, margin = Z.beam_search(x[u, :int(in_len[u])], K, C, nb, BOS, None, 20, 1, BOS, EOS, 0.0, 0.0, auto, MODEL_CW)
        if margin < Z.DECIDABLE:
            left_out += 1
            print(f"{name} utterance {u}: margin {margin:.1f}, left out")
            continue
        assert len(ref) == nb
        for r, (y, s, _, _, k) in zip(rows, ref):
            err = abs(float(scores[r, 0]) - s) / Z.bound(s)
            worst = max(worst, err)
            assert n[r] == len(y) and ids[r, :n[r]].tolist() == list(y) and parts["context"][r] == k, (name, u, r)
            assert err <= 1.0, (name, u, r, scores[r, 0], s)
    COUNTS[name] = (left_out, differs)
    print(f"{name}: {left_out} of {B} utterances left out, the best of {differs} differs from the unbiased search's; worst err / tolerance {worst:.4f}")


def test_model_level_counts(device):
    """the comparison above cannot pass by comparing nothing: at most 2 of the 9 utterances are left out, and on at least one the
    biased search's best hypothesis is not the unbiased one's (runs the models if run alone)"""
    for name in MODELS:
        if name not in COUNTS:
            test_biased_search_on_a_golden_model(device, name)
    print("left out / best differs per model:", COUNTS)
    assert sum(v[0] for v in COUNTS.values()) <= 2
    assert sum(v[1] for v in COUNTS.values()) >= 1


@functools.lru_cache(maxsize=None)
def model_lm():
    import ngram_reference as G
    from joeys2t_amd.lm import NGramLM
    return NGramLM.from_ngrams(G.case_lm("n32"), G.CASES["n32"]["V"], device="cuda:0")


@pytest.mark.parametrize("name", MODELS)
def test_biased_search_with_the_lm(device, name):
    """lm_fusion="search": the LM and the graph in one kernel, against the reference; lm_fusion="rescore": the kernel runs with LM
    weights 0 and js2t_ngram_rescore takes its final score as the base - the bits of the two ops called by hand"""
    import ngram_reference as G
    from joeys2t_amd import ops
    from joeys2t_amd.search import ctc_beam_search
    from test_hip_model import batch_kwargs
    model, g, gr, _, _ = golden(name)
    nb, K, C = SET["n_best"], SET["beam_size"], SET["candidates"]
    auto = X.Automaton(model_phrases(name), 20)
    logits, in_len = ctc_frames(model, batch_kwargs(g, device))
    B, T, V = logits.shape
    x = logits.cpu().numpy()
    ids, scores, n, parts = ctc_beam_search(model, batch_kwargs(g, device), lm=model_lm(), lm_weight=LMW, lm_fusion="search", context=gr,
                                            context_weight=MODEL_CW, return_parts=True, **SET)
    compared = 0
    for u in range(B):
        ref, margin = Z.beam_search(x[u, :int(in_len[u])], K, C, nb, BOS, G.case_lm("n32"), 20, 3, BOS, EOS, LMW, 0.0, auto, MODEL_CW)
        if margin < Z.DECIDABLE:
            continue
        compared += 1
        for r, (y, s, _, _, k) in zip(range(u * nb, (u + 1) * nb), ref):
            assert n[r] == len(y) and ids[r, :n[r]].tolist() == list(y) and parts["context"][r] == k, (name, u, r)
            assert abs(float(scores[r, 0]) - s) <= Z.bound(s), (name, u, r, scores[r, 0], s)
    assert compared >= 1
    # the rescore route: the biased list of beam_size, re-ranked by the LM
    ids, scores, n, parts = ctc_beam_search(model, batch_kwargs(g, device), lm=model_lm(), lm_weight=LMW, context=gr, context_weight=MODEL_CW,
                                            return_parts=True, **SET)
    cand_id, cand_lp, lse = ops.ctc_beam_candidates(logits.view(B * T, V), C, BOS)
    kids, kn, kscore, _, klm, kctx = ops.ctc_beam_search_ctx(logits, lse, cand_id, cand_lp, in_len, K, K, BOS, model.pad_index, None, BOS, EOS, 0.0,
                                                             0.0, gr, MODEL_CW)
    assert not klm[torch.isfinite(kscore)].any()
    _, _, rs, order = ops.ngram_rescore(kids, kn, kscore, K, model_lm(), BOS, EOS, LMW, 0.0)
    torch.cuda.synchronize()
    rows = (order[:, :nb].to(torch.int64) + torch.arange(B, device=device)[:, None] * K).reshape(-1)
    assert np.array_equal(scores[:, 0].view(np.int32), rs[rows].cpu().numpy().view(np.int32))
    assert np.array_equal(n, kn.view(-1)[rows].cpu().numpy()) and np.array_equal(parts["context"], kctx.view(-1)[rows].cpu().numpy())
    assert all(ids[r, :n[r]].tolist() == kids.view(B * K, T)[rows[r], :n[r]].tolist() for r in range(B * nb))


@pytest.mark.parametrize("name", MODELS)
def test_attention_rescoring_of_the_biased_list(device, name):
    """ctc_attention_rescore(context=...): the first pass is the biased kernel with n_best = n_rescore - every returned row's "ctc" is
    that kernel's out_ctc, bit for bit, at the row's "ctc_rank", its labels are that slot's; js2t_rescore took the pure CTC score and
    the context term came on top: "context" is the reference's count of the labels and the score is the three terms' sum"""
    from joeys2t_amd import ops
    from joeys2t_amd.search import ctc_attention_rescore
    from test_hip_model import batch_kwargs
    model, g, gr, _, _ = golden(name)
    nb, K, C, N = SET["n_best"], SET["beam_size"], SET["candidates"], 5
    auto = X.Automaton(model_phrases(name), 20)
    ids, scores, n, parts = ctc_attention_rescore(model, batch_kwargs(g, device), ctc_weight=CTCW, n_rescore=N, return_parts=True, context=gr,
                                                  context_weight=MODEL_CW, **SET)
    logits, in_len = ctc_frames(model, batch_kwargs(g, device))
    B, T, V = logits.shape
    cand_id, cand_lp, lse = ops.ctc_beam_candidates(logits.view(B * T, V), C, BOS)
    kids, kn, _, kctc, _, kctx = (o.cpu().numpy() for o in ops.ctc_beam_search_ctx(logits, lse, cand_id, cand_lp, in_len, K, N, BOS, model.pad_index,
                                                                                  None, BOS, EOS, 0.0, 0.0, gr, MODEL_CW))
    assert ids.shape[0] == B * nb and np.isfinite(scores).all() and parts["context"].dtype == np.int32
    for r in range(B * nb):
        u, slot = r // nb, int(parts["ctc_rank"][r])
        assert parts["ctc"][r].view(np.int32) == kctc[u, slot].view(np.int32), (name, r)
        assert n[r] == kn[u, slot] and ids[r, :n[r]].tolist() == kids[u, slot, :n[r]].tolist()
        assert parts["context"][r] == kctx[u, slot] == auto.ctx(ids[r, :n[r]].tolist())
        want = CTCW * float(parts["ctc"][r]) + (1 - CTCW) * float(parts["attention"][r]) + MODEL_CW * int(parts["context"][r])
        assert abs(float(scores[r, 0]) - want) <= Z.bound(want)
    assert all(scores[r, 0] >= scores[r + 1, 0] for u in range(B) for r in range(u * nb, (u + 1) * nb - 1))
    assert parts["context"].max() > 0


@pytest.mark.parametrize("name", MODELS[:1])
def test_predict_and_the_defaults(device, name):
    """predict(decoder="ctc", context=...) is the search call; a graph with weight 0, and no graph, give the bits of a call without
    the options"""
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    from test_hip_model import batch_kwargs
    model, g, gr, biased, plain = golden(name)
    K, nb = SET["beam_size"], SET["n_best"]
    ids, sentences, scores = predict(model, [batch_kwargs(g, device)], beam_size=K, n_best=nb, return_prob="hyp", decoder="ctc", context=gr,
                                     context_weight=MODEL_CW)
    want_ids, want_scores, want_n, _ = biased
    assert len(ids) == len(sentences) == len(scores) == len(want_ids)
    for r in range(len(ids)):
        assert np.asarray(ids[r])[:want_n[r]].tolist() == want_ids[r, :want_n[r]].tolist()
        assert abs(float(scores[r][0]) - want_scores[r, 0]) <= Z.bound(want_scores[r, 0])
    same = lambda a, b: all(np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x,  # noqa: E731
                                           y.view(np.int32) if y.dtype == np.float32 else y) for x, y in zip(a, b))
    assert same(ctc_beam_search(model, batch_kwargs(g, device), context=gr, context_weight=0.0, **SET), plain)
    att = ctc_attention_rescore(model, batch_kwargs(g, device), ctc_weight=CTCW, **SET)
    assert same(ctc_attention_rescore(model, batch_kwargs(g, device), ctc_weight=CTCW, context=gr, **SET), att)
