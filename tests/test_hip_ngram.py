"""GPU: n-gram LM rescoring of the n-best list (js2t_ngram_rescore, ops.ngram_rescore, the lm options of search.ctc_beam_search,
search.ctc_attention_rescore and predict) against the float64 NumPy reference of tests/ngram_reference.py (pinned on the CPU by
test_ngram_cpu.py).

Exactness.  `order` is compared exactly: every pinned case is DECIDABLE at the (lm_weight, length_bonus) it is used with (margin >= 4
tolerances between adjacent scores of an utterance; test_ngram_cpu.py::test_pinned_cases_are_decidable checks the inputs).  Token
log-probabilities, LM sums and combined scores: |x - ref| <= 1e-4 max(1, |ref|) (ctc_beam_reference.bound).  Every comparison prints
err / tolerance; the worst over the cases is printed by the last kernel-level test.
"""
import functools

import numpy as np
import pytest
import torch

import ngram_reference as G

pytestmark = pytest.mark.gpu

BOS, EOS = G.BOS, G.EOS
WORST = {}  # (case, lm_weight, length_bonus) -> worst err / tolerance seen


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def device_lm(name):
    """the case's LM as a device table, built once per process and shared: do not modify"""
    from joeys2t_amd.lm import NGramLM
    c = G.CASES[name]
    return NGramLM.from_ngrams(G.case_lm(name), c["V"], device="cuda:0", max_load=c.get("max_load", 0.5))


def on_device(name):
    x = G.case_inputs(name)
    return tuple(torch.from_numpy(x[k]).to("cuda:0") for k in ("ids", "n", "base"))


def run(name, ids, n, base, w, b, lm="case", **kw):
    from joeys2t_amd import ops
    c = G.CASES[name]
    kw.setdefault("want_tokens", True)
    out = ops.ngram_rescore(ids, n, base, c["N"], device_lm(name) if lm == "case" else lm, BOS, EOS, w, b, Lp=c["Lp"], **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def clean(name, w, b):
    """the pinned case run once on the GPU and shared by the tests that compare against it: do not modify"""
    return run(name, *on_device(name), w, b)


def garbage_outputs(like):
    return tuple(None if t is None else torch.full_like(t, 77) if t.dtype == torch.int32 else torch.full_like(t, float("nan")) for t in like)


def check_case(out, name, w, b):
    """the four outputs against the reference: order exact, values in tolerance, exact zeros behind the lengths, dead slots -inf and
    last in slot order"""
    c, x = G.CASES[name], G.case_inputs(name)
    B, N, Lp = c["B"], c["N"], c["Lp"]
    tok, lms, score, order = (o.cpu().numpy() for o in out)
    rtok, rlm, rscore, rorder = G.case_reference(name, w, b)
    assert tok.shape == (B * N, Lp) and lms.shape == score.shape == (B * N, ) and order.shape == (B, N)
    assert tok.dtype == lms.dtype == score.dtype == np.float32 and order.dtype == np.int32
    n, base = x["n"].reshape(-1), x["base"].reshape(-1)
    dead = G.dead_slots(n, base, Lp)
    worst = 0.0
    for r in range(B * N):
        if dead[r]:
            assert lms[r] == -np.inf and score[r] == -np.inf and not tok[r].view(np.int32).any(), (name, r)
            continue
        assert not tok[r, n[r] + 1:].view(np.int32).any(), (name, r)  # exactly +0.0 behind the length
        errs = [abs(float(tok[r, l]) - rtok[r, l]) / G.bound(rtok[r, l]) for l in range(n[r] + 1)]
        errs += [abs(float(lms[r]) - rlm[r]) / G.bound(rlm[r]), abs(float(score[r]) - rscore[r]) / G.bound(rscore[r])]
        worst = max(worst, max(errs))
        assert max(errs) <= 1.0, (name, w, b, r, errs)
    print(f"{name} lm_weight {w} bonus {b}: worst err / tolerance {worst:.4f}")
    assert np.array_equal(order, rorder), (name, w, b, order, rorder)
    for u in range(B):
        nd = int(dead[u * N:(u + 1) * N].sum())
        assert order[u, N - nd:].tolist() == [k for k in range(N) if dead[u * N + k]]
    WORST[(name, w, b)] = max(WORST.get((name, w, b), 0.0), worst)


# ---------------------------------------------------------------- the pinned cases against the reference
@pytest.mark.parametrize("w, b", G.COMBOS)
@pytest.mark.parametrize("name", list(G.CASES))
def test_pinned_case_matches_reference(device, name, w, b):
    check_case(clean(name, w, b), name, w, b)


def test_the_big_tables_are_what_the_cases_say(device):
    half, full = device_lm("big"), device_lm("big_full")
    assert (half.capacity, full.capacity) == (32768, 16384) and half.n_entries == full.n_entries == 15551 and full.max_probe >= 8
    assert full.table_dev.shape == (16384, 2) and full.table_dev.data_ptr() % 16 == 0 and full.uni_dev.shape == (5000, 2)
    # two layouts of one model: the same values, bit for bit
    assert same_bits(clean("big", 0.7, 0.5), clean("big_full", 0.7, 0.5))


@pytest.mark.parametrize("name", ["ragged", "big_full"])
def test_weight_zero_returns_the_base_score_s_bits(device, name):
    """lm_weight 0 and bonus 0: base_score's bits (dead slots -inf) and the stable sort of them, also with an id outside the
    vocabulary; lm_weight 0 with a bonus: no table and no unigrams are needed (lm None: NULL pointers, capacity 0)"""
    c = G.CASES[name]
    N, Lp = c["N"], c["Lp"]
    ids, n, base = on_device(name)
    ids = ids.clone()
    live = (~torch.from_numpy(G.dead_slots(n.cpu().numpy().reshape(-1), base.cpu().numpy().reshape(-1), Lp))).to(ids.device)
    first = int(torch.nonzero(live & (n.view(-1) > 0))[0])
    ids.view(c["B"] * N, -1)[first, 0] = c["V"] + 3
    assert run(name, ids, n, base, 0.5, 0.0)[2][first].item() == -np.inf  # the LM gives -inf for this live slot
    want = torch.where(live, base.view(-1), torch.full_like(base.view(-1), -np.inf))
    for lm in ("case", None):
        tok, lms, s, o = run(name, ids, n, base, 0.0, 0.0, lm=lm, V=c["V"])
        assert torch.equal(bits(s), bits(want)) and not bits(tok).any()
        assert torch.equal(bits(lms), bits(torch.where(live, torch.zeros_like(want), want)))
        key = want.cpu().numpy().reshape(c["B"], N)
        assert np.array_equal(o.cpu().numpy(), np.argsort(-key.astype(np.float64), axis=1, kind="stable"))
    _, _, sb, ob = run(name, ids, n, base, 0.0, 0.5, lm=None, V=c["V"])
    wantb = (want.double() + 0.5 * n.view(-1).double()).cpu().numpy()
    got = sb.cpu().numpy().astype(np.float64)
    assert all(g == w_ or abs(g - w_) <= G.bound(w_) for g, w_ in zip(got, wantb))
    assert all(sorted(r) == list(range(N)) for r in ob.tolist())
    assert same_bits(run(name, ids, n, base, 0.0, 0.5), run(name, ids, n, base, 0.0, 0.5, lm=None, V=c["V"]))


def test_an_id_outside_the_vocabulary(device):
    """that position is -inf, the contexts behind it are cut as specified (the reference on the same ids), the other slots untouched"""
    name = "o4"
    c = G.CASES[name]
    N, Lp, V = c["N"], c["Lp"], c["V"]
    ids, n, base = on_device(name)
    r = int(torch.nonzero(n.view(-1) >= 3)[0])
    for bad in (V, -1, 2**40 + 5):
        ids2 = ids.clone()
        ids2.view(-1, Lp + 1)[r, 1] = bad
        tok, lms, score, order = run(name, ids2, n, base, 0.3, 0.0)
        rtok, rlm, rscore, _ = G.rescore(ids2.cpu().numpy(), n.cpu().numpy(), base.cpu().numpy(), N, Lp, G.case_lm(name), V, c["order"], BOS, EOS,
                                         0.3, 0.0)
        assert tok[r, 1].item() == -np.inf and lms[r].item() == score[r].item() == -np.inf and rtok[r, 1] == -np.inf
        nr = int(n.view(-1)[r])
        for l in [0] + list(range(2, nr + 1)):
            assert abs(tok[r, l].item() - rtok[r, l]) <= G.bound(rtok[r, l]), (bad, l)
        assert sorted(order[r // N].tolist()) == list(range(N)) and order[r // N, -1].item() == r % N
        cl = clean(name, 0.3, 0.0)
        keep = [i for i in range(c["B"] * N) if i != r]
        assert same_bits([t[keep] for t in (tok, lms, score)], [t[keep] for t in cl[:3]])


def test_identical_hypotheses_keep_slot_order(device):
    name = "o3"
    N = G.CASES[name]["N"]
    ids, n, base = (t.clone() for t in on_device(name))
    ids[0, 3], n[0, 3], base[0, 3] = ids[0, 1], n[0, 1], base[0, 1]  # utterance 0: slot 3 = slot 1
    tok, lms, score, order = run(name, ids, n, base, 0.3, 0.5)
    assert bits(score)[1].item() == bits(score)[3].item() and torch.equal(bits(tok[1]), bits(tok[3]))
    o = order[0].tolist()
    assert sorted(o) == list(range(N)) and o.index(3) == o.index(1) + 1
    cl = clean(name, 0.3, 0.5)
    assert same_bits([t[N:] for t in (tok, lms, score)] + [order[1:]], [t[N:] for t in cl[:3]] + [cl[3][1:]])


def test_a_nan_base_score_keeps_the_permutation(device):
    name = "ragged"
    N = G.CASES[name]["N"]
    ids, n, base = (t.clone() for t in on_device(name))
    base[2, 1] = float("nan")
    tok, lms, score, order = run(name, ids, n, base, 0.3, 0.5)
    assert torch.isnan(score[2 * N + 1]).item() and torch.isfinite(lms[2 * N + 1]).item()
    assert all(sorted(r) == list(range(N)) for r in order.tolist()) and order[2, N - 1].item() == 1
    cl = clean(name, 0.3, 0.5)
    assert [k for k in order[2].tolist() if k != 1] == [k for k in cl[3][2].tolist() if k != 1]
    assert same_bits([t[:2 * N] for t in (tok, lms, score)] + [order[:2]], [t[:2 * N] for t in cl[:3]] + [cl[3][:2]])


@pytest.mark.parametrize("name", ["ragged", "big_full", "n32"])
def test_without_lm_tok_the_same_bits(device, name):
    got = run(name, *on_device(name), 0.7, 0.5, want_tokens=False)
    assert got[0] is None and same_bits(got[1:], clean(name, 0.7, 0.5)[1:])


@pytest.mark.parametrize("name", ["ragged", "big_full"])
def test_poison_behind_the_lengths_and_in_dead_slots(device, name):
    """ids of 2^40 + 5 and of -7 behind every n[r] and in every position of the dead slots, outputs pre-filled with garbage: the bits
    of the clean run, which a second clean launch repeats"""
    c = G.CASES[name]
    N, Lp = c["N"], c["Lp"]
    ids, n, base = on_device(name)
    again = run(name, ids, n, base, 0.3, 0.5)
    dead = torch.from_numpy(G.dead_slots(n.cpu().numpy().reshape(-1), base.cpu().numpy().reshape(-1), Lp)).to(ids.device).view(-1, 1)
    idpos = torch.arange(ids.shape[2], device=ids.device)[None, :]
    for poison in (2**40 + 5, -7):
        ids2 = ids.clone()
        ids2.view(c["B"] * N, -1)[(idpos >= n.view(-1, 1).long()) | dead] = poison
        out = garbage_outputs(clean(name, 0.3, 0.5))
        got = run(name, ids2, n, base, 0.3, 0.5, out=out)
        assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
        assert same_bits(got, clean(name, 0.3, 0.5))
    assert same_bits(again, clean(name, 0.3, 0.5))


@pytest.mark.parametrize("name", ["ragged", "big"])
def test_an_utterance_alone_and_in_a_batch(device, name):
    c = G.CASES[name]
    N = c["N"]
    ids, n, base = on_device(name)
    cl = clean(name, 0.3, 0.5)
    for u in range(c["B"]):
        s = slice(u * N, (u + 1) * N)
        one = run(name, ids[u:u + 1].contiguous(), n[u:u + 1].contiguous(), base[u:u + 1].contiguous(), 0.3, 0.5)
        assert same_bits(one, [cl[0][s], cl[1][s], cl[2][s], cl[3][u:u + 1]]), (name, u)


def test_captured_launch_replays_the_same_bits(device):
    """the entry point allocates nothing and does not synchronise: captured in a graph and replayed twice, the outputs re-filled in
    between, it gives the clean bits"""
    from joeys2t_amd import ops
    name = "ragged"
    c = G.CASES[name]
    ids, n, base = on_device(name)
    lm = device_lm(name)
    out = garbage_outputs(clean(name, 0.3, 0.5))
    args = (ids, n, base, c["N"], lm, BOS, EOS, 0.3, 0.5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ngram_rescore(*args, Lp=c["Lp"], out=out)  # first launch outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ngram_rescore(*args, Lp=c["Lp"], out=out)
    for fill in (7, 11):
        for o in out:
            o.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, clean(name, 0.3, 0.5))


def test_argument_errors(device):
    """one per rule of the header: a negative return with a message, nothing launched"""
    from joeys2t_amd import ops
    from joeys2t_amd._lib import lib
    name = "o3"
    c = G.CASES[name]
    B, N, Lp, V = c["B"], c["N"], c["Lp"], c["V"]
    ids, n, base = on_device(name)
    lm = device_lm(name)

    def op(ids=ids, n=n, base=base, N=N, lm=lm, bos=BOS, eos=EOS, w=0.3, b=0.0, **kw):
        return ops.ngram_rescore(ids, n, base, N, lm, bos, eos, w, b, **kw)

    with pytest.raises(ops.Js2tError, match="N 0 outside"):
        op(N=0)
    with pytest.raises(ops.Js2tError, match="N 33 outside"):
        op(ids=torch.zeros((1, 33, Lp), dtype=torch.int64, device=device), n=torch.zeros((33, ), dtype=torch.int32, device=device),
           base=torch.zeros((33, ), device=device), N=33)
    for who in ("bos", "eos"):
        for v in (-1, V):
            with pytest.raises(ops.Js2tError, match=f"{who} {v} outside"):
                op(**{who: v})
    for kw in (dict(w=float("nan")), dict(w=float("inf")), dict(b=float("nan")), dict(b=float("-inf"))):
        with pytest.raises(ops.Js2tError, match="not finite"):
            op(**kw)
    with pytest.raises(ops.Js2tError, match="ids_stride 6 below"):
        op(Lp=Lp + 3)
    with pytest.raises(ops.Js2tError, match="Lp 0 below"):
        op(Lp=0)
    with pytest.raises(ops.Js2tError, match="no multiple"):
        op(N=3)
    with pytest.raises(ops.Js2tError, match="out ="):
        op(Lp=Lp, out=clean(name, 0.3, 0.0)[:3])
    with pytest.raises(ops.Js2tError, match="lm_weight 0 and V"):
        op(lm=None)
    with pytest.raises(ops.Js2tError, match="lm.to"):
        op(lm=type(lm).from_ngrams(G.case_lm(name), V))
    with pytest.raises(ops.Js2tError, match="V = 12"):
        op(V=12)
    with pytest.raises(ops.Js2tError):
        op(ids=ids.cpu())
    with pytest.raises(ops.Js2tError):
        op(n=n.long())
    outs = garbage_outputs(clean(name, 0.3, 0.0))
    ptrs = [ids, n, base, lm.uni_dev, lm.table_dev, *outs]

    def call(p, B_=B, N_=N, Lp_=Lp, V_=V, bos=BOS, eos=EOS, w=0.3, b=0.0, stride=ids.shape[2], cap=lm.capacity, probe=lm.max_probe,
             order=lm.order):
        return lib().js2t_ngram_rescore(p[0], stride, p[1], p[2], p[3], p[4], cap, probe, order, p[5], p[6], p[7], p[8], B_, N_, Lp_, V_, bos,
                                        eos, w, b, None)

    full = [t.data_ptr() for t in ptrs]
    for drop in (0, 1, 2, 3, 6, 7, 8):  # (5 = lm_tok may be NULL; 4 = the table: its own message)
        rc = call([None if i == drop else v for i, v in enumerate(full)])
        assert rc < 0 and b"null pointer" in lib().js2t_last_error(), drop
    assert call([None if i == 4 else v for i, v in enumerate(full)]) < 0 and b"needs a table" in lib().js2t_last_error()
    for kw, what in ((dict(N_=0), b"N 0 outside"), (dict(N_=33), b"N 33 outside"), (dict(Lp_=0), b"Lp 0 below"), (dict(V_=1, bos=0, eos=0), b"V 1 outside"),
                     (dict(V_=65536), b"V 65536 outside"), (dict(order=0), b"order 0 outside"), (dict(order=5), b"order 5 outside"),
                     (dict(cap=48), b"capacity 48"), (dict(cap=-8), b"capacity -8"), (dict(cap=0), b"needs a table"), (dict(probe=0), b"max_probe 0"),
                     (dict(probe=lm.capacity + 1), b"max_probe"), (dict(stride=Lp - 2), b"ids_stride"), (dict(bos=V), b"bos"), (dict(eos=-1), b"eos"),
                     (dict(w=float("nan")), b"not finite"), (dict(b=float("inf")), b"not finite"), (dict(B_=2**31 // 32, N_=32), b"bad shape")):
        assert call(full, **kw) < 0 and what in lib().js2t_last_error(), kw
    misaligned = list(full)
    misaligned[4] += 8
    assert call(misaligned) < 0 and b"16-byte" in lib().js2t_last_error()
    torch.cuda.synchronize()
    assert (outs[3] == 77).all() and all(torch.isnan(o).all() for o in outs[:3])  # nothing was launched
    assert call([None] * 9, B_=0) == 0


def test_worst_error_over_the_kernel_cases(device):
    """the figure DESIGN.md quotes: the worst err / tolerance over the pinned cases (runs them if run alone)"""
    for name in G.CASES:
        for w, b in G.COMBOS:
            check_case(clean(name, w, b), name, w, b)
    print("worst err / tolerance per (case, lm_weight, bonus):", {f"{k[0]}@{k[1]}+{k[2]}": round(float(v), 4) for k, v in WORST.items()})
    assert max(WORST.values()) <= 1.0


# ---------------------------------------------------------------- model level
MODELS = ["model_pre", "model_post", "model_deepnet"]
SET = dict(beam_size=6, n_best=4, n_rescore=4)
LMW, CTCW = 0.5, 0.3
COUNTS = {}  # (model, route) -> (utterances left out of the order comparison, lists re-ordered against the first pass's list)


@functools.lru_cache(maxsize=None)
def model_lm():
    """a normalised order-3 LM over the golden models' 20 ids (the LM of the V = 20 kernel cases), on the device"""
    return device_lm("n32")


@functools.lru_cache(maxsize=None)
def golden(name):
    """(model, golden arrays, route A of both decoders, route B of both), built once per process: do not modify"""
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    from test_hip_model import batch_kwargs, build
    dev = torch.device("cuda:0")
    model, g = build(name, dev)
    model.eval()
    a = {"ctc": ctc_beam_search(model, batch_kwargs(g, dev), lm=model_lm(), lm_weight=LMW, **SET),
         "att": ctc_attention_rescore(model, batch_kwargs(g, dev), ctc_weight=CTCW, lm=model_lm(), lm_weight=LMW, return_parts=True, **SET)}
    b = {"ctc": ctc_beam_search(model, batch_kwargs(g, dev), beam_size=SET["beam_size"], n_best=SET["n_rescore"]),
         "att": ctc_attention_rescore(model, batch_kwargs(g, dev), ctc_weight=CTCW, return_parts=True, **SET)}
    return model, g, a, b


def host_route(ids, scores, n, nb):
    """route B's lists re-scored on the host by the reference: (score f64 [B * nb], order [B, nb], lm sums, token values)"""
    L = ids.shape[1]
    tok, lms, score, order = G.rescore(ids, n, scores.reshape(-1), nb, L + 1, G.case_lm("n32"), 20, 3, BOS, EOS, LMW, 0.0)
    return score, order, lms, tok


@pytest.mark.parametrize("route", ["ctc", "att"])
@pytest.mark.parametrize("name", MODELS)
def test_lm_rescoring_on_a_golden_model(device, name, route):
    model, g, a, b = golden(name)
    nb = SET["n_best"]
    B = g["src"].shape[0]
    ids, scores, n = a[route][:3]
    bids, bscores, bn = b[route][:3]
    assert ids.dtype == np.int64 and scores.dtype == np.float32 and n.dtype == np.int64
    assert ids.shape == (B * nb, max(int(n.max()), 1)) and scores.shape == (B * nb, 1) and n.shape == (B * nb, )
    assert all((ids[r, n[r]:] == model.pad_index).all() for r in range(B * nb))
    assert np.isfinite(bscores).all()  # (these utterances have more than four prefixes)
    rscore, rorder, rlm, rtok = host_route(bids, bscores, bn, nb)
    left_out = reordered = 0
    worst = 0.0
    for u in range(B):
        rows = range(u * nb, (u + 1) * nb)
        assert all(scores[r, 0] >= scores[r + 1, 0] for r in list(rows)[:-1])
        want = [u * nb + int(k) for k in rorder[u]]
        reordered += want != list(rows)
        # scores: the sorted lists agree whatever the order of near-ties
        for r, s in zip(rows, sorted((rscore[q] for q in rows), reverse=True)):
            err = abs(float(scores[r, 0]) - s) / G.bound(s)
            worst = max(worst, err)
            assert err <= 1.0, (name, route, r, scores[r, 0], s)
        if G.margin(rscore[u * nb:(u + 1) * nb]) < G.DECIDABLE:
            left_out += 1
            continue
        for r, q in zip(rows, want):
            assert n[r] == bn[q] and ids[r, :n[r]].tolist() == bids[q, :bn[q]].tolist(), (name, route, u, r, q)
            if route == "att":
                p = a["att"][3]
                assert abs(float(p["lm"][r]) - rlm[q]) <= G.bound(rlm[q])
                assert p["lm_token_log_probs"][r].shape == (n[r] + 1, ) and p["lm_token_log_probs"][r].dtype == np.float32
                assert all(abs(float(v) - rtok[q, l]) <= G.bound(rtok[q, l]) for l, v in enumerate(p["lm_token_log_probs"][r]))
                assert p["ctc"][r].view(np.int32) == b["att"][3]["ctc"][q].view(np.int32)
                assert p["attention"][r].view(np.int32) == b["att"][3]["attention"][q].view(np.int32)
    COUNTS[(name, route)] = (left_out, reordered)
    print(f"{name} {route}: {left_out} of {B} utterances left out of the order comparison, {reordered} lists re-ordered by the LM; "
          f"worst score err / tolerance {worst:.4f}")


def test_model_level_counts(device):
    """the order tests above cannot pass by comparing nothing: per route at most 3 of the 9 utterances are left out, and at least one
    list is re-ordered against the first pass's list (runs the models if run alone)"""
    for name in MODELS:
        for route in ("ctc", "att"):
            if (name, route) not in COUNTS:
                test_lm_rescoring_on_a_golden_model(device, name, route)
    print("left out / re-ordered per (model, route):", COUNTS)
    for route in ("ctc", "att"):
        assert sum(v[0] for k, v in COUNTS.items() if k[1] == route) <= 3
    assert sum(v[1] for k, v in COUNTS.items() if k[1] == "ctc") >= 1


@pytest.mark.parametrize("name", MODELS)
def test_n_best_one_is_the_first_row(device, name):
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    from test_hip_model import batch_kwargs
    model, g, a, _ = golden(name)
    nb = SET["n_best"]
    one = {"ctc": ctc_beam_search(model, batch_kwargs(g, device), lm=model_lm(), lm_weight=LMW, **dict(SET, n_best=1)),
           "att": ctc_attention_rescore(model, batch_kwargs(g, device), ctc_weight=CTCW, lm=model_lm(), lm_weight=LMW, **dict(SET, n_best=1))}
    for route in ("ctc", "att"):
        ids, scores, n = a[route][:3]
        ids1, scores1, n1 = one[route]
        assert np.array_equal(n1, n[::nb]) and np.array_equal(scores1.view(np.int32), scores[::nb].view(np.int32))
        assert np.array_equal(ids1, ids[::nb, :ids1.shape[1]]) and (ids[::nb, ids1.shape[1]:] == model.pad_index).all()


@pytest.mark.parametrize("name", MODELS)
def test_predict_with_an_lm(device, name):
    from joeys2t_amd.prediction import predict
    from test_hip_model import batch_kwargs
    from joeys2t_amd import search
    model, g, _, _ = golden(name)
    K, nb = SET["beam_size"], SET["n_best"]
    for decoder, route in (("ctc", "ctc"), ("ctc-attention", "att")):
        ids, sentences, scores = predict(model, [batch_kwargs(g, device)], beam_size=K, n_best=nb, return_prob="hyp", decoder=decoder,
                                         ctc_weight=CTCW, lm=model_lm(), lm_weight=LMW)
        # predict re-scores the whole beam (n_rescore = beam_size): the decoder's own result at those settings, in batch order
        fn = search.ctc_beam_search if route == "ctc" else search.ctc_attention_rescore
        kw = dict(beam_size=K, n_best=nb, lm=model_lm(), lm_weight=LMW, **({"ctc_weight": CTCW} if route == "att" else {}))
        want_ids, want_scores, want_n = fn(model, batch_kwargs(g, device), **kw)[:3]
        assert len(ids) == len(sentences) == len(scores) == len(want_ids)  # predict sorts the batch by length and puts the rows back
        for r in range(len(ids)):
            assert np.asarray(ids[r])[:want_n[r]].tolist() == want_ids[r, :want_n[r]].tolist()
            assert (np.asarray(ids[r])[want_n[r]:] == model.pad_index).all()
            assert abs(float(scores[r][0]) - want_scores[r, 0]) <= G.bound(want_scores[r, 0])
    with pytest.raises(ValueError, match="lm / lm_weight / length_bonus"):
        predict(model, [batch_kwargs(g, device)], decoder="attention", lm=model_lm(), lm_weight=LMW)


@pytest.mark.parametrize("name", MODELS)
def test_without_an_lm_nothing_changes(device, name):
    """lm=None and a zero bonus: the calls of the parent, bit for bit; an lm with weight 0 and no bonus re-ranks by the first pass's
    own score, which returns the same lists"""
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    from test_hip_model import batch_kwargs
    model, g, _, b = golden(name)
    plain = ctc_beam_search(model, batch_kwargs(g, device), beam_size=SET["beam_size"], n_best=SET["n_rescore"], lm=None, lm_weight=0.0,
                            length_bonus=0.0)
    zero = ctc_beam_search(model, batch_kwargs(g, device), lm=model_lm(), lm_weight=0.0, **SET)
    for got in (plain, zero):
        assert all(np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
                   for x, y in zip(got, b["ctc"]))
    att0 = ctc_attention_rescore(model, batch_kwargs(g, device), ctc_weight=CTCW, lm=model_lm(), lm_weight=0.0, **SET)
    assert all(np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
               for x, y in zip(att0, b["att"][:3]))
    assert "lm" not in b["att"][3]
    # the bonus alone: every score moves by 0.5 n, within the rounding of one addition
    ids, scores, n = ctc_beam_search(model, batch_kwargs(g, device), length_bonus=0.5, **SET)
    bids, bscores, bn = b["ctc"]
    want = sorted((float(bscores[r, 0]) + 0.5 * int(bn[r]) for r in range(SET["n_best"])), reverse=True)
    assert all(abs(float(scores[r, 0]) - want[r]) <= G.bound(want[r]) for r in range(SET["n_best"]))
