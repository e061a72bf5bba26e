"""GPU: attention rescoring of the CTC n-best (js2t_rescore, ops.rescore, search.ctc_attention_rescore,
predict(decoder="ctc-attention")) against the float64 NumPy reference of tests/rescore_reference.py (pinned on the CPU by
test_rescore_cpu.py) and, at model level, against the CPU oracle's decoder.

Exactness.  `order` is compared exactly: every pinned case is DECIDABLE at the weights it is used with (margin >= 4 tolerances between
adjacent scores of an utterance; test_rescore_cpu.py::test_pinned_cases_are_decidable checks the inputs).  Token log-probabilities,
attention sums and combined scores: |x - ref| <= 1e-4 max(1, |ref|) (ctc_beam_reference.bound, the project's budget for accumulated
log-likelihoods).  Every comparison prints err / tolerance; the worst over the cases is printed by the last kernel-level test.
"""
import functools

import numpy as np
import pytest
import torch

import rescore_reference as R

pytestmark = pytest.mark.gpu

EOS = R.EOS
WORST = {}  # (case, weight) -> worst err / tolerance seen


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def on_device(name, device=None):
    """(logits f32 or bf16 [R, Lp, V], ids, n, ctc) of a pinned case on the device"""
    device = device or torch.device("cuda:0")
    c, x = R.CASES[name], R.case_inputs(name)
    lg = torch.from_numpy(x["logits"])
    if c.get("bf16"):
        assert np.array_equal(lg.to(torch.bfloat16).float().numpy(), x["logits"])
        lg = lg.to(torch.bfloat16)
    return lg.to(device), torch.from_numpy(x["ids"]).to(device), torch.from_numpy(x["n"]).to(device), torch.from_numpy(x["ctc"]).to(device)


def run(lg, ids, n, ctc, N, w, **kw):
    from joeys2t_amd import ops
    out = ops.rescore(lg, ids, n, ctc, N, EOS, w, **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def clean(name, w):
    """the pinned case run once on the GPU and shared by the tests that compare against it: do not modify"""
    return run(*on_device(name), R.CASES[name]["N"], w)


def garbage_outputs(like):
    return tuple(torch.full_like(t, 77) if t.dtype == torch.int32 else torch.full_like(t, float("nan")) for t in like)


def check_case(out, name, w):
    """the four outputs against the reference: order exact, values in tolerance, exact zeros behind the lengths, dead slots -inf and
    last in slot order"""
    c, x = R.CASES[name], R.case_inputs(name)
    B, N, Lp = c["B"], c["N"], c["Lp"]
    tok, att, score, order = (o.cpu().numpy() for o in out)
    rtok, ratt, rscore, rorder = R.case_reference(name, w)
    assert tok.shape == (B * N, Lp) and att.shape == score.shape == (B * N, ) and order.shape == (B, N)
    assert tok.dtype == att.dtype == score.dtype == np.float32 and order.dtype == np.int32
    n, ctc = x["n"].reshape(-1), x["ctc"].reshape(-1)
    dead = R.dead_slots(n, ctc, Lp)
    worst = 0.0
    for r in range(B * N):
        if dead[r]:
            assert att[r] == -np.inf and score[r] == -np.inf and not tok[r].view(np.int32).any(), (name, r)
            continue
        assert not tok[r, n[r] + 1:].view(np.int32).any(), (name, r)  # exactly +0.0 behind the length
        errs = [abs(float(tok[r, l]) - rtok[r, l]) / R.bound(rtok[r, l]) for l in range(n[r] + 1)]
        errs += [abs(float(att[r]) - ratt[r]) / R.bound(ratt[r]), abs(float(score[r]) - rscore[r]) / R.bound(rscore[r])]
        worst = max(worst, max(errs))
        assert max(errs) <= 1.0, (name, w, r, errs)
    print(f"{name} w {w}: worst err / tolerance {worst:.4f}")
    assert np.array_equal(order, rorder), (name, w, order, rorder)
    for b in range(B):
        nd = int(dead[b * N:(b + 1) * N].sum())
        assert order[b, N - nd:].tolist() == [k for k in range(N) if dead[b * N + k]]
    WORST[(name, w)] = max(WORST.get((name, w), 0.0), worst)


# ---------------------------------------------------------------- the pinned cases against the reference
@pytest.mark.parametrize("w", R.WEIGHTS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_pinned_case_matches_reference(device, name, w):
    check_case(clean(name, w), name, w)


@pytest.mark.parametrize("name", ["ragged", "v5000", "bf16_4100"])
def test_weight_one_and_weight_zero_return_a_head_s_own_bits(device, name):
    """w = 1: the CTC scores' bits (also where the attention score is -inf) and the stable sort of them; w = 0: att_score's bits"""
    c = R.CASES[name]
    N, Lp = c["N"], c["Lp"]
    lg, ids, n, ctc = on_device(name)
    ids = ids.clone()
    live = (~torch.from_numpy(R.dead_slots(n.cpu().numpy().reshape(-1), ctc.cpu().numpy().reshape(-1), Lp))).to(device)
    first = int(torch.nonzero(live & (n.view(-1) > 0))[0])
    ids.view(c["B"] * N, -1)[first, 0] = c["V"] + 3  # a label outside the vocabulary: att_score -inf for this live slot
    tok1, att1, s1, o1 = run(lg, ids, n, ctc, N, 1.0)
    assert att1[first].item() == -np.inf and tok1[first, 0].item() == -np.inf
    want = torch.where(live, ctc.view(-1), torch.full_like(ctc.view(-1), -np.inf))
    assert torch.equal(bits(s1), bits(want))
    key = want.cpu().numpy().reshape(c["B"], N)
    assert np.array_equal(o1.cpu().numpy(), np.argsort(-key.astype(np.float64), axis=1, kind="stable"))
    _, att0, s0, o0 = run(lg, ids, n, ctc, N, 0.0)
    assert torch.equal(bits(s0), bits(att0)) and torch.equal(bits(att0), bits(att1))
    assert np.array_equal(o0.cpu().numpy(), np.argsort(-att0.cpu().numpy().astype(np.float64).reshape(c["B"], N), axis=1, kind="stable"))


def test_identical_hypotheses_keep_slot_order(device):
    name = "v20"
    c = R.CASES[name]
    N = c["N"]
    lg, ids, n, ctc = (t.clone() for t in on_device(name))
    lg[3], ids[0, 3], n[0, 3], ctc[0, 3] = lg[1], ids[0, 1], n[0, 1], ctc[0, 1]  # utterance 0: slot 3 = slot 1
    tok, att, score, order = run(lg, ids, n, ctc, N, 0.3)
    assert bits(score)[1].item() == bits(score)[3].item() and torch.equal(bits(tok[1]), bits(tok[3]))
    o = order[0].tolist()
    assert sorted(o) == list(range(N)) and o.index(3) == o.index(1) + 1
    assert same_bits([t[N:] for t in (tok, att, score)] + [order[1:]], [t[N:] for t in clean(name, 0.3)[:3]] + [clean(name, 0.3)[3][1:]])


@pytest.mark.parametrize("name", ["ragged", "v5000", "bf16_4096"])
def test_poison_behind_the_lengths_and_in_dead_slots(device, name):
    """NaN logits behind every n[r] and in every row of the dead slots, ids of 2^40 + 5 behind n, outputs pre-filled with garbage:
    the bits of the clean run, which a second clean launch repeats"""
    c = R.CASES[name]
    N, Lp = c["N"], c["Lp"]
    lg, ids, n, ctc = on_device(name)
    again = run(lg, ids, n, ctc, N, 0.3)
    lg, ids = lg.clone(), ids.clone()
    nn = n.view(-1, 1).long()
    dead = torch.from_numpy(R.dead_slots(n.cpu().numpy().reshape(-1), ctc.cpu().numpy().reshape(-1), Lp)).to(device).view(-1, 1)
    pos = torch.arange(Lp, device=device)[None, :]
    lg[(pos > nn) | dead] = float("nan")
    idpos = torch.arange(ids.shape[2], device=device)[None, :]
    ids.view(c["B"] * N, -1)[(idpos >= nn) | dead] = 2**40 + 5
    assert torch.isnan(lg.float()).any() or name != "ragged"
    out = garbage_outputs(clean(name, 0.3))
    got = run(lg, ids, n, ctc, N, 0.3, out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    assert same_bits(again, clean(name, 0.3)) and same_bits(got, clean(name, 0.3))


def test_nan_in_a_live_row_keeps_the_permutation(device):
    """an output property on valid memory: a NaN logit in one live row makes that slot's scores NaN, `order` stays a permutation with
    that slot behind every finite one, and the other utterance keeps its clean bits"""
    name = "n5"
    c = R.CASES[name]
    N = c["N"]
    lg, ids, n, ctc = on_device(name)
    lg = lg.clone()
    lg[1, 0, 7] = float("nan")  # utterance 0, slot 1, position 0 (live for every n >= 0)
    tok, att, score, order = run(lg, ids, n, ctc, N, 0.3)
    assert torch.isnan(score[1]).item() and torch.isnan(att[1]).item() and torch.isfinite(score[:N][[0, 2, 3, 4]]).all()
    for b in range(c["B"]):
        assert sorted(order[b].tolist()) == list(range(N))
    assert order[0, N - 1].item() == 1
    cl = clean(name, 0.3)
    assert [k for k in order[0].tolist() if k != 1] == [k for k in cl[3][0].tolist() if k != 1]
    assert same_bits([t[N:] for t in (tok, att, score)] + [order[1:]], [t[N:] for t in cl[:3]] + [cl[3][1:]])


@pytest.mark.parametrize("name", ["ragged", "v5003"])
def test_an_utterance_alone_and_in_a_batch(device, name):
    c = R.CASES[name]
    N = c["N"]
    lg, ids, n, ctc = on_device(name)
    cl = clean(name, 0.3)
    for b in range(c["B"]):
        s = slice(b * N, (b + 1) * N)
        one = run(lg[s], ids[b:b + 1].contiguous(), n[b:b + 1].contiguous(), ctc[b:b + 1].contiguous(), N, 0.3)
        assert same_bits(one, [cl[0][s], cl[1][s], cl[2][s], cl[3][b:b + 1]]), (name, b)


@pytest.mark.parametrize("name, offset", [("v5000", 1), ("v5000", 2), ("bf16_4096", 1), ("bf16_4096", 4), ("v20", 3)])
def test_a_view_at_an_odd_offset_equals_its_contiguous_copy(device, name, offset):
    """a vector-sized V at an address that is not 16-byte aligned: the element-wise loads, the bits of the 16-byte ones"""
    c = R.CASES[name]
    lg, ids, n, ctc = on_device(name)
    buf = torch.zeros((lg.numel() + 16, ), dtype=lg.dtype, device=device)
    view = buf[offset:offset + lg.numel()].view(lg.shape)
    view.copy_(lg)
    assert view.data_ptr() % 16 != 0 and lg.data_ptr() % 16 == 0 and c["V"] * lg.element_size() % 16 == 0
    assert same_bits(run(view, ids, n, ctc, c["N"], 0.3), clean(name, 0.3))


def test_captured_launch_replays_the_same_bits(device):
    """the entry point allocates nothing and does not synchronise: captured in a graph and replayed twice, the outputs re-filled in
    between, it gives the clean bits"""
    from joeys2t_amd import ops
    name = "ragged"
    N = R.CASES[name]["N"]
    lg, ids, n, ctc = on_device(name)
    out = garbage_outputs(clean(name, 0.3))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.rescore(lg, ids, n, ctc, N, EOS, 0.3, out=out)  # first launch outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.rescore(lg, ids, n, ctc, N, EOS, 0.3, out=out)
    for fill in (7, 11):
        for o in out:
            o.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, clean(name, 0.3))


def test_argument_errors(device):
    """one per rule of the header: a negative return with a message, nothing launched"""
    from joeys2t_amd import ops
    from joeys2t_amd._lib import lib
    c = R.CASES["v20"]
    B, N, Lp, V = c["B"], c["N"], c["Lp"], c["V"]
    lg, ids, n, ctc = on_device("v20")
    with pytest.raises(ops.Js2tError, match="N 0 outside"):
        ops.rescore(lg, ids, n, ctc, 0, EOS, 0.3)
    wide = torch.zeros((33, Lp, V), device=device)
    with pytest.raises(ops.Js2tError, match="N 33 outside"):
        ops.rescore(wide, torch.zeros((1, 33, Lp), dtype=torch.int64, device=device), torch.zeros((33, ), dtype=torch.int32, device=device),
                    torch.zeros((33, ), device=device), 33, EOS, 0.3)
    with pytest.raises(ops.Js2tError, match="V 1 outside"):
        ops.rescore(lg[:, :, :1].contiguous(), ids, n, ctc, N, 0, 0.3)
    for eos in (-1, V):
        with pytest.raises(ops.Js2tError, match=f"eos {eos} outside"):
            ops.rescore(lg, ids, n, ctc, N, eos, 0.3)
    for w in (-0.1, 1.5, float("nan")):
        with pytest.raises(ops.Js2tError, match="ctc_weight .* outside"):
            ops.rescore(lg, ids, n, ctc, N, EOS, w)
    with pytest.raises(ops.Js2tError, match="ids_stride 3 below"):
        ops.rescore(lg, ids[:, :, :Lp - 2].contiguous(), n, ctc, N, EOS, 0.3)
    with pytest.raises(ops.Js2tError, match="no multiple"):
        ops.rescore(lg, ids, n, ctc, 3, EOS, 0.3)
    with pytest.raises(ops.Js2tError, match="dense rows"):
        ops.rescore(lg[:, :, ::2], ids, n, ctc, N, EOS, 0.3)
    with pytest.raises(ops.Js2tError, match="out ="):
        ops.rescore(lg, ids, n, ctc, N, EOS, 0.3, out=clean("v20", 0.3)[:3])
    with pytest.raises(ops.Js2tError):
        ops.rescore(lg.cpu(), ids, n, ctc, N, EOS, 0.3)
    with pytest.raises(ops.Js2tError):
        ops.rescore(lg, ids, n.long(), ctc, N, EOS, 0.3)
    outs = garbage_outputs(clean("v20", 0.3))
    ptrs = [lg, ids, n, ctc, *outs]

    def call(p, dt=0, B_=B, N_=N, Lp_=Lp, V_=V, eos=EOS, w=0.3, stride=ids.shape[2]):
        return lib().js2t_rescore(p[0], dt, p[1], stride, p[2], p[3], p[4], p[5], p[6], p[7], B_, N_, Lp_, V_, eos, w, None)

    for drop in range(len(ptrs)):
        rc = call([None if i == drop else t.data_ptr() for i, t in enumerate(ptrs)])
        assert rc < 0 and b"null pointer" in lib().js2t_last_error()
    p = [t.data_ptr() for t in ptrs]
    for kw, what in ((dict(N_=0), b"N 0 outside"), (dict(N_=33), b"N 33 outside"), (dict(Lp_=0), b"Lp 0 below"), (dict(V_=1, eos=0), b"V 1 outside"),
                     (dict(dt=7), b"bad dtype 7"), (dict(stride=Lp - 2), b"ids_stride"), (dict(w=float("nan")), b"ctc_weight")):
        assert call(p, **kw) < 0 and what in lib().js2t_last_error(), kw
    torch.cuda.synchronize()
    assert (outs[3] == 77).all() and all(torch.isnan(o).all() for o in outs[:3])  # nothing was launched
    assert call([None] * 8, B_=0) == 0


def test_worst_error_over_the_kernel_cases(device):
    """the figure DESIGN.md quotes: the worst err / tolerance over the pinned cases (runs them if run alone)"""
    for name in R.CASES:
        for w in R.WEIGHTS:
            check_case(clean(name, w), name, w)
    print("worst err / tolerance per (case, weight):", {f"{k[0]}@{k[1]}": round(float(v), 4) for k, v in WORST.items()})
    assert max(WORST.values()) <= 1.0


# ---------------------------------------------------------------- model level
MODELS = ["model_pre", "model_post", "model_deepnet"]
SETTINGS = dict(beam_size=6, n_best=4, n_rescore=4, ctc_weight=0.3)
COUNTS = {}  # model -> (utterances whose order was comparable with the oracle's, utterances whose order differs from the CTC list's)
MODEL_WORST = {}  # model -> worst |attention - oracle| / hyp_bound


@functools.lru_cache(maxsize=None)
def golden(name):
    """(model, golden arrays, the rescoring result at SETTINGS with its parts), built once per process: do not modify"""
    from joeys2t_amd.search import ctc_attention_rescore
    from test_hip_model import batch_kwargs, build
    dev = torch.device("cuda:0")
    model, g = build(name, dev)
    model.eval()
    return model, g, ctc_attention_rescore(model, batch_kwargs(g, dev), return_parts=True, **SETTINGS)


def oracle_attention(name, g, ids, n):
    """per returned row: (the attention score by the CPU oracle - its decoder on [BOS] + y with an all-true mask, a float64 log-softmax,
    the gold ids followed by EOS - and hyp_bound = the sum over the n + 1 positions of 2 (1e-4 + 1e-4 max |logit of the row|): the
    forward tolerance of test_hip_model.py on the logits, rtol = atol = 1e-4, moves the gold logit and the log-sum-exp by that each)"""
    from conftest import golden_sd
    from golden_cfg import FIXTURES, SPECIALS, oracle_cfg
    from oracle import s2t_oracle as O
    sd, cfg = golden_sd(g), oracle_cfg(FIXTURES[name]["cfg"])
    with torch.no_grad():
        enc, mask, _ = O.encoder_forward(sd, cfg, torch.from_numpy(g["src"]), torch.from_numpy(g["src_length"]))
        B = enc.shape[0]
        per = len(n) // B
        out = []
        for r in range(len(n)):
            b, y = r // per, ids[r, :n[r]].tolist()
            trg_input = torch.tensor([[SPECIALS["bos"]] + y], dtype=torch.int64)
            logits, _, _, _ = O.decoder_forward(sd, cfg, trg_input, enc[b:b + 1], mask[b:b + 1], torch.ones((1, 1, len(y) + 1), dtype=torch.bool))
            x = logits[0].double().numpy()
            lp = x - x.max(-1, keepdims=True)
            lp = lp - np.log(np.exp(lp).sum(-1, keepdims=True))
            gold = y + [SPECIALS["eos"]]
            out.append((float(sum(lp[l, gold[l]] for l in range(len(gold)))), float(sum(2 * (1e-4 + 1e-4 * np.abs(x[l]).max()) for l in range(len(gold))))))
    return out


@pytest.mark.parametrize("name", MODELS)
def test_rescore_on_a_golden_model(device, name):
    from joeys2t_amd.search import ctc_beam_search
    from test_hip_model import batch_kwargs
    model, g, (ids, scores, n, parts) = golden(name)
    K, nb, w = SETTINGS["beam_size"], SETTINGS["n_best"], SETTINGS["ctc_weight"]
    B = g["src"].shape[0]
    assert ids.dtype == np.int64 and scores.dtype == np.float32 and n.dtype == np.int64
    assert ids.shape == (B * nb, max(int(n.max()), 1)) and scores.shape == (B * nb, 1) and n.shape == (B * nb, )
    assert all((ids[r, n[r]:] == model.pad_index).all() for r in range(B * nb))
    # the CTC scores and hypotheses are ctc_beam_search's for the same settings, bit for bit
    cids, cscores, cn = ctc_beam_search(model, batch_kwargs(g, device), beam_size=K, n_best=nb)
    rank = parts["ctc_rank"]
    assert rank.shape == (B * nb, ) and all(sorted(rank[b * nb:(b + 1) * nb].tolist()) == list(range(nb)) for b in range(B))
    for r in range(B * nb):
        src = (r // nb) * nb + int(rank[r])
        assert parts["ctc"][r].view(np.int32) == cscores[src, 0].view(np.int32) and n[r] == cn[src]
        assert ids[r, :n[r]].tolist() == cids[src, :cn[src]].tolist()
    assert np.isfinite(scores).all()  # (these utterances have more than four prefixes)
    ref = oracle_attention(name, g, ids, n)
    worst = 0.0
    for r, (att_ref, hb) in enumerate(ref):
        err = abs(float(parts["attention"][r]) - att_ref)
        worst = max(worst, err / hb)
        print(f"{name} row {r}: n {n[r]} attention {parts['attention'][r]:.6f} oracle {att_ref:.6f} err / bound {err / hb:.4f}")
        assert err <= hb, (name, r, parts["attention"][r], att_ref, hb)
        comb = w * float(parts["ctc"][r]) + (1 - w) * float(parts["attention"][r])
        assert abs(float(scores[r, 0]) - comb) <= R.bound(comb)
        tl = parts["token_log_probs"][r]
        assert tl.shape == (n[r] + 1, ) and tl.dtype == np.float32
        acc = np.float32(0.0)
        for v in tl:
            acc = np.float32(acc + v)
        assert acc.view(np.int32) == parts["attention"][r].view(np.int32)  # the same f32 sum in ascending order
    MODEL_WORST[name] = worst
    comparable = differing = 0
    for b in range(B):
        rows = list(range(b * nb, (b + 1) * nb))
        assert all(scores[r, 0] >= scores[r + 1, 0] for r in rows[:-1])
        differing += rank[rows].tolist() != list(range(nb))
        comb = {r: w * float(parts["ctc"][r]) + (1 - w) * ref[r][0] for r in rows}
        want = sorted(rows, key=lambda r: -comb[r])
        if all(comb[i] - comb[j] >= 4 * (ref[i][1] + ref[j][1]) for i, j in zip(want, want[1:])):
            comparable += 1
            assert want == rows, (name, b, want, [comb[r] for r in rows])
    COUNTS[name] = (comparable, differing)
    print(f"{name}: {comparable} of {B} utterances comparable with the oracle's order, {differing} re-ordered by the attention score; "
          f"worst err / bound {worst:.4f}")


def test_model_level_counts(device):
    """the order tests above cannot pass by comparing nothing: over the nine utterances at least one is comparable with the oracle and
    at least one returned list differs in order from the CTC list (runs the models if run alone)"""
    for name in MODELS:
        if name not in COUNTS:
            test_rescore_on_a_golden_model(device, name)
    print("comparable / re-ordered per model:", COUNTS, "worst err / bound:", {k: round(v, 4) for k, v in MODEL_WORST.items()})
    assert sum(c for c, _ in COUNTS.values()) >= 1 and sum(d for _, d in COUNTS.values()) >= 1


@pytest.mark.parametrize("name", MODELS)
def test_n_best_one_is_the_first_row(device, name):
    from joeys2t_amd.search import ctc_attention_rescore
    from test_hip_model import batch_kwargs
    model, g, (ids, scores, n, _) = golden(name)
    nb = SETTINGS["n_best"]
    ids1, scores1, n1 = ctc_attention_rescore(model, batch_kwargs(g, device), **dict(SETTINGS, n_best=1))
    assert np.array_equal(n1, n[::nb]) and np.array_equal(scores1.view(np.int32), scores[::nb].view(np.int32))
    assert np.array_equal(ids1, ids[::nb, :ids1.shape[1]]) and (ids[::nb, ids1.shape[1]:] == model.pad_index).all()


@pytest.mark.parametrize("name", MODELS)
def test_predict_with_the_ctc_attention_decoder(device, name):
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search, search
    from test_hip_model import batch_kwargs
    model, g, _ = golden(name)
    K, nb = 5, 2
    want_ids, want_scores, want_n = ctc_attention_rescore(model, batch_kwargs(g, device), beam_size=K, n_best=nb, ctc_weight=0.3)
    ids, sentences, scores = predict(model, [batch_kwargs(g, device)], beam_size=K, n_best=nb, return_prob="hyp", decoder="ctc-attention",
                                     ctc_weight=0.3)
    assert len(ids) == len(sentences) == len(scores) == len(want_ids)  # predict sorts the batch by length and puts the rows back
    for r in range(len(ids)):
        assert np.asarray(ids[r])[:want_n[r]].tolist() == want_ids[r, :want_n[r]].tolist() and (np.asarray(ids[r])[want_n[r]:] == model.pad_index).all()
        assert abs(float(scores[r][0]) - want_scores[r, 0]) <= R.bound(want_scores[r, 0])
    # the two existing decoders are what they were: ctc_weight is not theirs to read
    cids, cscores, cn = ctc_beam_search(model, batch_kwargs(g, device), beam_size=K, n_best=nb)
    pids, _, pscores = predict(model, [batch_kwargs(g, device)], beam_size=K, n_best=nb, return_prob="hyp", decoder="ctc", ctc_weight=0.9)
    for r in range(len(pids)):
        assert np.asarray(pids[r])[:cn[r]].tolist() == cids[r, :cn[r]].tolist() and abs(float(pscores[r][0]) - cscores[r, 0]) <= R.bound(cscores[r, 0])
    gids, _, _ = search(model, batch_kwargs(g, device), max_output_length=12, beam_size=1, beam_alpha=-1.0, n_best=1, min_output_length=1,
                        generate_unk=True, return_prob="none", repetition_penalty=-1, no_repeat_ngram_size=-1, return_attention=False)
    aids, _, ascores = predict(model, [batch_kwargs(g, device)], max_output_length=12, ctc_weight=0.9)
    assert ascores is None and np.array_equal(np.asarray(aids), gids)
    with pytest.raises(ValueError, match="decoder.*attention.*ctc.*ctc-attention"):
        predict(model, [batch_kwargs(g, device)], decoder="rnn")


def test_bf16_compute_runs(device):
    """one bf16-compute run: finite scores, sorted rows, a permutation per utterance, the shapes of the f32 run"""
    from joeys2t_amd.search import ctc_attention_rescore
    from test_hip_model import batch_kwargs, build
    model, g = build("model_pre", device, torch.bfloat16)
    model.eval()
    nb = SETTINGS["n_best"]
    ids, scores, n, parts = ctc_attention_rescore(model, batch_kwargs(g, device), return_parts=True, **SETTINGS)
    B = g["src"].shape[0]
    assert ids.shape == (B * nb, max(int(n.max()), 1)) and scores.shape == (B * nb, 1) and n.shape == (B * nb, )
    assert np.isfinite(scores).all() and np.isfinite(parts["attention"]).all() and np.isfinite(parts["ctc"]).all()
    for b in range(B):
        assert sorted(parts["ctc_rank"][b * nb:(b + 1) * nb].tolist()) == list(range(nb))
        assert all(scores[r, 0] >= scores[r + 1, 0] for r in range(b * nb, (b + 1) * nb - 1))
    assert all(len(t) == n[r] + 1 for r, t in enumerate(parts["token_log_probs"]))


def test_a_model_without_a_ctc_layer_is_refused(device):
    from joeys2t_amd.search import ctc_attention_rescore
    from test_hip_model import batch_kwargs, build
    model, g = build("model_pre", device)
    model.loss_function = ("crossentropy", 0.1, 0.0)  # drops the CTC output layer
    model.eval()
    with pytest.raises(ValueError, match="no CTC output layer"):
        ctc_attention_rescore(model, batch_kwargs(g, device), beam_size=4)
