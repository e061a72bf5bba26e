"""GPU: CTC prefix beam search (js2t_ctc_beam_search, ops.ctc_beam_search, search.ctc_beam_search, predict(decoder="ctc")) against
the float64 NumPy reference of tests/ctc_beam_reference.py (pinned on the CPU by test_ctc_beam_cpu.py).

Exactness.  An f32 kernel and an f64 reference may prune differently where two scores nearly tie, so ids are compared exactly only
on DECIDABLE inputs (margin >= 4 tolerances at every pruning step and between the returned scores; the reference module states the
rule, test_ctc_beam_cpu.py::test_pinned_cases_are_decidable checks every pinned case).  There: ids and lengths equal, pad fill,
|score - ref| <= 1e-4 max(1, |ref|) - the project's budget for accumulated log-likelihoods (tests/test_hip_ctc_align.py).  Every
comparison prints err / tolerance; the worst over the cases is printed by the last kernel-level test.
"""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_reference as R

pytestmark = pytest.mark.gpu

BLANK = R.BLANK
PAD = -1
WORST = {}  # test name -> worst err / tolerance seen


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def tables(device, logits, C, blank=BLANK):
    """(logits on the device, lse of ops.row_lse, cand_id, cand_lp): the inputs of ops.ctc_beam_search for [B, T, V] logits"""
    from joeys2t_amd import ops
    lg = torch.as_tensor(logits).to(device).contiguous()
    V = lg.shape[-1]
    lse, _ = ops.row_lse(lg.view(-1, V))
    cand_id, cand_lp, _ = ops.ctc_beam_candidates(lg.float().view(-1, V), C, blank)
    return lg, lse, cand_id, cand_lp


def run(device, logits, in_len, K, C, n_best, blank=BLANK, **kw):
    from joeys2t_amd import ops
    lg, lse, cand_id, cand_lp = tables(device, logits, C, blank)
    out = ops.ctc_beam_search(lg, lse, cand_id, cand_lp, torch.as_tensor(in_len).to(device), K, n_best, blank, PAD, **kw)
    torch.cuda.synchronize()
    return out


def check_utterance(out, b, hyps, n_best, what):
    """utterance b of (ids, lengths, scores) against the reference's hypotheses: exact ids, lengths, pad fill, scores in tolerance"""
    ids, n, score = (o[b].cpu().numpy() for o in out)
    assert ids.shape[0] == n.shape[0] == score.shape[0] == n_best
    worst = 0.0
    for i in range(n_best):
        if i < len(hyps):
            y, s = hyps[i]
            err = abs(float(score[i]) - s) / R.bound(s)
            worst = max(worst, err)
            print(f"{what} utterance {b} slot {i}: len {n[i]} score {score[i]:.6f} ref {s:.6f} err/tol {err:.3f}")
            assert n[i] == len(y) and ids[i, :len(y)].tolist() == list(y), (what, b, i, ids[i, :n[i]].tolist(), y)
            assert (ids[i, len(y):] == PAD).all()
            assert err <= 1.0, (what, b, i, score[i], s)
        else:
            assert score[i] == -np.inf and n[i] == 0 and (ids[i] == PAD).all(), (what, b, i)
    WORST[what] = max(WORST.get(what, 0.0), worst)


@functools.lru_cache(maxsize=None)
def clean(name):
    """the pinned case run once on the GPU and shared by the tests that compare against it: do not modify"""
    c = R.CASES[name]
    x = torch.from_numpy(R.case_logits(name))
    return run(torch.device("cuda:0"), x.to(torch.bfloat16) if c.get("bf16") else x, c["in_len"], c["K"], c["C"], c["n_best"])


# ---------------------------------------------------------------- exact comparison on decidable inputs
@pytest.mark.parametrize("name", ["short", "k8", "k16", "k32", "long_k2", "long_k1", "identity"])
def test_pinned_case_matches_reference(device, name):
    c = R.CASES[name]
    out = clean(name)
    assert out[0].shape == (c["B"], c["n_best"], c["T"]) and out[0].dtype == torch.int64 and out[1].dtype == torch.int32
    for b, (hyps, margin) in enumerate(R.case_reference(name)):
        assert margin >= R.DECIDABLE
        check_utterance(out, b, hyps, c["n_best"], name)


def test_identity_case_is_the_sequence_rule(device):
    """the pinned identity case is one where identity by trie node returns something else (test_ctc_beam_cpu.py): the kernel's
    result is the sequence-keyed one"""
    assert R.differs(R.case_reference("identity"), R.run_case("identity", identity="node"))
    check_utterance(clean("identity"), 0, R.case_reference("identity")[0][0], R.CASES["identity"]["n_best"], "identity")


def test_bf16_logits(device):
    """bf16 logits against the reference on the bf16-rounded values (the candidates come from the same values as f32)"""
    c = R.CASES["bf16"]
    x = R.case_logits("bf16")
    assert np.array_equal(torch.from_numpy(x).to(torch.bfloat16).float().numpy(), x)
    for b, (hyps, _) in enumerate(R.case_reference("bf16")):
        check_utterance(clean("bf16"), b, hyps, c["n_best"], "bf16")


def test_enumeration_on_the_device(device):
    """T = 4, V = 3, K = 32, C = 2, n_best = 32: at most 31 prefixes exist, nothing is pruned, so the whole list is the brute
    force's; the unused slots are -inf / 0 / pad; and every score is -nll of ops.ctc_alpha for that labelling"""
    from joeys2t_amd import ops
    T, V, K, C = 4, 3, 32, 2
    x = R.random_logits(5, 1, T, V, scale=1.5)
    want = R.brute_force(x[0], C, BLANK)
    ids, n, score = (o[0].cpu().numpy() for o in run(device, torch.from_numpy(x), [T], K, C, K))
    got = {}
    worst = 0.0
    for i in range(K):
        if i < len(want):
            y = tuple(ids[i, :n[i]].tolist())
            assert y not in got and (ids[i, n[i]:] == PAD).all()
            got[y] = float(score[i])
        else:
            assert score[i] == -np.inf and n[i] == 0 and (ids[i] == PAD).all()
    assert set(got) == set(want) and len(want) <= 31
    assert all(score[i] >= score[i + 1] for i in range(len(want) - 1))
    hyp = sorted(got)
    Lmax = max(len(y) for y in hyp)
    tg = torch.tensor([list(y) + [1] * (Lmax - len(y)) for y in hyp], dtype=torch.int64, device=device)
    tl = torch.tensor([len(y) for y in hyp], dtype=torch.int64, device=device)
    lg = torch.from_numpy(x).to(device).expand(len(hyp), T, V).contiguous()
    lse, _ = ops.row_lse(lg.view(-1, V))
    _, nll, _, _ = ops.ctc_alpha(lg, lse, tg, torch.full((len(hyp), ), T, dtype=torch.int64, device=device), tl, BLANK, False)
    nll = nll.cpu().numpy()
    for y, v in zip(hyp, nll):
        worst = max(worst, abs(got[y] - want[y]) / R.bound(want[y]))
        assert abs(got[y] - want[y]) <= R.bound(want[y]), (y, got[y], want[y])
        assert abs(got[y] + float(v)) <= R.bound(float(v)), (y, got[y], -float(v))  # C = V - 1: nothing is truncated
    WORST["enumeration"] = worst


def test_known_answer(device):
    """two frames of blank 0.6 / a 0.4: the best path is all blank (0.36), the best labelling is `a` (0.64)"""
    x = torch.log(torch.tensor([[[0.6, 0.4], [0.6, 0.4]]]))
    ids, n, score = (o[0].cpu().numpy() for o in run(device, x, [2], 2, 1, 2))
    assert n.tolist() == [1, 0] and ids.tolist() == [[1, PAD], [PAD, PAD]]
    assert abs(score[0] - np.log(0.64)) <= 1e-4 and abs(score[1] - np.log(0.36)) <= 1e-4
    WORST["known answer"] = max(abs(score[0] - np.log(0.64)), abs(score[1] - np.log(0.36))) / 1e-4


# ---------------------------------------------------------------- edges and invariants
def test_no_frames_and_clamped_length(device):
    c = R.CASES["short"]
    x = torch.from_numpy(R.case_logits("short"))
    out = run(device, x, [c["T"] + 7, 0, 1], c["K"], c["C"], c["n_best"])
    ref = R.case_reference("short")
    check_utterance(out, 0, ref[0][0], c["n_best"], "clamped")  # in_len > T is T
    check_utterance(out, 1, [((), 0.0)], c["n_best"], "no frames")  # the empty hypothesis with score 0, nothing else
    check_utterance(out, 2, ref[2][0], c["n_best"], "one frame")
    assert same_bits([o[0] for o in out], [o[0] for o in clean("short")]) and out[2][1, 0].item() == 0.0


def test_garbage_behind_the_length_and_in_the_workspace(device):
    """NaN logits and lse, NaN / out-of-range candidate rows behind every utterance's length, a workspace full of 0xFF: the bits of
    the clean run (which a second clean launch repeats)"""
    from joeys2t_amd import ops
    c = R.CASES["short"]
    B, T, V = c["B"], c["T"], c["V"]
    lg, lse, cand_id, cand_lp = tables(device, R.case_logits("short"), c["C"])
    il = torch.as_tensor(c["in_len"]).to(device)
    again = ops.ctc_beam_search(lg, lse, cand_id, cand_lp, il, c["K"], c["n_best"], BLANK, PAD)
    dead = (torch.arange(T)[None, :] >= torch.as_tensor(c["in_len"])[:, None]).to(device)
    lg, lse, cand_id, cand_lp = lg.clone(), lse.clone(), cand_id.clone(), cand_lp.clone()
    lg[dead] = float("nan")
    lse[dead.view(-1)] = float("nan")
    cand_lp[dead.view(-1)] = float("nan")
    cand_id[dead.view(-1)] = 2**40 + 5
    ws = torch.full((ops.ctc_beam_workspace_bytes(B, T, c["K"]) + 64, ), 0xFF, dtype=torch.uint8, device=device)
    out = ops.ctc_beam_search(lg, lse, cand_id, cand_lp, il, c["K"], c["n_best"], BLANK, PAD, workspace=ws)
    torch.cuda.synchronize()
    assert same_bits(again, clean("short")) and same_bits(out, clean("short"))


def test_ignored_candidates(device):
    """a candidate slot that holds the blank, an id outside the vocabulary or -inf is ignored: the search over the remaining slots"""
    from joeys2t_amd import ops
    c = R.CASES["k8"]
    lg, lse, cand_id, cand_lp = tables(device, R.case_logits("k8"), 4)
    il = torch.as_tensor(c["in_len"]).to(device)
    want = ops.ctc_beam_search(lg, lse, cand_id, cand_lp, il, c["K"], c["n_best"], BLANK, PAD)
    rows = cand_id.shape[0]
    wide_id = torch.cat([torch.full((rows, 1), BLANK, device=device), cand_id[:, :2], torch.full((rows, 1), c["V"], device=device),
                         cand_id[:, 2:], torch.full((rows, 1), 5, device=device)], dim=1).contiguous()
    ninf = torch.full((rows, 1), float("-inf"), device=device)
    wide_lp = torch.cat([torch.zeros((rows, 1), device=device), cand_lp[:, :2], torch.zeros((rows, 1), device=device), cand_lp[:, 2:], ninf],
                        dim=1).contiguous()
    out = ops.ctc_beam_search(lg, lse, wide_id, wide_lp, il, c["K"], c["n_best"], BLANK, PAD)
    torch.cuda.synchronize()
    assert same_bits(out, want)


def test_an_utterance_alone_and_in_a_batch(device):
    c = R.CASES["short"]
    x = torch.from_numpy(R.case_logits("short"))
    for b in range(c["B"]):
        one = run(device, x[b:b + 1], c["in_len"][b:b + 1], c["K"], c["C"], c["n_best"])
        assert same_bits(one, [o[b:b + 1] for o in clean("short")]), b


def test_packed_rows_equal_padded(device):
    from joeys2t_amd import ops
    c = R.CASES["short"]
    B, T, V = c["B"], c["T"], c["V"]
    lg, lse, cand_id, cand_lp = tables(device, R.case_logits("short"), c["C"])
    pk = ops.PackedRows.from_lengths(list(c["in_len"]), T, device, round_to=16)
    live = (torch.arange(T)[None, :] < torch.as_tensor(c["in_len"])[:, None]).view(-1).to(device)
    n_live = int(sum(c["in_len"]))

    def packed(t, fill):
        out = torch.full((pk.rows, ) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=device)
        out[:n_live] = t[live]
        return out

    out = ops.ctc_beam_search(packed(lg.view(B * T, V), 0.0), packed(lse, 0.0), packed(cand_id, 0), packed(cand_lp, 0.0),
                              torch.as_tensor(c["in_len"]).to(device), c["K"], c["n_best"], BLANK, PAD, pack=pk)
    torch.cuda.synchronize()
    assert same_bits(out, clean("short"))


def test_captured_launch_replays_the_same_bits(device):
    """the entry point allocates nothing and does not synchronise: captured in a graph and replayed twice it gives the clean bits"""
    from joeys2t_amd import ops
    c = R.CASES["short"]
    lg, lse, cand_id, cand_lp = tables(device, R.case_logits("short"), c["C"])
    il = torch.as_tensor(c["in_len"]).to(device)
    ws = torch.empty((ops.ctc_beam_workspace_bytes(c["B"], c["T"], c["K"]), ), dtype=torch.uint8, device=device)
    args = (lg, lse, cand_id, cand_lp, il, c["K"], c["n_best"], BLANK, PAD)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ctc_beam_search(*args, workspace=ws)  # first launch outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.ctc_beam_search(*args, workspace=ws)
    for _ in range(2):
        for o in out:
            o.fill_(7)
        ws.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, clean("short"))


def test_argument_errors(device):
    """beam 0 and 33, 9 candidates, n_best > beam, a null pointer, a CPU tensor: a negative return with a message, nothing launched"""
    from joeys2t_amd import ops
    from joeys2t_amd._lib import lib
    c = R.CASES["short"]
    B, T, V = c["B"], c["T"], c["V"]
    lg, lse, cand_id, cand_lp = tables(device, R.case_logits("short"), c["C"])
    il = torch.as_tensor(c["in_len"]).to(device)
    for K, n_best, what in ((0, 1, "beam 0 outside"), (33, 1, "beam 33 outside"), (4, 5, "n_best 5 outside")):
        with pytest.raises(ops.Js2tError, match=what):
            ops.ctc_beam_search(lg, lse, cand_id, cand_lp, il, K, n_best, BLANK, PAD)
    wide = torch.zeros((B * T, 9), device=device)
    with pytest.raises(ops.Js2tError, match="9 candidates outside"):
        ops.ctc_beam_search(lg, lse, wide.long(), wide, il, 4, 1, BLANK, PAD)
    with pytest.raises(ops.Js2tError, match="blank 11 outside"):
        ops.ctc_beam_search(lg, lse, cand_id, cand_lp, il, 4, 1, V, PAD)
    with pytest.raises(ops.Js2tError, match="a contiguous workspace"):
        ops.ctc_beam_search(lg, lse, cand_id, cand_lp, il, 4, 1, BLANK, PAD, workspace=torch.empty(8, dtype=torch.uint8, device=device))
    with pytest.raises(ops.Js2tError):
        ops.ctc_beam_search(lg.cpu(), lse, cand_id, cand_lp, il, 4, 1, BLANK, PAD)
    with pytest.raises(ops.Js2tError, match="labels"):
        ops.ctc_beam_candidates(lg.view(-1, V)[:, :3].contiguous(), 3, BLANK)
    ids = torch.empty((B, 1, T), dtype=torch.int64, device=device)
    n = torch.empty((B, 1), dtype=torch.int32, device=device)
    score = torch.empty((B, 1), dtype=torch.float32, device=device)
    ws = torch.empty((ops.ctc_beam_workspace_bytes(B, T, 4), ), dtype=torch.uint8, device=device)
    ptrs = [lg, lse, cand_id, cand_lp, il, ids, n, score, ws]
    for drop in range(len(ptrs)):
        p = [None if i == drop else t.data_ptr() for i, t in enumerate(ptrs)]
        rc = lib().js2t_ctc_beam_search(p[0], 0, p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], B, T, V, 4, c["C"], 1, BLANK, PAD, None, None)
        assert rc < 0 and b"null pointer" in lib().js2t_last_error()
    p = [t.data_ptr() for t in ptrs]
    rc = lib().js2t_ctc_beam_search(p[0], 0, p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], B, T, V, 4, c["C"], 0, BLANK, PAD, None, None)
    assert rc < 0 and b"n_best 0 outside" in lib().js2t_last_error()
    assert ops.ctc_beam_workspace_bytes(B, T, 4) == B * (1 + 4 * T) * 8
    assert lib().js2t_ctc_beam_search(None, 0, None, None, None, None, None, None, None, None, 0, T, V, 4, 3, 1, BLANK, PAD, None, None) == 0


def test_worst_error_over_the_kernel_cases(device):
    """the figure DESIGN.md quotes: the worst err / tolerance of the scores over the exact cases above (runs them if run alone)"""
    for name in ("short", "k8", "k16", "k32", "long_k2", "long_k1", "identity", "bf16"):
        c = R.CASES[name]
        for b, (hyps, _) in enumerate(R.case_reference(name)):
            check_utterance(clean(name), b, hyps, c["n_best"], name)
    print("worst err / tolerance per case:", {k: round(float(v), 4) for k, v in WORST.items()})
    assert max(WORST.values()) <= 1.0


# ---------------------------------------------------------------- model level
@pytest.fixture(scope="module", params=["model_pre", "model_post", "model_deepnet"])
def golden_model(request, device):
    from test_hip_model import build
    model, g = build(request.param, device)
    model.eval()
    return model, g


def ctc_frames(model, batch):
    with torch.no_grad():
        enc, _, src_mask, _ = model(return_type="encode", **vars(batch))
        ctc_out = model.decoder.project(model.decoder.ctc_output_layer, enc, model.runtime.compute_dtype)
    return ctc_out.float(), src_mask.squeeze(1).sum(dim=1)


def check_model_result(model, batch, ids, scores, n, K, n_best, C):
    """shapes, hypotheses distinct and sorted, every score <= -nll of ops.ctc_alpha for its labelling (the truncated distribution
    can only lose mass), equality with the reference where the utterance's margin allows it; returns how many it did"""
    from joeys2t_amd import ops
    logits, in_len = ctc_frames(model, batch)
    B, T, V = logits.shape
    assert ids.shape[0] == B * n_best and scores.shape == (B * n_best, 1) and n.shape == (B * n_best, ) and ids.shape[1] == max(n.max(), 1)
    x = logits.cpu().numpy()
    decided = 0
    for b in range(B):
        rows = range(b * n_best, (b + 1) * n_best)
        live = [r for r in rows if np.isfinite(scores[r, 0])]
        hyps = [tuple(ids[r, :n[r]].tolist()) for r in live]
        assert len(set(hyps)) == len(hyps) and len(hyps) >= 1
        assert all(scores[r, 0] >= scores[r + 1, 0] for r in list(rows)[:-1])
        assert all((ids[r, n[r]:] == model.pad_index).all() for r in rows) and all(model.bos_index not in y for y in hyps)
        Lmax = max(max(len(y) for y in hyps), 1)
        tg = torch.tensor([list(y) + [model.pad_index] * (Lmax - len(y)) for y in hyps], dtype=torch.int64, device=logits.device)
        tl = torch.tensor([len(y) for y in hyps], dtype=torch.int64, device=logits.device)
        lg = logits[b:b + 1].expand(len(hyps), T, V).contiguous()
        lse, _ = ops.row_lse(lg.view(-1, V))
        _, nll, _, _ = ops.ctc_alpha(lg, lse, tg, in_len[b:b + 1].expand(len(hyps)).contiguous().long(), tl, model.bos_index, False)
        for r, v in zip(live, nll.cpu().numpy()):
            assert scores[r, 0] <= -float(v) + R.bound(float(v)), (b, r, scores[r, 0], -float(v))
        ref, margin = R.beam_search(x[b, :int(in_len[b])], K, C, n_best, model.bos_index)
        if margin >= R.DECIDABLE:
            decided += 1
            assert hyps == [y for y, _ in ref[:len(hyps)]] and len(hyps) == len(ref)
            assert all(abs(scores[r, 0] - s) <= R.bound(s) for r, (_, s) in zip(live, ref))
    return decided


def test_search_ctc_beam_search_on_a_golden_model(device, golden_model):
    from joeys2t_amd import alignment
    from joeys2t_amd.search import ctc_beam_search
    from test_hip_model import batch_kwargs
    model, g = golden_model
    batch = batch_kwargs(g, device)
    K, n_best, C = 6, 3, 8
    ids, scores, n = ctc_beam_search(model, batch, beam_size=K, n_best=n_best, candidates=C)
    assert ids.dtype == np.int64 and scores.dtype == np.float32
    decided = check_model_result(model, batch, ids, scores, n, K, n_best, C)
    print(f"{decided} of {batch.nseqs} utterances decidable (random-initialised model)")
    als = alignment.align_hypotheses(model, batch_kwargs(g, device), ids[::n_best])  # the best hypothesis of every utterance
    assert len(als) == batch.nseqs
    cut = alignment.hypothesis_lengths(ids[::n_best], model.eos_index, model.pad_index)  # (a random model's labels include pad / EOS)
    for b, a in enumerate(als):
        assert cut[b] <= n[b * n_best] and a.tokens == ids[b * n_best, :cut[b]].tolist() and np.isfinite(a.score)
    one_id, one_score, one_n = ctc_beam_search(model, batch_kwargs(g, device), beam_size=1, n_best=1, candidates=1)
    assert one_id.shape[0] == batch.nseqs and np.isfinite(one_score).all()
    with pytest.raises(ValueError, match="n_best"):
        ctc_beam_search(model, batch, beam_size=2, n_best=3)


def test_predict_with_the_ctc_decoder(device, golden_model):
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import ctc_beam_search
    from test_hip_model import batch_kwargs
    model, g = golden_model
    K, n_best = 5, 2
    want_ids, want_scores, want_n = ctc_beam_search(model, batch_kwargs(g, device), beam_size=K, n_best=n_best)
    ids, sentences, scores = predict(model, [batch_kwargs(g, device)], beam_size=K, n_best=n_best, return_prob="hyp", decoder="ctc")
    assert len(ids) == len(sentences) == len(scores) == len(want_ids)  # predict sorts the batch by length and puts the rows back
    for r in range(len(ids)):
        assert np.asarray(ids[r])[:want_n[r]].tolist() == want_ids[r, :want_n[r]].tolist() and (np.asarray(ids[r])[want_n[r]:] == model.pad_index).all()
        assert abs(float(scores[r][0]) - want_scores[r, 0]) <= R.bound(want_scores[r, 0])
    ids1, _, scores1 = predict(model, [batch_kwargs(g, device)], beam_size=1, decoder="ctc")
    assert len(ids1) == len(want_ids) // n_best and scores1 is None
    with pytest.raises(ValueError, match="decoder"):
        predict(model, [batch_kwargs(g, device)], decoder="rnn")
