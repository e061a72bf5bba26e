"""GPU: CTC prefix beam search with the n-gram LM fused into the beam (js2t_ctc_beam_search_lm, ops.ctc_beam_search_lm,
search.ctc_beam_search / ctc_attention_rescore / predict with lm_fusion="search") against the float64 NumPy reference of
tests/ctc_beam_lm_reference.py (pinned on the CPU by test_ctc_beam_lm_cpu.py).

Exactness as in test_hip_ctc_beam.py: ids and lengths are compared exactly on DECIDABLE inputs (margin >= 4 tolerances at every
pruning step and between the returned final scores), the three scores within 1e-4 max(1, |ref|).  Every comparison prints err /
tolerance; the worst over the cases is printed and asserted by test_worst_error_over_the_kernel_cases.
"""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_lm_reference as F
import ctc_beam_reference as R
import ngram_reference as G

pytestmark = pytest.mark.gpu

BLANK, BOS, EOS = F.BLANK, F.BOS, F.EOS
PAD = -1
WORST = {}  # what -> worst err / tolerance seen


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def tables(device, logits, C, blank=BLANK):
    """(logits on the device, lse of ops.row_lse, cand_id, cand_lp): the inputs of the two beam searches for [B, T, V] logits"""
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
    if name == "wins":
        return NGramLM.from_ngrams(F.wins_lm(), F.WINS["V"], device="cuda:0")
    if name in G.CASES:
        return NGramLM.from_ngrams(G.case_lm(name), G.CASES[name]["V"], device="cuda:0", max_load=G.CASES[name].get("max_load", 0.5))
    return NGramLM.from_ngrams(F.case_lm(name), F.CASES[name]["V"], device="cuda:0")


def run(device, logits, in_len, K, C, n_best, lm, w, b, eos=EOS, **kw):
    from joeys2t_amd import ops
    lg, lse, cand_id, cand_lp = tables(device, logits, C)
    out = ops.ctc_beam_search_lm(lg, lse, cand_id, cand_lp, torch.as_tensor(in_len).to(device), K, n_best, BLANK, PAD, lm, BOS, eos, w, b, **kw)
    torch.cuda.synchronize()
    return out


def case_input(name, w, b):
    x = torch.from_numpy(F.case_logits(name, w, b))
    return x.to(torch.bfloat16) if F.CASES[name].get("bf16") else x


@functools.lru_cache(maxsize=None)
def clean(name, w, b):
    """the pinned case run once on the GPU and shared by the tests that compare against it: do not modify"""
    c = F.CASES[name]
    return run(torch.device("cuda:0"), case_input(name, w, b), c["in_len"], c["K"], c["C"], c["n_best"], device_lm(name), w, b)


def check_utterance(out, u, hyps, n_best, what):
    """utterance u of (ids, lengths, final, ctc, lm) against the reference's hypotheses: exact ids, lengths, pad fill, the three
    scores in tolerance; the slots without a prefix -inf / -inf / -inf, length 0, all pad"""
    ids, n, score, ctc, lms = (o[u].cpu().numpy() for o in out)
    assert ids.shape[0] == n.shape[0] == score.shape[0] == ctc.shape[0] == lms.shape[0] == n_best
    worst = 0.0
    for i in range(n_best):
        if i < len(hyps):
            y, s, c, l = hyps[i]
            errs = [abs(float(score[i]) - s) / F.bound(s), abs(float(ctc[i]) - c) / F.bound(c), abs(float(lms[i]) - l) / F.bound(l)]
            worst = max(worst, max(errs))
            print(f"{what} utterance {u} slot {i}: len {n[i]} final {score[i]:.6f} ref {s:.6f} err/tol {errs[0]:.3f}, ctc {errs[1]:.3f}, "
                  f"lm {errs[2]:.3f}")
            assert n[i] == len(y) and ids[i, :len(y)].tolist() == list(y), (what, u, i, ids[i, :n[i]].tolist(), y)
            assert (ids[i, len(y):] == PAD).all()
            assert max(errs) <= 1.0, (what, u, i, (score[i], ctc[i], lms[i]), (s, c, l))
        else:
            assert score[i] == -np.inf and ctc[i] == -np.inf and lms[i] == -np.inf and n[i] == 0 and (ids[i] == PAD).all(), (what, u, i)
    WORST[what] = max(WORST.get(what, 0.0), worst)


def check_case(name, w, b):
    c = F.CASES[name]
    out = clean(name, w, b)
    assert out[0].shape == (c["B"], c["n_best"], c["T"]) and out[0].dtype == torch.int64 and out[1].dtype == torch.int32
    assert all(o.shape == (c["B"], c["n_best"]) and o.dtype == torch.float32 for o in out[2:])
    for u, (hyps, margin) in enumerate(F.case_reference(name, w, b)):
        assert margin >= F.DECIDABLE
        check_utterance(out, u, hyps, c["n_best"], f"{name}@{w}+{b}")


# ---------------------------------------------------------------- exact comparison on decidable inputs
@pytest.mark.parametrize("name, w, b", F.PINNED)
def test_pinned_case_matches_reference(device, name, w, b):
    """f32 logits, bf16 logits on `bf16` (the reference runs on the bf16-rounded values)"""
    if F.CASES[name].get("bf16"):
        x = F.case_logits(name, w, b)
        assert np.array_equal(torch.from_numpy(x).to(torch.bfloat16).float().numpy(), x) and case_input(name, w, b).dtype == torch.bfloat16
    check_case(name, w, b)


@pytest.mark.parametrize("w, b", F.COMBOS)
def test_identity_case_is_the_sequence_rule(device, w, b):
    """the identity case is one where identity by trie node returns something else under LM keys: a prefix that is created again
    carries its twin's LM value and folds into it - the kernel's result is the sequence-keyed one"""
    assert F.differs(F.case_reference("identity_lm", w, b), F.run_case("identity_lm", w, b, identity="node"))
    check_case("identity_lm", w, b)


@pytest.mark.parametrize("K", F.WINS_K)
def test_fusion_returns_what_rescoring_cannot(device, K):
    """the kernel returns the reference's fused best; the rescore route (ops.ctc_beam_search + ops.ngram_rescore over the whole
    CTC-only beam of the same K) on the same input does not contain it, and its best score is lower"""
    from joeys2t_amd import ops
    w = F.WINS
    ok, fused, route, _ = F.wins_reference(K)
    assert ok
    x = torch.from_numpy(F.wins_logits(K))
    out = run(device, x, [w["T"]], K, w["C"], 1, device_lm("wins"), w["lm_weight"], w["length_bonus"])
    check_utterance(out, 0, fused[:1], 1, f"wins K {K}")
    lg, lse, cand_id, cand_lp = tables(device, x, w["C"])
    ids, n, ctc = ops.ctc_beam_search(lg, lse, cand_id, cand_lp, torch.as_tensor([w["T"]]).to(device), K, K, BLANK, PAD)
    _, _, score, order = ops.ngram_rescore(ids, n, ctc, K, device_lm("wins"), BOS, EOS, w["lm_weight"], w["length_bonus"])
    torch.cuda.synchronize()
    ids, n, score, order = ids[0].cpu().numpy(), n[0].cpu().numpy(), score.cpu().numpy(), order[0].cpu().numpy()
    kept = [tuple(ids[k, :n[k]].tolist()) for k in range(K)]
    assert fused[0][0] not in kept and kept[order[0]] == route[0][0]
    assert abs(float(score[order[0]]) - route[0][1]) <= F.bound(route[0][1])
    assert float(out[2][0, 0]) > float(score[order[0]]) + 2 * F.bound(route[0][1])


# ---------------------------------------------------------------- weights of zero
@pytest.mark.parametrize("name", list(R.CASES))
def test_zero_weights_and_no_lm_are_the_ctc_only_search(device, name):
    """both weights 0, NULL model pointers: ids, lengths and scores are js2t_ctc_beam_search's bits on every pinned case of
    ctc_beam_reference; out_ctc is the score and out_lm is 0 (-inf in the slots without a prefix)"""
    from joeys2t_amd import ops
    c = R.CASES[name]
    x = torch.from_numpy(R.case_logits(name))
    x = x.to(torch.bfloat16) if c.get("bf16") else x
    lg, lse, cand_id, cand_lp = tables(device, x, c["C"])
    il = torch.as_tensor(c["in_len"]).to(device)
    want = ops.ctc_beam_search(lg, lse, cand_id, cand_lp, il, c["K"], c["n_best"], BLANK, PAD)
    got = ops.ctc_beam_search_lm(lg, lse, cand_id, cand_lp, il, c["K"], c["n_best"], BLANK, PAD, None, min(BOS, c["V"] - 1), min(EOS, c["V"] - 1),
                                 0.0, 0.0)
    torch.cuda.synchronize()
    assert same_bits(got[:3], want) and same_bits(got[3:4], want[2:3])
    live = torch.isfinite(want[2])
    assert not bits(got[4][live]).any() and (got[4][~live] == -np.inf).all()


def test_bonus_alone_reads_no_model(device):
    """lm_weight 0, length_bonus 0.5: NULL model pointers and a model whose tables are poisoned give the same bits; lm is 0, final =
    ctc + 0.5 n; the reference's list (the input is decidable at these weights too)"""
    from joeys2t_amd.lm import NGramLM
    c = F.CASES["k8"]
    x = torch.from_numpy(F.case_logits("k8", 0.5, 0.5))
    none = run(device, x, c["in_len"], c["K"], c["C"], c["n_best"], None, 0.0, 0.5)
    bad = NGramLM.from_ngrams(F.case_lm("k8"), c["V"], device="cuda:0")
    bad.uni_dev.fill_(float("nan"))
    bad.table_dev.fill_(-1)
    assert same_bits(run(device, x, c["in_len"], c["K"], c["C"], c["n_best"], bad, 0.0, 0.5), none)
    ids, n, score, ctc, lms = (o.cpu().numpy() for o in none)
    assert np.isfinite(score).all() and not lms.view(np.int32).any()
    assert all(abs(float(s) - (float(a) + 0.5 * int(k))) <= F.bound(float(s)) for s, a, k in zip(score.ravel(), ctc.ravel(), n.ravel()))
    hyps, margin = F.beam_search(x[0].numpy(), c["K"], c["C"], c["n_best"], BLANK, None, c["V"], c["order"], BOS, EOS, 0.0, 0.5)
    assert margin >= F.DECIDABLE
    check_utterance(none, 0, hyps, c["n_best"], "bonus alone")


# ---------------------------------------------------------------- edges and invariants
SHORT = ("short", 0.5, 0.5)


def test_no_frames_and_clamped_length(device):
    c = F.CASES["short"]
    out = run(device, case_input(*SHORT), [c["T"] + 7, 0, 1], c["K"], c["C"], c["n_best"], device_lm("short"), 0.5, 0.5)
    ref = F.case_reference(*SHORT)
    check_utterance(out, 0, ref[0][0], c["n_best"], "clamped")  # in_len > T is T
    empty, _ = F.beam_search(np.zeros((0, c["V"])), c["K"], c["C"], c["n_best"], BLANK, F.case_lm("short"), c["V"], c["order"], BOS, EOS, 0.5, 0.5)
    assert len(empty) == 1 and empty[0][0] == () and empty[0][2] == 0.0
    check_utterance(out, 1, empty, c["n_best"], "no frames")  # the empty hypothesis with final = lm_weight * p(eos | bos), nothing else
    check_utterance(out, 2, ref[2][0], c["n_best"], "one frame")
    assert same_bits([o[0] for o in out], [o[0] for o in clean(*SHORT)]) and out[3][1, 0].item() == 0.0


def test_an_utterance_alone_and_in_a_batch(device):
    c = F.CASES["short"]
    x = case_input(*SHORT)
    for u in range(c["B"]):
        one = run(device, x[u:u + 1], c["in_len"][u:u + 1], c["K"], c["C"], c["n_best"], device_lm("short"), 0.5, 0.5)
        assert same_bits(one, [o[u:u + 1] for o in clean(*SHORT)]), u


@pytest.mark.parametrize("name, w, b", [SHORT, ("long_k2", 0.5, 0.0)])
def test_garbage_behind_the_length_in_the_workspace_and_in_ignored_slots(device, name, w, b):
    """NaN logits and lse and NaN / out-of-range candidate rows behind every utterance's length, a workspace full of 0xFF, and
    candidate slots that are ignored (the blank, an id outside the vocabulary, -inf) in between the real ones: the bits of the clean
    run (which a second clean launch repeats)"""
    from joeys2t_amd import ops
    c = F.CASES[name]
    B, T, V = c["B"], c["T"], c["V"]
    lg, lse, cand_id, cand_lp = tables(device, case_input(name, w, b), c["C"])
    il = torch.as_tensor(c["in_len"]).to(device)
    args = (il, c["K"], c["n_best"], BLANK, PAD, device_lm(name), BOS, EOS, w, b)
    again = ops.ctc_beam_search_lm(lg, lse, cand_id, cand_lp, *args)
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
    out = ops.ctc_beam_search_lm(lg, lse, cand_id, cand_lp, *args, workspace=ws)
    torch.cuda.synchronize()
    assert same_bits(again, clean(name, w, b)) and same_bits(out, clean(name, w, b))


def test_packed_rows_equal_padded(device):
    from joeys2t_amd import ops
    c = F.CASES["short"]
    B, T, V = c["B"], c["T"], c["V"]
    lg, lse, cand_id, cand_lp = tables(device, case_input(*SHORT), c["C"])
    pk = ops.PackedRows.from_lengths(list(c["in_len"]), T, device, round_to=16)
    live = (torch.arange(T)[None, :] < torch.as_tensor(c["in_len"])[:, None]).view(-1).to(device)
    n_live = int(sum(c["in_len"]))

    def packed(t, fill):
        out = torch.full((pk.rows, ) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=device)
        out[:n_live] = t[live]
        return out

    out = ops.ctc_beam_search_lm(packed(lg.view(B * T, V), 0.0), packed(lse, 0.0), packed(cand_id, 0), packed(cand_lp, 0.0),
                                 torch.as_tensor(c["in_len"]).to(device), c["K"], c["n_best"], BLANK, PAD, device_lm("short"), BOS, EOS, 0.5, 0.5,
                                 pack=pk)
    torch.cuda.synchronize()
    assert same_bits(out, clean(*SHORT))


def test_a_label_the_lm_forbids_is_never_extended(device):
    """a unigram of -inf: the label is never proposed, although the clean run's hypotheses hold it; every score stays finite"""
    from joeys2t_amd.lm import NGramLM
    c = F.CASES["short"]
    lm = dict(F.case_lm("short"))
    lm[(5, )] = (-np.inf, 0.0)
    x = F.case_logits(*SHORT)
    clean_ids, clean_n = clean(*SHORT)[0][0].cpu().numpy(), clean(*SHORT)[1][0].cpu().numpy()
    assert any(5 in clean_ids[i, :clean_n[i]] for i in range(c["n_best"]))
    out = run(device, torch.from_numpy(x), c["in_len"], c["K"], c["C"], c["n_best"], NGramLM.from_ngrams(lm, c["V"], device="cuda:0"), 0.5, 0.5)
    ids, n, score = (o.cpu().numpy() for o in out[:3])
    live = np.isfinite(score)
    assert live[:, 0].all() and (n[~live] == 0).all() and not np.isnan(score).any()
    assert all(5 not in ids[u, i, :n[u, i]] for u in range(c["B"]) for i in range(c["n_best"]))
    for u in range(c["B"]):
        hyps, margin = F.beam_search(x[u, :c["in_len"][u]], c["K"], c["C"], c["n_best"], BLANK, lm, c["V"], c["order"], BOS, EOS, 0.5, 0.5)
        assert margin >= F.DECIDABLE
        check_utterance(out, u, hyps, c["n_best"], "forbidden label")


def test_near_full_table(device):
    """ngram_reference's big_full model: V = 5000, order 4, load 0.949, chains of up to 41 slots that wrap around"""
    c = F.BIG
    lm = device_lm("big_full")
    assert lm.capacity == 16384 and lm.max_probe == 41 and lm.order == 4
    hyps, margin = F.big_reference()
    assert margin >= F.DECIDABLE
    out = run(device, torch.from_numpy(F.big_logits()), [c["T"]], c["K"], c["C"], c["n_best"], lm, c["lm_weight"], c["length_bonus"])
    check_utterance(out, 0, hyps, c["n_best"], "big_full")


def test_captured_launch_replays_the_same_bits(device):
    """the entry point allocates nothing and does not synchronise: captured in a graph and replayed twice it gives the clean bits"""
    from joeys2t_amd import ops
    c = F.CASES["short"]
    lg, lse, cand_id, cand_lp = tables(device, case_input(*SHORT), c["C"])
    il = torch.as_tensor(c["in_len"]).to(device)
    ws = torch.empty((ops.ctc_beam_workspace_bytes(c["B"], c["T"], c["K"]), ), dtype=torch.uint8, device=device)
    args = (lg, lse, cand_id, cand_lp, il, c["K"], c["n_best"], BLANK, PAD, device_lm("short"), BOS, EOS, 0.5, 0.5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ctc_beam_search_lm(*args, workspace=ws)  # first launch outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.ctc_beam_search_lm(*args, workspace=ws)
    for _ in range(2):
        for o in out:
            o.fill_(7)
        ws.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, clean(*SHORT))


def test_argument_errors(device):
    """every limit of the header: a negative return with a message, nothing launched (the outputs keep their fill)"""
    from joeys2t_amd import ops
    from joeys2t_amd._lib import lib
    name = "k16"
    c = F.CASES[name]
    B, T, V = c["B"], c["T"], c["V"]
    lm = device_lm(name)
    lg, lse, cand_id, cand_lp = tables(device, case_input(name, 0.5, 0.5), c["C"])
    il = torch.as_tensor(c["in_len"]).to(device)
    ids = torch.full((B, 1, T), 77, dtype=torch.int64, device=device)
    n = torch.full((B, 1), 77, dtype=torch.int32, device=device)
    score, ctc, lms = (torch.full((B, 1), 77.0, dtype=torch.float32, device=device) for _ in range(3))
    ws = torch.empty((ops.ctc_beam_workspace_bytes(B, T, 4), ), dtype=torch.uint8, device=device)
    good = dict(logits=lg.data_ptr(), dt=0, lse=lse.data_ptr(), cand_id=cand_id.data_ptr(), cand_lp=cand_lp.data_ptr(), in_len=il.data_ptr(),
                uni=lm.uni_dev.data_ptr(), table=lm.table_dev.data_ptr(), capacity=lm.capacity, max_probe=lm.max_probe, lm_order=lm.order,
                out_ids=ids.data_ptr(), out_len=n.data_ptr(), out_score=score.data_ptr(), out_ctc=ctc.data_ptr(), out_lm=lms.data_ptr(),
                workspace=ws.data_ptr(), B=B, T=T, V=V, beam=4, n_cand=c["C"], n_best=1, blank=BLANK, pad=PAD, bos=BOS, eos=EOS, lm_weight=0.5,
                length_bonus=0.5, row_offsets=None, stream=None)
    assert len(good) == 31

    def call(**change):
        return lib().js2t_ctc_beam_search_lm(*dict(good, **change).values())

    bad = [(dict(beam=0), b"beam 0 outside"), (dict(beam=33), b"beam 33 outside"), (dict(n_cand=0), b"0 candidates outside"),
           (dict(n_cand=9), b"9 candidates outside"), (dict(n_best=0), b"n_best 0 outside"), (dict(n_best=5), b"n_best 5 outside"),
           (dict(T=2**31 // 32), b"frames exceed"), (dict(blank=V), b"blank 37 outside"), (dict(blank=-1), b"blank -1 outside"),
           (dict(dt=7), b"bad dtype"), (dict(T=0), b"bad shape"), (dict(B=-1), b"bad shape"),
           (dict(V=1), b"V 1 outside"), (dict(V=65536), b"V 65536 outside"), (dict(bos=V), b"bos 37 outside"), (dict(bos=-1), b"bos -1 outside"),
           (dict(eos=V), b"eos 37 outside"), (dict(eos=-1), b"eos -1 outside"), (dict(lm_order=0), b"order 0 outside"),
           (dict(lm_order=5), b"order 5 outside"), (dict(capacity=48), b"capacity 48 is neither"), (dict(capacity=-4), b"capacity -4 is neither"),
           (dict(lm_weight=float("nan")), b"not finite"), (dict(lm_weight=float("inf")), b"not finite"),
           (dict(length_bonus=float("-inf")), b"not finite"), (dict(uni=None), b"null pointer (uni"), (dict(table=None), b"needs a table"),
           (dict(capacity=0), b"needs a table"), (dict(table=lm.table_dev.data_ptr() + 8), b"not 16-byte aligned"),
           (dict(max_probe=0), b"max_probe 0 outside"), (dict(max_probe=lm.capacity + 1), b"max_probe"),
           (dict(out_ctc=None), b"null pointer"), (dict(out_lm=None), b"null pointer")]
    bad += [({k: None}, b"null pointer") for k in ("logits", "lse", "cand_id", "cand_lp", "in_len", "out_ids", "out_len", "out_score", "workspace")]
    for change, msg in bad:
        rc = call(**change)
        assert rc < 0 and msg in lib().js2t_last_error(), (change, rc, lib().js2t_last_error())
    torch.cuda.synchronize()
    assert (ids == 77).all() and (n == 77).all() and all((t == 77.0).all() for t in (score, ctc, lms))
    assert call(B=0, logits=None, out_ctc=None) == 0  # B = 0 returns OK before anything is looked at
    # with lm_weight 0 the model may be missing altogether; an order-1 model needs no table
    assert call(lm_weight=0.0, uni=None, table=None, capacity=0, max_probe=0) == 0
    assert call(lm_order=1, table=None, capacity=0, max_probe=0) == 0
    assert call() == 0
    torch.cuda.synchronize()
    # the Python layer: a model on another device or over another vocabulary, a weight without a model, a short workspace
    args = (lg, lse, cand_id, cand_lp, il, 4, 1, BLANK, PAD)
    with pytest.raises(ops.Js2tError, match="lm_weight 0 expected"):
        ops.ctc_beam_search_lm(*args, None, BOS, EOS, 0.5, 0.0)
    with pytest.raises(ops.Js2tError, match="the lm is over 11 ids"):
        ops.ctc_beam_search_lm(*args, device_lm("short"), BOS, EOS, 0.5, 0.0)
    from joeys2t_amd.lm import NGramLM
    with pytest.raises(ops.Js2tError, match="lm.to"):
        ops.ctc_beam_search_lm(*args, NGramLM.from_ngrams(F.case_lm(name), V), BOS, EOS, 0.5, 0.0)
    with pytest.raises(ops.Js2tError, match="a contiguous workspace"):
        ops.ctc_beam_search_lm(*args, lm, BOS, EOS, 0.5, 0.0, workspace=torch.empty(8, dtype=torch.uint8, device=device))
    with pytest.raises(ops.Js2tError, match="beam 33 outside"):
        ops.ctc_beam_search_lm(lg, lse, cand_id, cand_lp, il, 33, 1, BLANK, PAD, lm, BOS, EOS, 0.5, 0.0)


def test_worst_error_over_the_kernel_cases(device):
    """the figure DESIGN.md quotes: the worst err / tolerance of the scores over the pinned cases (runs them if run alone)"""
    for name, w, b in F.PINNED:
        check_case(name, w, b)
    print("worst err / tolerance per case:", {k: round(float(v), 4) for k, v in WORST.items()})
    assert max(WORST.values()) <= 1.0


# ---------------------------------------------------------------- model level
MODELS = ["model_pre", "model_post", "model_deepnet"]
SET = dict(beam_size=6, n_best=4, candidates=8)
LMW, CTCW = 0.5, 0.3
COUNTS = {}  # model -> (utterances left out of the exact comparison, utterances whose best differs from the rescore route's)


@functools.lru_cache(maxsize=None)
def model_lm():
    """ngram_reference's order-3 LM over the golden models' 20 ids (its case n32), on the device"""
    return device_lm("n32")


@functools.lru_cache(maxsize=None)
def golden(name):
    """(model, golden arrays, the fused search's result, the rescore route's), built once per process: do not modify"""
    from joeys2t_amd.search import ctc_beam_search
    from test_hip_model import batch_kwargs, build
    dev = torch.device("cuda:0")
    model, g = build(name, dev)
    model.eval()
    fused = ctc_beam_search(model, batch_kwargs(g, dev), lm=model_lm(), lm_weight=LMW, lm_fusion="search", **SET)
    route = ctc_beam_search(model, batch_kwargs(g, dev), lm=model_lm(), lm_weight=LMW, **SET)
    return model, g, fused, route


def ctc_frames(model, batch):
    with torch.no_grad():
        enc, _, src_mask, _ = model(return_type="encode", **vars(batch))
        ctc_out = model.decoder.project(model.decoder.ctc_output_layer, enc, model.runtime.compute_dtype)
    return ctc_out.float().contiguous(), src_mask.squeeze(1).sum(dim=1)


@pytest.mark.parametrize("name", MODELS)
def test_fused_search_on_a_golden_model(device, name):
    """search.ctc_beam_search(lm_fusion="search") against the reference run on the device's own CTC logits: ids exact and scores in
    tolerance on the decidable utterances"""
    from test_hip_model import batch_kwargs
    model, g, fused, route = golden(name)
    assert (model.bos_index, model.eos_index) == (BOS, EOS) and len(model.trg_vocab) == 20
    nb, K, C = SET["n_best"], SET["beam_size"], SET["candidates"]
    ids, scores, n = fused
    logits, in_len = ctc_frames(model, batch_kwargs(g, device))
    B = logits.shape[0]
    assert ids.dtype == np.int64 and scores.dtype == np.float32 and n.dtype == np.int64
    assert ids.shape == (B * nb, max(int(n.max()), 1)) and scores.shape == (B * nb, 1) and n.shape == (B * nb, )
    x = logits.cpu().numpy()
    left_out = differs = 0
    worst = 0.0
    for u in range(B):
        rows = list(range(u * nb, (u + 1) * nb))
        assert all(scores[r, 0] >= scores[r + 1, 0] for r in rows[:-1])
        assert all((ids[r, n[r]:] == model.pad_index).all() for r in rows)
        differs += ids[rows[0], :n[rows[0]]].tolist() != route[0][rows[0], :route[2][rows[0]]].tolist()
        ref, margin = F.beam_search(x[u, :int(in_len[u])], K, C, nb, model.bos_index, G.case_lm("n32"), 20, 3, BOS, EOS, LMW, 0.0)
        if margin < F.DECIDABLE:
            left_out += 1
            print(f"{name} utterance {u}: margin {margin:.1f}, left out")
            continue
        assert len(ref) == nb
        for r, (y, s, _, _) in zip(rows, ref):
            err = abs(float(scores[r, 0]) - s) / F.bound(s)
            worst = max(worst, err)
            assert n[r] == len(y) and ids[r, :n[r]].tolist() == list(y), (name, u, r)
            assert err <= 1.0, (name, u, r, scores[r, 0], s)
    COUNTS[name] = (left_out, differs)
    print(f"{name}: {left_out} of {B} utterances left out, the best of {differs} differs from the rescore route's; worst err / tolerance {worst:.4f}")


def test_model_level_counts(device):
    """the comparison above cannot pass by comparing nothing: at most 3 of the 9 utterances are left out, and on at least one the
    fused search's best hypothesis is not the rescore route's (runs the models if run alone)"""
    for name in MODELS:
        if name not in COUNTS:
            test_fused_search_on_a_golden_model(device, name)
    print("left out / best differs per model:", COUNTS)
    assert sum(v[0] for v in COUNTS.values()) <= 3
    assert sum(v[1] for v in COUNTS.values()) >= 1


@pytest.mark.parametrize("name", MODELS)
def test_attention_rescoring_of_the_fused_list(device, name):
    """ctc_attention_rescore(lm_fusion="search"): the first pass is the fused kernel with n_best = n_rescore - every returned row's
    "ctc" is that kernel's out_ctc, bit for bit, at the row's "ctc_rank", its labels are that slot's, and its "lm" (js2t_ngram_rescore's
    sum) is the kernel's out_lm within the tolerance"""
    from joeys2t_amd import ops
    from joeys2t_amd.search import ctc_attention_rescore
    from test_hip_model import batch_kwargs
    model, g, _, _ = golden(name)
    nb, K, C, N = SET["n_best"], SET["beam_size"], SET["candidates"], 5
    ids, scores, n, parts = ctc_attention_rescore(model, batch_kwargs(g, device), ctc_weight=CTCW, lm=model_lm(), lm_weight=LMW, n_rescore=N,
                                                  return_parts=True, lm_fusion="search", **SET)
    logits, in_len = ctc_frames(model, batch_kwargs(g, device))
    B, T, V = logits.shape
    cand_id, cand_lp, lse = ops.ctc_beam_candidates(logits.view(B * T, V), C, model.bos_index)
    kids, kn, _, kctc, klm = (o.cpu().numpy() for o in ops.ctc_beam_search_lm(logits, lse, cand_id, cand_lp, in_len, K, N, model.bos_index,
                                                                              model.pad_index, model_lm(), BOS, EOS, LMW, 0.0))
    assert ids.shape[0] == B * nb and np.isfinite(scores).all()
    for r in range(B * nb):
        u, slot = r // nb, int(parts["ctc_rank"][r])
        assert parts["ctc"][r].view(np.int32) == kctc[u, slot].view(np.int32), (name, r)
        assert n[r] == kn[u, slot] and ids[r, :n[r]].tolist() == kids[u, slot, :n[r]].tolist()
        assert abs(float(parts["lm"][r]) - float(klm[u, slot])) <= F.bound(float(klm[u, slot]))
        want = CTCW * float(parts["ctc"][r]) + (1 - CTCW) * float(parts["attention"][r]) + LMW * float(parts["lm"][r])
        assert abs(float(scores[r, 0]) - want) <= F.bound(want)


@pytest.mark.parametrize("name", MODELS)
def test_predict_and_the_default(device, name):
    """predict(decoder="ctc", lm_fusion="search") is the search call; the default lm_fusion gives the bits of a call without the option"""
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    from test_hip_model import batch_kwargs
    model, g, fused, route = golden(name)
    K, nb = SET["beam_size"], SET["n_best"]
    ids, sentences, scores = predict(model, [batch_kwargs(g, device)], beam_size=K, n_best=nb, return_prob="hyp", decoder="ctc",
                                     lm=model_lm(), lm_weight=LMW, lm_fusion="search")
    want_ids, want_scores, want_n = fused
    assert len(ids) == len(sentences) == len(scores) == len(want_ids)  # predict sorts the batch by length and puts the rows back
    for r in range(len(ids)):
        assert np.asarray(ids[r])[:want_n[r]].tolist() == want_ids[r, :want_n[r]].tolist()
        assert (np.asarray(ids[r])[want_n[r]:] == model.pad_index).all()
        assert abs(float(scores[r][0]) - want_scores[r, 0]) <= F.bound(want_scores[r, 0])
    same = lambda a, b: all(np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x,  # noqa: E731
                                           y.view(np.int32) if y.dtype == np.float32 else y) for x, y in zip(a, b))
    assert same(ctc_beam_search(model, batch_kwargs(g, device), lm=model_lm(), lm_weight=LMW, lm_fusion="rescore", **SET), route)
    att = ctc_attention_rescore(model, batch_kwargs(g, device), ctc_weight=CTCW, lm=model_lm(), lm_weight=LMW, **SET)
    assert same(ctc_attention_rescore(model, batch_kwargs(g, device), ctc_weight=CTCW, lm=model_lm(), lm_weight=LMW, lm_fusion="rescore", **SET), att)
    ids2, _, scores2 = predict(model, [batch_kwargs(g, device)], beam_size=K, n_best=nb, return_prob="hyp", decoder="ctc-attention",
                               ctc_weight=CTCW, lm=model_lm(), lm_weight=LMW, lm_fusion="search")
    want2 = ctc_attention_rescore(model, batch_kwargs(g, device), beam_size=K, n_best=nb, ctc_weight=CTCW, lm=model_lm(), lm_weight=LMW,
                                  lm_fusion="search")
    assert all(np.asarray(ids2[r])[:want2[2][r]].tolist() == want2[0][r, :want2[2][r]].tolist() for r in range(len(ids2)))
    assert all(abs(float(scores2[r][0]) - want2[1][r, 0]) <= F.bound(want2[1][r, 0]) for r in range(len(ids2)))


def test_refusals(device):
    from joeys2t_amd.prediction import predict
    from joeys2t_amd.search import ctc_attention_rescore, ctc_beam_search
    from test_hip_model import batch_kwargs
    model, g, _, _ = golden("model_pre")
    kw = dict(lm=model_lm(), lm_weight=LMW)
    with pytest.raises(ValueError, match="n_rescore with lm_fusion"):
        ctc_beam_search(model, batch_kwargs(g, device), n_rescore=4, lm_fusion="search", **kw, **SET)
    with pytest.raises(ValueError, match="without an lm or a length_bonus"):
        ctc_beam_search(model, batch_kwargs(g, device), lm_fusion="search", **SET)
    with pytest.raises(ValueError, match="without an lm or a length_bonus"):
        ctc_attention_rescore(model, batch_kwargs(g, device), lm_fusion="search", **SET)
    with pytest.raises(ValueError, match="neither 'rescore' nor 'search'"):
        ctc_beam_search(model, batch_kwargs(g, device), lm_fusion="both", **kw, **SET)
    with pytest.raises(ValueError, match="neither 'rescore' nor 'search'"):
        ctc_attention_rescore(model, batch_kwargs(g, device), lm_fusion="both", **kw, **SET)
    with pytest.raises(ValueError, match="decoder='attention' has none"):
        predict(model, [batch_kwargs(g, device)], decoder="attention", lm_fusion="search")
    with pytest.raises(ValueError, match="without an lm or a length_bonus"):
        predict(model, [batch_kwargs(g, device)], decoder="ctc", beam_size=4, lm_fusion="search")
    # the bonus alone is enough for the fused search
    ids, scores, n = ctc_beam_search(model, batch_kwargs(g, device), length_bonus=0.5, lm_fusion="search", **SET)
    assert np.isfinite(scores[::SET["n_best"]]).all()
