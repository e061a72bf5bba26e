"""GPU: CTC forced alignment (js2t_ctc_align, ops.ctc_align, joeys2t_amd.alignment) against the float64 NumPy reference of
tests/ctc_align_reference.py (pinned on the CPU by test_ctc_align_cpu.py).

Bounds.  Path identity with the reference is required only where the input fixes the path (known answer, planted paths): on random
inputs two paths may differ by less than f32 resolves.  What is tested there, per utterance:
  * the path's structure (start, end, steps, skips only where allowed, collapse == target) and the agreement of tok_start / tok_end /
    frame_logp with the path;
  * |score - opt| <= 1e-4 max(1, |opt|) and |f64 score of the GPU's path - opt| <= the same, opt = the reference's optimum (the
    project's budget for accumulated log-likelihoods, loss.hip);
  * score <= -nll + 1e-4 max(1, |nll|), nll from ops.ctc_alpha on the same inputs: the best path cannot beat the sum over paths.
frame_logp against the float64 log-softmax: lse comes from js2t_row_lse (hardware exp / log: relative error of the sum <= 3e-7, so
3e-7 absolute on the logarithm), is rounded once at |lse| < 32 (2e-6) and subtracted with one more rounding at |lp| < 64 (4e-6):
1e-5 absolute covers the three.
"""
import functools

import numpy as np
import pytest
import torch

import ctc_align_reference as R

pytestmark = pytest.mark.gpu

BLANK = 0
FRAME_LOGP_ATOL = 1e-5


def bound(opt):
    return 1e-4 * max(1.0, abs(opt))


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def targets_without_repeats(rs, L, V):
    t = rs.randint(1, V, size=L)
    for i in range(1, L):
        while t[i] == t[i - 1]:
            t[i] = rs.randint(1, V)
    return t


def run(device, logits, targets, in_len, tgt_len, blank=BLANK, **kw):
    """(path, tok_start, tok_end, frame_logp, score) device tensors + nll of ops.ctc_alpha on the same inputs"""
    from joeys2t_amd import ops
    lg, tg = logits.to(device).contiguous(), torch.as_tensor(targets).to(device).contiguous()
    il, tl = torch.as_tensor(in_len).to(device), torch.as_tensor(tgt_len).to(device)
    lse, _ = ops.row_lse(lg.view(-1, lg.shape[-1]))
    out = ops.ctc_align(lg, lse, tg, il, tl, blank, **kw)
    _, nll, _, _ = ops.ctc_alpha(lg, lse, tg, il, tl, blank, False)
    torch.cuda.synchronize()
    return out, nll.cpu().numpy()


def check_utterance(out, b, logp64, target, Tb, nll, blank=BLANK, want_path=None):
    """every per-utterance check of the module docstring; logp64: float64 log-softmax [T, V] of the utterance's logits"""
    path, ts, te, fl, score = (o[b].cpu().numpy() for o in out)
    L = len(target)
    ref = R.align(logp64[:max(Tb, 0)], target, blank)
    if ref["path"] is None:
        assert score == -np.inf and (path == -1).all() and (ts == -1).all() and (te == -1).all() and (fl == 0).all(), b
        return
    p = path[:Tb]
    R.check_path(p, target, blank)
    assert (path[Tb:] == -1).all() and (fl[Tb:] == 0).all() and (ts[L:] == -1).all() and (te[L:] == -1).all(), b
    s_ref, e_ref = R.spans(p, L)
    assert np.array_equal(ts[:L], s_ref) and np.array_equal(te[:L], e_ref), b
    em = R.emissions(logp64[:Tb], R.extended(target, blank))
    assert np.abs(fl[:Tb] - em[np.arange(Tb), p]).max() <= FRAME_LOGP_ATOL, b
    opt = float(ref["score"])
    own = R.path_score(logp64[:Tb], target, blank, p)
    print(f"utterance {b}: T {Tb} L {L} score {score:.6f} opt {opt:.6f} f64 score of the path {own:.6f} -nll {-nll[b]:.6f} "
          f"same path {np.array_equal(p, ref['path'])}")
    assert abs(float(score) - opt) <= bound(opt), (b, score, opt)
    assert abs(own - opt) <= bound(opt), (b, own, opt)
    assert float(score) <= -float(nll[b]) + bound(float(nll[b])), (b, score, nll[b])
    if want_path is not None:
        assert np.array_equal(p, want_path), b


def check_batch(out, nll, logits, targets, in_len, tgt_len, want_paths=None):
    logits = logits.float().numpy().astype(np.float64)
    for b in range(logits.shape[0]):
        Tb, L = int(in_len[b]), int(tgt_len[b])
        check_utterance(out, b, R.log_softmax(logits[b]), [int(v) for v in np.asarray(targets)[b, :L]], Tb, nll,
                        want_path=None if want_paths is None else want_paths[b])


# ---------------------------------------------------------------- case A: chunking and short lengths
@functools.lru_cache(maxsize=None)
def case_a(V=37):
    """in_len: two full emission chunks of 32 plus a tail, both sides of a chunk edge, one frame, five; tgt_len: the longest the shape
    allows, none at all, and a doubled label in the last target"""
    rs = np.random.RandomState(5)
    B, T, Lmax = 6, 70, 12
    logits = torch.from_numpy((rs.randn(B, T, V) * 3.0).astype(np.float32))
    targets = np.stack([targets_without_repeats(rs, Lmax, V) for _ in range(B)])
    targets[5, :2] = 9
    in_len = np.array([70, 33, 32, 1, 64, 5])
    tgt_len = np.array([12, 7, 1, 0, 12, 2])
    return logits, targets, in_len, tgt_len


@functools.lru_cache(maxsize=None)
def clean_a(dtype, V=37):
    logits, targets, in_len, tgt_len = case_a(V)
    return run(torch.device("cuda:0"), logits.to(dtype), targets, in_len, tgt_len)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_chunking_and_short_lengths(device, dtype):
    logits, targets, in_len, tgt_len = case_a()
    out, nll = clean_a(dtype)
    check_batch(out, nll, logits.to(dtype), targets, in_len, tgt_len)  # (the reference reads the bf16 values upcast)
    assert torch.isfinite(out[4]).all()


# ---------------------------------------------------------------- case B: both kernel forms, both homes of the back-pointers
def test_both_kernel_forms(device):
    """S = 191, 193, 201.  The form is chosen per launch from Lmax, as js2t_ctc_alpha chooses: the batch (Lmax = 100) runs the block
    form, its first utterance alone with Lmax = 95 the one-wave form at its last size - and the two forms give the same bits."""
    rs = np.random.RandomState(11)
    B, T, V = 3, 210, 50
    tgt_len = np.array([95, 96, 100])
    in_len = np.array([210, 207, 210])
    logits = torch.from_numpy((rs.randn(B, T, V) * 3.0).astype(np.float32))
    targets = rs.randint(1, V, size=(B, 100))
    out, nll = run(device, logits, targets, in_len, tgt_len)
    check_batch(out, nll, logits, targets, in_len, tgt_len)
    one, nll1 = run(device, logits[:1], targets[:1, :95], in_len[:1], tgt_len[:1])
    check_batch(one, nll1, logits[:1], targets[:1, :95], in_len[:1], tgt_len[:1])
    assert same_bits([out[0][:1], out[1][:1, :95], out[2][:1, :95], out[3][:1], out[4][:1]], one)


def test_back_pointers_in_lds_and_in_the_workspace(device):
    """The back-pointers of an utterance take ceil(T_b / 16) * S words; the kernel keeps them in LDS up to 88 KB = 22528 words and in
    the workspace beyond: T = 512 is 32 word rows, so S = 703 (22496 words) is the last size in LDS, S = 705 the first in the workspace,
    S = 1023 the largest there is.  The workspace is handed over full of ones (an unwritten word would read as back-pointer 3)."""
    from joeys2t_amd import ops
    rs = np.random.RandomState(12)
    B, T, V = 3, 512, 50
    tgt_len = np.array([351, 352, 511])
    in_len = np.array([512, 512, 512])
    logits = torch.from_numpy((rs.randn(B, T, V) * 3.0).astype(np.float32))
    targets = np.stack([targets_without_repeats(rs, 511, V) for _ in range(B)])
    ws = torch.full((ops.ctc_align_workspace_bytes(B, T, 511),), 0xFF, dtype=torch.uint8, device=device)
    out, nll = run(device, logits, targets, in_len, tgt_len, workspace=ws)
    check_batch(out, nll, logits, targets, in_len, tgt_len)
    assert torch.isfinite(out[4]).all()
    again, _ = run(device, logits, targets, in_len, tgt_len)
    assert same_bits(out, again)


# ---------------------------------------------------------------- case C: known answer (the tie rule)
def test_known_answer_uniform_logits(device):
    """uniform logits, V = 6, targets [2, 3, 3, 4]: every complete path ties, the tie rule decides (test_ctc_align_cpu.py).  The score
    is exact: T additions of the one emission value x - lse, in f32, in order."""
    from joeys2t_amd import ops
    V, T = 6, 10
    logits = torch.zeros(3, T, V)
    targets = np.array([[2, 3, 3, 4]] * 3)
    in_len, tgt_len = np.array([10, 5, 4]), np.array([4, 4, 4])
    out, _ = run(device, logits, targets, in_len, tgt_len)
    path, ts, te, fl, score = (o.cpu().numpy() for o in out)
    assert path[0].tolist() == [1, 3, 4, 5, 7, 8, 8, 8, 8, 8]
    assert ts[0].tolist() == [0, 1, 3, 4] and te[0].tolist() == [1, 2, 4, 5]
    assert path[1].tolist() == [1, 3, 4, 5, 7] + [-1] * 5
    assert ts[1].tolist() == [0, 1, 3, 4] and te[1].tolist() == [1, 2, 4, 5]
    assert score[2] == -np.inf and (path[2] == -1).all() and (ts[2] == -1).all() and (te[2] == -1).all() and (fl[2] == 0).all()
    lse, _ = ops.row_lse(logits.view(-1, V).to(device))
    lp = np.float32(0.0) - lse.cpu().numpy().astype(np.float32)
    assert abs(float(lp[0]) + np.log(6.0)) <= 1e-6
    for b, n in ((0, 10), (1, 5)):
        want = np.float32(lp[b * T])
        for t in range(1, n):
            want = np.float32(want + lp[b * T + t])
        assert score[b] == want and (fl[b, :n] == lp[b * T:b * T + n]).all() and (fl[b, n:] == 0).all()


# ---------------------------------------------------------------- case D: planted paths
def planted(rs, T, V):
    """a random target with one doubled token, a random state path for it over T frames, logits = noise in +-1 with +8 on the path's
    label of every frame"""
    L = int(rs.randint(3, 11))
    target = targets_without_repeats(rs, L, V)
    k = int(rs.randint(0, L - 1))
    target[k + 1] = target[k]
    if k + 2 < L and target[k + 2] == target[k + 1]:
        target[k + 2] = target[k + 1] % (V - 1) + 1
    ext = R.extended(target, BLANK)
    states = []
    for s in range(len(ext)):
        forced = s & 1 or (0 < s < len(ext) - 1 and ext[s - 1] == ext[s + 1])
        if forced or rs.rand() < 0.5:
            states.append(s)
    cuts = np.sort(rs.choice(np.arange(1, T), size=len(states) - 1, replace=False))
    path = np.repeat(states, np.diff(np.concatenate(([0], cuts, [T]))))
    x = rs.uniform(-1.0, 1.0, size=(T, V))
    x[np.arange(T), ext[path]] += 8.0
    return target, path, x.astype(np.float32)


def test_planted_paths(device):
    rs = np.random.RandomState(21)
    V, Tmax, Lmax = 32, 150, 10
    lens = [30, 150, 31, 64, 65, 97, 128, 129, 45, 111]
    B = len(lens)
    logits = torch.zeros(B, Tmax, V)
    targets, in_len, tgt_len, paths = np.ones((B, Lmax), dtype=np.int64), np.array(lens), np.zeros(B, dtype=np.int64), []
    for b, T in enumerate(lens):
        t, p, x = planted(rs, T, V)
        R.check_path(p, t.tolist(), BLANK)
        targets[b, :len(t)], tgt_len[b] = t, len(t)
        logits[b, :T] = torch.from_numpy(x)
        paths.append(p)
    out, nll = run(device, logits, targets, in_len, tgt_len)
    check_batch(out, nll, logits, targets, in_len, tgt_len, want_paths=paths)


# ---------------------------------------------------------------- padding, packing, infeasible neighbours, repeatability
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_poisoned_padding(device, dtype):
    """NaN in the logits and lse rows behind every length, an id outside the vocabulary in the target slots behind every target
    length, garbage in the workspace: all five outputs bit for bit those of the clean run"""
    from joeys2t_amd import ops
    logits, targets, in_len, tgt_len = case_a()
    B, T, V = logits.shape
    clean, _ = clean_a(dtype)
    dead = torch.arange(T)[None, :] >= torch.as_tensor(in_len)[:, None]
    lg = logits.to(dtype).to(device)
    lse, _ = ops.row_lse(lg.view(B * T, V))
    lg = lg.clone()
    lg[dead.to(device)] = float("nan")
    lse = lse.clone()
    lse[dead.view(-1).to(device)] = float("nan")
    tg = torch.as_tensor(targets).clone()
    tg[torch.arange(tg.shape[1])[None, :] >= torch.as_tensor(tgt_len)[:, None]] = V + 1000
    ws = torch.randint(0, 256, (ops.ctc_align_workspace_bytes(B, T, tg.shape[1]) + 64,), dtype=torch.uint8,
                       generator=torch.Generator().manual_seed(1)).to(device)
    out = ops.ctc_align(lg, lse, tg.to(device), torch.as_tensor(in_len).to(device), torch.as_tensor(tgt_len).to(device), BLANK, workspace=ws)
    torch.cuda.synchronize()
    assert same_bits(out, clean)


@pytest.mark.parametrize("V", [37, 40])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_packed_rows_equal_padded(device, dtype, V):
    """case A through ops.PackedRows: bit for bit the padded run.  ops.pack_rows moves rows of a multiple of 16 bytes, which rows of
    V = 37 logits are not - those are packed by indexing; the same case at V = 40 goes through ops.pack_rows itself."""
    from joeys2t_amd import ops
    logits, targets, in_len, tgt_len = case_a(V)
    B, T, _ = logits.shape
    clean, _ = clean_a(dtype, V)
    pk = ops.PackedRows.from_lengths(in_len.tolist(), T, device, round_to=16)
    lg = logits.to(dtype).to(device).view(B * T, V)
    if V * lg.element_size() % 16 == 0:
        lg_p = ops.pack_rows(lg, pk)
    else:
        live = (torch.arange(T)[None, :] < torch.as_tensor(in_len)[:, None]).view(-1).to(device)
        lg_p = torch.zeros((pk.rows, V), dtype=dtype, device=device)
        lg_p[:int(in_len.sum())] = lg[live]
    lse_p, _ = ops.row_lse(lg_p)
    out = ops.ctc_align(lg_p, lse_p, torch.as_tensor(targets).to(device), torch.as_tensor(in_len).to(device),
                        torch.as_tensor(tgt_len).to(device), BLANK, pack=pk)
    torch.cuda.synchronize()
    assert same_bits(out, clean)


def test_infeasible_utterances_leave_their_neighbour_alone(device):
    rs = np.random.RandomState(31)
    B, T, V, Lmax = 3, 12, 20, 6
    logits = torch.from_numpy((rs.randn(B, T, V) * 3.0).astype(np.float32))
    targets = np.stack([targets_without_repeats(rs, Lmax, V) for _ in range(B)])
    targets[2, :3] = [7, 7, 8]
    in_len, tgt_len = np.array([5, 12, 3]), np.array([6, 4, 3])  # L - 1 frames; feasible; a doubled label in L frames
    out, nll = run(device, logits, targets, in_len, tgt_len)
    check_batch(out, nll, logits, targets, in_len, tgt_len)
    path, ts, te, fl, score = (o.cpu().numpy() for o in out)
    for b in (0, 2):
        assert score[b] == -np.inf and (path[b] == -1).all() and (ts[b] == -1).all() and (te[b] == -1).all() and (fl[b] == 0).all()
    assert np.isfinite(score[1])
    one, _ = run(device, logits[1:2], targets[1:2], in_len[1:2], tgt_len[1:2])
    assert same_bits([o[1:2] for o in out], one)


def test_no_frames_and_cpu_tensors(device):
    from joeys2t_amd import ops
    logits = torch.randn(2, 4, 8, generator=torch.Generator().manual_seed(2))
    out, _ = run(device, logits, np.array([[1, 2], [3, 4]]), np.array([0, 4]), np.array([0, 2]))
    assert out[4][0].item() == -np.inf and (out[0][0] == -1).all() and (out[3][0] == 0).all() and np.isfinite(out[4][1].item())
    with pytest.raises(ops.Js2tError):
        ops.ctc_align(logits, torch.zeros(8), torch.zeros(2, 2, dtype=torch.int64), torch.tensor([4, 4]), torch.tensor([2, 2]), 0)
    with pytest.raises(ops.Js2tError, match="exceeds"):
        ops.ctc_align(logits.to(device), torch.zeros(8, device=device), torch.zeros(2, 512, dtype=torch.int64, device=device),
                      torch.tensor([4, 4], device=device), torch.tensor([2, 2], device=device), 0)


def test_two_launches_give_the_same_bits(device):
    logits, targets, in_len, tgt_len = case_a()
    for dtype in (torch.float32, torch.bfloat16):
        again, _ = run(device, logits.to(dtype), targets, in_len, tgt_len)
        assert same_bits(again, clean_a(dtype)[0])


def test_captured_launch_replays_the_same_bits(device):
    """the entry point allocates nothing and does not synchronise: captured in a graph and replayed it gives the clean run's bits"""
    from joeys2t_amd import ops
    logits, targets, in_len, tgt_len = case_a()
    B, T, V = logits.shape
    clean, _ = clean_a(torch.float32)
    lg, tg = logits.to(device), torch.as_tensor(targets).to(device)
    il, tl = torch.as_tensor(in_len).to(device), torch.as_tensor(tgt_len).to(device)
    lse, _ = ops.row_lse(lg.view(B * T, V))
    ws = torch.empty((ops.ctc_align_workspace_bytes(B, T, tg.shape[1]),), dtype=torch.uint8, device=device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ctc_align(lg, lse, tg, il, tl, BLANK, workspace=ws)  # first launch outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.ctc_align(lg, lse, tg, il, tl, BLANK, workspace=ws)
    for o in out:
        o.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, clean)


# ---------------------------------------------------------------- end to end on a golden model
@pytest.fixture(scope="module")
def golden_model(device):
    from test_hip_model import batch_kwargs, build
    model, g = build("model_pre", device)
    model.eval()
    return model, batch_kwargs(g, device)


def ctc_frames(model, batch):
    """the model's own CTC logits and input lengths, obtained the way search.ctc_greedy obtains them"""
    with torch.no_grad():
        enc, _, src_mask, _ = model(return_type="encode", **vars(batch))
        ctc_out = model.decoder.project(model.decoder.ctc_output_layer, enc, model.runtime.compute_dtype)
    return ctc_out.float().cpu().numpy().astype(np.float64), src_mask.squeeze(1).sum(dim=1).cpu().numpy()


def check_alignment(a, logp64, Tb, nll_b=None):
    """an alignment.Alignment against the reference run on the same frames: the spans' structure, the two score bounds"""
    ref = R.align(logp64[:Tb], a.tokens, 2)
    if ref["path"] is None:
        assert a.score == -np.inf and all(v == -1 for v in a.start_frame + a.end_frame)
        return False
    L = len(a.tokens)
    path = np.zeros(Tb, dtype=np.int64)  # the state path the spans stand for: blanks between them
    for l in range(L):
        assert 0 <= a.start_frame[l] < a.end_frame[l] <= Tb
        if l:
            assert a.end_frame[l - 1] <= a.start_frame[l] and (a.tokens[l] != a.tokens[l - 1] or a.end_frame[l - 1] < a.start_frame[l])
            path[a.end_frame[l - 1]:a.start_frame[l]] = 2 * l
        path[a.start_frame[l]:a.end_frame[l]] = 2 * l + 1
    if L:
        path[a.end_frame[-1]:] = 2 * L
    R.check_path(path, a.tokens, 2)
    opt = float(ref["score"])
    own = R.path_score(logp64[:Tb], a.tokens, 2, path)
    print(f"tokens {a.tokens} score {a.score:.6f} opt {opt:.6f} f64 score of the path {own:.6f}")
    assert abs(a.score - opt) <= bound(opt) and abs(own - opt) <= bound(opt)
    em = R.emissions(logp64[:Tb], R.extended(a.tokens, 2))[np.arange(Tb), path]
    for l in range(L):
        assert abs(a.logp[l] - em[a.start_frame[l]:a.end_frame[l]].mean()) <= FRAME_LOGP_ATOL
    return True


def test_forced_align_end_to_end(device, golden_model):
    from joeys2t_amd import alignment
    model, batch = golden_model
    assert model.bos_index == 2 and model.encoder.subsampler.n_layers == 2
    logits, in_len = ctc_frames(model, batch)
    als = alignment.forced_align(model, batch)
    trg, trg_len = batch.trg.cpu().numpy(), batch.trg_length.cpu().numpy()
    assert len(als) == trg.shape[0]
    feasible = 0
    for b, a in enumerate(als):
        assert a.tokens == trg[b, :trg_len[b]].tolist()
        if check_alignment(a, R.log_softmax(logits[b]), int(in_len[b])):
            feasible += 1
            assert a.start == [f * 0.04 for f in a.start_frame] and a.end == [f * 0.04 for f in a.end_frame]
    assert feasible >= 1
    assert alignment.forced_align(model, batch, frame_shift_ms=12.5)[0].start == [f * 0.05 for f in als[0].start_frame]


def test_align_hypotheses_of_ctc_greedy(device, golden_model):
    """the frame-wise best path is the best path of its own collapse: its score is the sum of the frames' largest log-probabilities"""
    from joeys2t_amd import alignment
    from joeys2t_amd.search import ctc_greedy
    model, batch = golden_model
    logits, in_len = ctc_frames(model, batch)
    ids, n = ctc_greedy(model, batch)
    als = alignment.align_hypotheses(model, batch, ids)
    for b, a in enumerate(als):
        assert a.tokens == ids[b, :n[b]].tolist()
        logp = R.log_softmax(logits[b])[:int(in_len[b])]
        assert check_alignment(a, logp, int(in_len[b]))
        want = float(logp.max(axis=1).sum())
        assert abs(a.score - want) <= bound(want), (b, a.score, want)


def test_model_without_a_ctc_layer(device):
    from joeys2t_amd import alignment
    from test_hip_model import batch_kwargs, build
    model, g = build("model_pre", device)
    model.loss_function = ("crossentropy", 0.1, 0.0)  # drops the CTC output layer
    model.eval()
    with pytest.raises(ValueError, match="no CTC output layer"):
        alignment.forced_align(model, batch_kwargs(g, device))
