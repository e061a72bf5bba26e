"""GPU: CTC forced alignment of a whole recording (js2t_ctc_align_long, ops.ctc_align_long, alignment.align_stream,
long_form.align_long) against js2t_ctc_align where both run and against tests/ctc_align_long_reference.py (pinned on the CPU by
test_ctc_align_long_cpu.py).

Bounds.  The kernel's arithmetic is f32 with one rounding per step and a stated tie rule, and so is the reference run in float32
on lp = logits - lse formed in f32 (the kernel's lse, so no exp / log separates the two): path, spans and the BITS of the score must
be identical.  Against the float64 optimum on the same lp: the float64 score of the kernel's path lies within
2 * T * 2^-24 * max(1, |score|) - each of the T additions of either side of a comparison rounds once, by at most 2^-24 relative to
a partial sum no larger than |score|.  score == the sequential f32 sum of frame_logp, bit for bit.

Shapes come from js2t_ctc_align_long_tiles.  S = 2 L + 1 is odd and the tile sizes are even, so "at the edge" is the L whose
last state is the first state of the next lane / wave / block column (S = edge + 1); one below is S = edge - 1, one above S = edge + 3.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ctc_align_long_reference as RL
import ctc_align_reference as R

pytestmark = pytest.mark.gpu

BLANK, V = 0, 32
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def tiles():
    from joeys2t_amd import ops
    return ops.ctc_align_long_tiles()


def targets_without_repeats(rs, L, hi=V):
    t = rs.randint(1, hi, size=L)
    for i in range(1, L):
        while t[i] == t[i - 1]:
            t[i] = rs.randint(1, hi)
    return t.astype(np.int64)


def repeats(target):
    return int(sum(a == b for a, b in zip(target[:-1], target[1:])))


def run(x, target, free_start=False, free_end=False, dtype=torch.float32, blank=BLANK, lse=None, workspace=None, poison=None):
    """the five outputs as NumPy arrays, and lp = logits - lse in f32 (what the kernel adds up); poison: logits to hand to the kernel
    in place of x (lse stays that of x)"""
    from joeys2t_amd import ops
    dev = torch.device("cuda:0")
    lg = torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dtype).contiguous()
    tg = torch.from_numpy(np.asarray(target, dtype=np.int64)).to(dev)
    if lse is None:
        lse = ops.row_lse(lg)[0] if lg.shape[0] else torch.empty((0, ), dtype=torch.float32, device=dev)
    given = lg if poison is None else torch.from_numpy(np.ascontiguousarray(poison)).to(dev).to(dtype).contiguous()
    out = ops.ctc_align_long(given, lse, tg, blank, free_start=free_start, free_end=free_end, workspace=workspace)
    torch.cuda.synchronize()
    lp = (lg.float() - lse[:, None]).cpu().numpy()
    return tuple(o.cpu().numpy() for o in out), lp


def check(out, lp, target, free_start, free_end, blank=BLANK, what=""):
    """every check of the module docstring for one call"""
    path, ts, te, fl, score = out
    T, L = lp.shape[0], len(target)
    ref = RL.align_free(lp, target, blank, free_start, free_end, dtype=np.float32)
    if ref["path"] is None:
        assert score[0] == -np.inf and (path == -1).all() and (ts == -1).all() and (te == -1).all() and (fl == 0).all(), what
        return ref
    assert np.array_equal(path, ref["path"]), (what, np.nonzero(path != ref["path"])[0][:5])
    assert np.array_equal(ts, ref["tok_start"]) and np.array_equal(te, ref["tok_end"]), what
    assert np.array_equal(bits(score), bits(np.float32([ref["score"]]))), (what, score, ref["score"])
    assert np.array_equal(bits(fl), bits(ref["frame_logp"].astype(np.float32))), what
    assert np.array_equal(bits(np.cumsum(fl, dtype=np.float32)[-1:]), bits(score)), what  # the sequential f32 sum, ascending t
    opt = float(RL.align_free(lp, target, blank, free_start, free_end)["score"])
    own = RL.path_score_free(lp, target, blank, path, free_start, free_end)
    tol = 2.0 * T * 2.0 ** -24 * max(1.0, abs(float(score[0])))
    print(f"{what}: T {T} L {L} free {int(free_start)}{int(free_end)} score {score[0]:.6f} f64 optimum {opt:.6f} "
          f"f64 score of the path {own:.6f} |diff| / tol {abs(own - opt) / tol:.4f}")
    assert abs(own - opt) <= tol, (what, own, opt, tol)
    return ref


def logits_for(seed, T, scale=3.0):
    return (np.random.RandomState(seed).randn(T, V) * scale).astype(np.float32)


# ---------------------------------------------------------------- the bits of js2t_ctc_align
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("L", [0, 1, 95, 511])
def test_bits_of_the_utterance_kernel(device, L, dtype):
    """flags 0: all five outputs are ops.ctc_align's for B = 1 (T = L + repeats: the fewest frames with a path, 1 where that is 0 -
    js2t_ctc_align takes no empty batch; T = 375 has no path for L = 511)"""
    from joeys2t_amd import ops
    rs = np.random.RandomState(100 + L)
    target = rs.randint(1, V, size=L).astype(np.int64)  # (repeats included)
    for T in (max(1, L + repeats(target)), 375, 1500):
        lg = torch.from_numpy(logits_for(7 * L + T, T)).to(device).to(dtype)
        tg = torch.from_numpy(target).to(device)
        lse, _ = ops.row_lse(lg)
        new = ops.ctc_align_long(lg, lse, tg, BLANK)
        old = ops.ctc_align(lg[None], lse, tg[None], torch.tensor([T], device=device), torch.tensor([L], device=device), BLANK)
        torch.cuda.synchronize()
        feasible = T >= L + repeats(target)
        assert bool(np.isfinite(old[4].cpu().numpy()[0])) == feasible
        for name, a, b in zip(("path", "tok_start", "tok_end", "frame_logp", "score"), new, old):
            assert np.array_equal(bits(a.cpu().numpy()), bits(b.reshape(a.shape).cpu().numpy())), (name, T, L)


# ---------------------------------------------------------------- tile edges
@pytest.mark.parametrize("off", [-1, 0, 1], ids=["below", "at", "above"])
@pytest.mark.parametrize("unit", [0, 1, 2], ids=["lane", "wave", "block_column"])
def test_tile_edges(device, unit, off):
    t = tiles()
    edge, tt = t[unit], t[3]
    L = edge // 2 + off  # S = edge - 1, edge + 1, edge + 3
    target = targets_without_repeats(np.random.RandomState(edge + off), L)
    n = 0
    for i, T in enumerate((tt - 1, tt, tt + 1, 2 * tt - 1, 2 * tt, 2 * tt + 1)):
        if unit == 2 and T < L + repeats(target):
            continue  # (the block-column case wants a path)
        fs, fe = FLAGS[(i + unit + off) % 4]
        out, lp = run(logits_for(1000 * unit + 10 * T + off, T), target, fs, fe)
        ref = check(out, lp, target, fs, fe, what=f"{('lane', 'wave', 'block column')[unit]} {off:+d}")
        assert ref["path"] is not None or T < L
        n += 1
    assert n >= 3


def test_several_columns_and_tiles(device):
    """three block columns by three time tiles: every anti-diagonal has more than one block; bf16 logits"""
    t = tiles()
    L, T = t[2] + 37, 2 * t[3] + 91
    target = targets_without_repeats(np.random.RandomState(2), L)
    for fs, fe in ((False, False), (True, True)):
        out, lp = run(logits_for(11, T), target, fs, fe, dtype=torch.bfloat16)
        assert check(out, lp, target, fs, fe, what="3 x 3")["path"] is not None


# ---------------------------------------------------------------- free ends
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_free_ends_planted_path(device, seed):
    x, target, runs = RL.planted_case(seed)
    for fs, fe in FLAGS:
        out, lp = run(x, target, fs, fe)
        check(out, lp, target, fs, fe, what=f"planted {seed}")
        if fs and fe:
            assert RL.planted_ok(dict(path=out[0], tok_start=out[1], tok_end=out[2]), runs)
            assert (out[3][out[0] == 0] == 0).all() and (out[3][out[0] == 2 * len(target)] == 0).all()  # free frames count 0.0f


# ---------------------------------------------------------------- skips and repeats at the edges
def test_repeats_across_lane_wave_and_column_edges(device):
    """the s-2 skip is forbidden exactly where the label two states back - in the lane to the left, the last lane of the wave to the
    left, the last wave of the column to the left - is the same label; few frames to spare, so every allowed skip is taken"""
    kl, ws, sb, _ = tiles()
    L = sb // 2 + 9
    target = targets_without_repeats(np.random.RandomState(9), L)
    for edge in (kl, 2 * kl, ws, 2 * ws, sb):  # state `edge` + 1 is label edge / 2, the first label of its lane; two back: label edge / 2 - 1
        target[edge // 2] = target[edge // 2 - 1]
        target[edge // 2 + 1] = next(v for v in range(1, V) if v not in (target[edge // 2], target[edge // 2 + 2]))
    rep = repeats(target)
    assert rep == 5
    for T in (L + rep - 1, L + rep, L + rep + 3, 2 * L):
        out, lp = run(logits_for(T, T), target)
        ref = check(out, lp, target, False, False, what="repeats")
        assert (ref["path"] is None) == (T < L + rep)
        if ref["path"] is not None:
            R.check_path(out[0], target, BLANK)


# ---------------------------------------------------------------- poison
def test_poison_in_workspace_and_unread_columns(device):
    from joeys2t_amd import ops
    kl, ws, sb, tt = tiles()
    L, T = ws + 3, tt + 70
    rs = np.random.RandomState(31)
    target = targets_without_repeats(rs, L, hi=16)  # ids 1 .. 15: columns 16 .. 31 are read by no state
    x = logits_for(32, T)
    clean, _ = run(x, target, True, False)
    poisoned = x.copy()
    poisoned[:, 16:] = np.nan
    need = ops.ctc_align_long_workspace_bytes(T, L)
    fills = (torch.full((need, ), 0xFF, dtype=torch.uint8, device=device),
             torch.from_numpy(rs.randint(0, 256, size=need).astype(np.uint8)).to(device))
    for wsp in fills:
        got, _ = run(x, target, True, False, workspace=wsp, poison=poisoned)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, clean))
    with pytest.raises(ops.Js2tError, match="workspace"):
        run(x, target, workspace=fills[0][:need - 1])


# ---------------------------------------------------------------- infeasible and degenerate
def no_path(out):
    path, ts, te, fl, score = out
    return score[0] == -np.inf and (path == -1).all() and (ts == -1).all() and (te == -1).all() and (fl == 0).all()


def test_infeasible_and_degenerate(device):
    target = targets_without_repeats(np.random.RandomState(1), 9)
    for fs, fe in FLAGS:
        out, _ = run(np.zeros((0, V), dtype=np.float32), target, fs, fe)  # no frames
        assert no_path(out) and out[0].shape == (0, ) and out[1].shape == (9, )
        out, _ = run(logits_for(3, 8), target, fs, fe)  # T = L - 1
        assert no_path(out)
        bad = target.copy()
        bad[4] = V  # an id outside the vocabulary: every path passes its state
        assert no_path(run(logits_for(4, 40), bad, fs, fe)[0])
        bad[4] = -1
        assert no_path(run(logits_for(4, 40), bad, fs, fe)[0])
        out, lp = run(logits_for(5, 7), [], fs, fe)  # no labels: one state, freed by either flag
        assert (out[0] == 0).all() and out[1].shape == (0, )
        want = np.zeros(7, dtype=np.float32) if (fs or fe) else lp[:, BLANK]
        assert np.array_equal(bits(out[3]), bits(want)) and np.array_equal(bits(out[4]), bits(np.cumsum(want, dtype=np.float32)[-1:]))
    out, _ = run(np.zeros((0, V), dtype=np.float32), [])
    assert out[4][0] == -np.inf
    # a blank outside the vocabulary: -inf unless both of a one-label text's blank states are free
    out, lp = run(logits_for(6, 5), [3], True, True, blank=V)
    assert np.isfinite(out[4][0]) and check(out, lp, [3], True, True, blank=V, what="blank outside")["path"] is not None
    assert no_path(run(logits_for(6, 5), [3, 3], True, True, blank=V)[0])  # (the blank between the repeats cannot be skipped)


def test_limits_and_nulls_are_refused(device):
    from joeys2t_amd import ops
    from joeys2t_amd._lib import lib
    T, L = 6, 2
    lg = torch.zeros((T, V), device=device)
    lse = torch.zeros((T, ), device=device)
    tg = torch.ones((L, ), dtype=torch.int64, device=device)
    out = [torch.full((n, ), 7, dtype=dt, device=device) for n, dt in ((T, torch.int32), (L, torch.int32), (L, torch.int32), (T, torch.float32),
                                                                     (1, torch.float32))]
    wsp = torch.zeros((ops.ctc_align_long_workspace_bytes(T, L), ), dtype=torch.uint8, device=device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    good = dict(logits=p(lg), dt=0, lse=p(lse), targets=p(tg), path=p(out[0]), ts=p(out[1]), te=p(out[2]), fl=p(out[3]), score=p(out[4]),
                ws=p(wsp), T=T, V=V, L=L, blank=0, fs=0, fe=0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cases = [(dict(T=2**31), "bad shape"), (dict(T=-1), "bad shape"), (dict(V=0), "bad shape"), (dict(L=-1), "bad shape"),
             (dict(L=2**20), "exceeds"), (dict(dt=7), "dtype"), (dict(ws=None), "workspace"), (dict(logits=None), "null"),
             (dict(targets=None), "null"), (dict(score=None), "null"), (dict(ws=ctypes.c_void_p(wsp.data_ptr() + 4)), "aligned")]
    for change, word in cases:
        a = {**good, **change}
        rc = lib().js2t_ctc_align_long(*a.values(), stream)
        assert rc != 0 and word in lib().js2t_last_error().decode(), (change, lib().js2t_last_error())
    torch.cuda.synchronize()
    assert all((o == 7).all() for o in out)  # nothing was launched
    assert ops.ctc_align_long_workspace_bytes(0, 5) == 0 and ops.ctc_align_long_workspace_bytes(1, 0) > 0
    assert lib().js2t_ctc_align_long(*good.values(), stream) == 0  # (the unchanged arguments are accepted)
    torch.cuda.synchronize()
    assert np.isfinite(out[4].item())
    with pytest.raises(ops.Js2tError, match="CPU tensor"):
        ops.ctc_align_long(lg.cpu(), lse, tg, 0)
    with pytest.raises(ops.Js2tError, match="CPU tensor"):
        ops.ctc_align_long(lg, lse, tg.cpu(), 0)
    with pytest.raises(ops.Js2tError, match="int64"):
        ops.ctc_align_long(lg, lse, tg.int(), 0)
    with pytest.raises(ops.Js2tError, match="lse"):
        ops.ctc_align_long(lg, lse[:3], tg, 0)
    with pytest.raises(ops.Js2tError, match=r"\[T, V\]"):
        ops.ctc_align_long(lg[None], lse, tg, 0)


# ---------------------------------------------------------------- determinism, capture
def test_two_calls_and_a_replayed_capture_give_the_same_bits(device):
    from joeys2t_amd import ops
    kl, ws, sb, tt = tiles()
    L, T = sb // 2 + 20, tt + 130  # two block columns, two time tiles: four forward launches, the back-trace, the outputs
    target = targets_without_repeats(np.random.RandomState(3), L)
    lg = torch.from_numpy(logits_for(8, T)).to(device)
    tg = torch.from_numpy(target).to(device)
    lse, _ = ops.row_lse(lg)
    wsp = torch.empty((ops.ctc_align_long_workspace_bytes(T, L), ), dtype=torch.uint8, device=device)
    first = [o.clone() for o in ops.ctc_align_long(lg, lse, tg, BLANK, True, True, workspace=wsp)]
    second = ops.ctc_align_long(lg, lse, tg, BLANK, True, True, workspace=wsp)
    torch.cuda.synchronize()
    assert np.isfinite(first[4].item())
    assert all(np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())) for a, b in zip(first, second))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ctc_align_long(lg, lse, tg, BLANK, True, True, workspace=wsp)  # first launch outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # every launch of the call is on the capturing stream: a chain, no parallel branches
        out = ops.ctc_align_long(lg, lse, tg, BLANK, True, True, workspace=wsp)
    for fill in (7, 11):
        for o in out:
            o.fill_(fill)
        wsp.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())) for a, b in zip(first, out))


# ---------------------------------------------------------------- end to end with the golden model
@functools.lru_cache(maxsize=None)
def golden_model():
    from test_hip_model import build
    model, _ = build("model_pre", torch.device("cuda:0"))
    model.eval()
    return model


def test_align_long_on_the_golden_model(device):
    import joeys2t_amd
    from joeys2t_amd import alignment, long_form
    model = golden_model()
    feat = np.random.RandomState(3).randn(96, 8).astype(np.float32)  # 5 windows of 32 feature frames, 24 encoder frames
    kw = dict(window=32, overlap=8, batch_size=2)
    recs = joeys2t_amd.transcribe_long(model, feat, beam_size=4, **kw)  # no segmentation: one utterance, so its labelling has a path
    said = [int(v) for r in recs for v in r["ids"][0].tolist()]
    st, lse, _, _ = long_form.stitch_posteriors(model, feat, **kw)
    lp = (st - lse[:, None]).cpu().numpy()
    sec = alignment.frame_seconds(model)
    for tokens in (said, [5, 6, 6, 7, 9]):
        for fs, fe in ((True, True), (False, False)):
            al = joeys2t_amd.align_long(model, feat, tokens, free_start=fs, free_end=fe, **kw)
            ref = RL.align_free(lp, tokens, int(model.bos_index), fs, fe, dtype=np.float32)
            assert ref["path"] is not None and al.tokens == list(tokens)
            assert al.start_frame == ref["tok_start"].tolist() and al.end_frame == ref["tok_end"].tolist()
            assert np.float32(al.score) == np.float32(ref["score"])
            assert al.start == [f * sec for f in al.start_frame] and al.end == [f * sec for f in al.end_frame]
    tokens = [5, 6, 6, 7, 9]
    al, spans = joeys2t_amd.align_long(model, feat, torch.tensor(tokens), utterances=[2, 3], **kw)
    assert len(spans) == 2 and all(s[0] <= s[1] for s in spans) and spans[0][1] <= spans[1][0]
    assert spans[0][0] == al.start[0] and spans[1][1] == al.end[4] and all(s[3] == s[2] for s in spans)  # (shorter than the window)
    assert len(alignment.word_segments(["▁a", "b", "▁c", "d", "e"], al)) == 2
    with pytest.raises(ValueError, match="utterances"):
        joeys2t_amd.align_long(model, feat, tokens, utterances=[2, 2], **kw)
    with pytest.raises(ValueError, match="1-d integer"):
        joeys2t_amd.align_long(model, feat, [[5, 6]], **kw)
    with pytest.raises(ValueError, match="1-d integer"):
        joeys2t_amd.align_long(model, feat, [5.0, 6.0], **kw)


def test_align_long_refuses_a_model_without_a_ctc_layer(device):
    import joeys2t_amd
    from types import SimpleNamespace
    model = SimpleNamespace(decoder=SimpleNamespace(), encoder=SimpleNamespace(), bos_index=2)
    with pytest.raises(ValueError, match="no CTC output layer"):
        joeys2t_amd.align_long(model, np.zeros((40, 8), dtype=np.float32), [5], window=32, overlap=8)
