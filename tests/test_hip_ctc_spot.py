"""GPU: phrase spotting in a CTC stream (js2t_ctc_spot, ops.ctc_spot, spotting.find_phrases, long_form.spot_long) against
tests/ctc_spot_reference.py (pinned on the CPU by test_ctc_spot_cpu.py).

Bounds.  The kernel's arithmetic is f32 with one rounding per step and a stated tie rule, and so is the reference run in float32 on
the same f32 logits and normaliser: frame_score, frame_start and the hit lists must be identical, the scores bit for bit.  Against
the float64 reference, at the end frame of every reported hit: |score - h64| <= 2 (n + 1) 2^-24 max(1, |score|), n the number of
frames from the earlier of the two starts to the end - one rounding per addition on either side of a comparison, one for the
emission.  The ratio is printed.

Shapes come from js2t_ctc_spot_tiles: (most labels per phrase, phrases per block, frames per prefetch group); the dense outputs are
stored 64 frames (one per lane) at a time, so T also crosses 64 and 128.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import ctc_spot_reference as RS

pytestmark = pytest.mark.gpu

BLANK, V = 0, 32
ALL = -1e30  # a threshold every finite score passes
SENT = 77    # what outputs are pre-filled with


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def tiles():
    from joeys2t_amd import ops
    return ops.ctc_spot_tiles()


def logits_for(seed, T, scale=2.0):
    return (np.random.RandomState(seed).randn(T, V) * scale).astype(np.float32)


def phrase_of(rs, L, hi=16):
    """L ids from 1 .. hi - 1, repeats included"""
    return [int(v) for v in rs.randint(1, hi, size=L)]


def pack(phrases, Lmax=None, fill=0):
    Lmax = Lmax or max(len(p) for p in phrases)
    tok = np.full((len(phrases), Lmax), fill, dtype=np.int64)
    for k, p in enumerate(phrases):
        tok[k, :len(p)] = p
    return tok, np.array([len(p) for p in phrases], dtype=np.int32)


def run(x, phrases, thr, dtype=torch.float32, blank=BLANK, max_hits=16, Lmax=None, fill=0, given=None, prefill=True):
    """(the six outputs as NumPy arrays, the logits as f32 after the conversion to `dtype`, norm f32 = their row maximum); given:
    logits to hand to the kernel in place of x (norm stays that of x); outputs pre-filled with SENT"""
    from joeys2t_amd import ops
    dev = torch.device("cuda:0")
    lg = torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dtype).contiguous()
    T, K = lg.shape[0], len(phrases)
    norm = lg.float().max(dim=1).values.contiguous() if T else torch.empty((0, ), dtype=torch.float32, device=dev)
    tok, length = pack(phrases, Lmax, fill)
    out = None
    if prefill:
        out = tuple(torch.full(shape, SENT, dtype=dt, device=dev) for shape, dt in (
            ((K, ), torch.int32), ((K, max_hits), torch.int32), ((K, max_hits), torch.int32), ((K, max_hits), torch.float32),
            ((K, T), torch.float32), ((K, T), torch.int32)))
    handed = lg if given is None else torch.from_numpy(np.ascontiguousarray(given)).to(dev).to(dtype).contiguous()
    out = ops.ctc_spot(handed, norm, torch.from_numpy(tok).to(dev), torch.from_numpy(length).to(dev), blank, thr, max_hits=max_hits,
                       frame_scores=True, out=out)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out), lg.float().cpu().numpy(), norm.cpu().numpy()


def check(out, xf, norm, phrases, thr, blank=BLANK, what=""):
    """every check of the module docstring for one call; returns the reference hits per phrase"""
    count, start, end, score, fscore, fstart = out
    max_hits, all_hits, worst = start.shape[1], [], 0.0
    thr32 = np.float32(thr)
    for k, phrase in enumerate(phrases):
        h, s = RS.spot(xf, norm, phrase, blank, np.float32)
        assert np.array_equal(bits(fscore[k]), bits(h)), (what, k, np.nonzero(bits(fscore[k]) != bits(h))[0][:5])
        assert np.array_equal(fstart[k], s), (what, k, np.nonzero(fstart[k] != s)[0][:5])
        hits = RS.pick(h, s, thr32)
        all_hits.append(hits)
        assert count[k] == len(hits), (what, k, count[k], len(hits))
        n = min(len(hits), max_hits)
        assert start[k, :n].tolist() == [a for a, _, _ in hits[:n]] and end[k, :n].tolist() == [e for _, e, _ in hits[:n]], (what, k)
        assert np.array_equal(bits(score[k, :n]), bits(np.array([sc for _, _, sc in hits[:n]], dtype=np.float32))), (what, k)
        assert (start[k, n:] == SENT).all() and (end[k, n:] == SENT).all() and (score[k, n:] == SENT).all(), (what, k)
        if n:
            h64, s64 = RS.spot(xf.astype(np.float64), norm.astype(np.float64), phrase, blank, np.float64)
            for a, e, sc in hits[:n]:
                frames = e - min(a, int(s64[e - 1]))
                tol = 2.0 * (frames + 1) * 2.0 ** -24 * max(1.0, abs(float(sc)))
                worst = max(worst, abs(float(sc) - float(h64[e - 1])) / tol)
                assert abs(float(sc) - float(h64[e - 1])) <= tol, (what, k, a, e, sc, h64[e - 1], tol)
    print(f"{what}: T {xf.shape[0]} K {len(phrases)} hits {[len(h) for h in all_hits][:8]} worst |f32 - f64| / tol {worst:.4f}")
    return all_hits


def thresholds(xf, norm, phrases, blank=BLANK):
    """everything, and a threshold in the middle of the finite scores, at which candidates are replaced, extended and dropped"""
    h = np.concatenate([RS.spot(xf, norm, p, blank, np.float32)[0] for p in phrases]) if phrases else np.zeros(0)
    h = h[np.isfinite(h)]
    return (ALL, float(np.median(h))) if h.size else (ALL, )


def run_and_check(x, phrases, what, dtype=torch.float32, blank=BLANK, **kw):
    xf = torch.from_numpy(x).to(dtype).float().numpy()
    norm = xf.max(axis=1) if xf.shape[0] else np.zeros(0, dtype=np.float32)
    found = []
    for thr in thresholds(xf, norm, phrases, blank):
        out, xf2, norm2 = run(x, phrases, thr, dtype=dtype, blank=blank, **kw)
        assert np.array_equal(bits(xf), bits(xf2)) and np.array_equal(bits(norm), bits(norm2))
        found.append(check(out, xf, norm, phrases, thr, blank, what=f"{what} thr {thr:.3g}"))
    return found


# ---------------------------------------------------------------- phrase length: the last lane in use
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_phrase_lengths(device, dtype):
    most = tiles()[0]
    assert most == 32
    rs = np.random.RandomState(0)
    for L in (1, 2, most - 1, most):  # the last lane in use: 0, 2, 60, 62
        phrase = phrase_of(rs, L)
        found = run_and_check(logits_for(L, 75), [phrase], f"L {L}", dtype=dtype, max_hits=80)
        assert len(found[0][0]) >= 1  # (with every finite score a candidate there is a hit)


# ---------------------------------------------------------------- block occupancy
@pytest.mark.parametrize("off", [-1, 0, 1], ids=["below", "at", "above"])
def test_block_occupancy(device, off):
    most, per_block, _ = tiles()
    K = per_block + off
    rs = np.random.RandomState(10 + off)
    lengths = [1, most] + [int(rs.randint(2, 9)) for _ in range(K - 2)]  # a one-label phrase beside a 32-label phrase
    phrases = [phrase_of(rs, L) for L in lengths]
    run_and_check(logits_for(20 + off, 70), phrases, f"K {K}", max_hits=70)
    run_and_check(logits_for(30 + off, 40), phrases[::-1] + phrases, f"K {2 * K}", max_hits=40)  # more than one block in every case


# ---------------------------------------------------------------- prefetch groups and the 64-frame output buffer
def test_frame_counts_at_group_and_buffer_edges(device):
    G = tiles()[2]
    rs = np.random.RandomState(3)
    phrases = [phrase_of(rs, L) for L in (1, 2, 3, 5)] + [[4, 4]]
    for T in (1, 2, 3, G - 1, G, G + 1, 2 * G + 1, 63, 64, 65, 128, 129):  # (T = 1 .. 3: below L for some of the phrases)
        found = run_and_check(logits_for(100 + T, T), phrases, f"T {T}", max_hits=T)
        for p, hits in zip(phrases, found[0]):
            need = len(p) + sum(a == b for a, b in zip(p[:-1], p[1:]))
            assert bool(hits) == (T >= need), (T, p)


# ---------------------------------------------------------------- repeats: the blank between them cannot be skipped
def test_repeats_need_their_blank(device):
    for phrase, need in (([4, 4], 3), ([3, 4, 4, 5], 5)):
        out, xf, norm = run(logits_for(7, need - 1), [phrase], ALL)
        check(out, xf, norm, [phrase], ALL, what=f"{phrase} one frame short")
        assert out[0][0] == 0 and (out[4] == -np.inf).all() and (out[5] == -1).all()
        out, xf, norm = run(logits_for(7, need), [phrase], ALL)
        hits = check(out, xf, norm, [phrase], ALL, what=f"{phrase} feasible")[0]
        assert [(a, e) for a, e, _ in hits] == [(0, need)] and np.isfinite(out[4][0, -1]) and (out[4][0, :-1] == -np.inf).all()


# ---------------------------------------------------------------- planted phrases
@functools.lru_cache(maxsize=None)
def planted(seed):
    return RS.planted_case(seed)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_planted_phrases(device, seed, dtype):
    x, expected = planted(seed)
    phrases = list(RS.PHRASES) + [RS.ABSENT]
    thr = math.log(0.5)
    out, xf, norm = run(x, phrases, thr, dtype=dtype)
    check(out, xf, norm, phrases, thr, what=f"planted {seed}")
    count, start, end, score = out[:4]
    for k, want in enumerate(expected):
        assert count[k] == len(want) and list(zip(start[k, :count[k]].tolist(), end[k, :count[k]].tolist())) == want
        assert (score[k, :count[k]] == 0.0).all()
    assert count[len(expected)] == 0


# ---------------------------------------------------------------- more hits than room
def three_of_seven():
    """[7] three times (frames 5, 15 .. 16, 30), [9] once (frame 22), ids 16 .. 31 elsewhere"""
    rs = np.random.RandomState(5)
    x = rs.randn(40, V).astype(np.float32)
    ids = {5: 7, 15: 7, 16: 7, 30: 7, 22: 9}
    for t in range(40):
        x[t, ids.get(t, int(rs.randint(16, 32)))] += 8.0
    return x


def test_more_hits_than_room(device):
    from joeys2t_amd import spotting
    x, thr = three_of_seven(), math.log(0.5)
    phrases = [[7], RS.ABSENT, [9]]
    for room in (1, 2):
        out, xf, norm = run(x, phrases, thr, max_hits=room)
        check(out, xf, norm, phrases, thr, what=f"room {room}")  # (the entries behind min(count, room): SENT)
        count, start, end, score = out[:4]
        assert count.tolist() == [3, 0, 1]  # what was FOUND
        assert (start[0, 0], end[0, 0], score[0, 0]) == (5, 6, 0.0) and (start[2, 0], end[2, 0]) == (22, 23)
        assert (start[1] == SENT).all() and (score[1] == SENT).all()
        if room == 2:
            assert (start[0, 1], end[0, 1]) == (15, 17) and start[2, 1] == SENT and end[2, 1] == SENT and score[2, 1] == SENT
    lg = torch.from_numpy(x).to(device)
    stream = (lg, lg.new_zeros(40), lg.argmax(dim=1), lg.new_zeros(40))  # (lse and blank_lp are not read)
    hits = spotting.find_phrases(stream, phrases, BLANK, 0.04, max_hits=1)
    assert [(h.phrase, h.start_frame, h.end_frame, h.score) for h in hits] == [(0, 5, 6, 0.0), (0, 15, 17, 0.0), (2, 22, 23, 0.0), (0, 30, 31, 0.0)]
    assert [(h.start, h.end) for h in hits] == [(h.start_frame * 0.04, h.end_frame * 0.04) for h in hits]
    hits2, fscore, fstart = spotting.find_phrases(stream, phrases, BLANK, 0.04, frame_scores=True)
    assert hits2 == hits and fscore.shape == (3, 40) and fstart.dtype == torch.int32 and fscore[0, 16].item() == 0.0 and fstart[0, 16].item() == 15
    assert spotting.find_phrases(stream, [], BLANK, 0.04) == []


# ---------------------------------------------------------------- poison
def test_poison_in_padding_unread_columns_and_outputs(device):
    rs = np.random.RandomState(8)
    phrases = [phrase_of(rs, L) for L in (1, 3, 7, 2, 12)]  # ids 1 .. 15 and the blank: columns 16 .. 31 are read by no phrase
    x = logits_for(9, 90)
    xf, norm = x, x.max(axis=1)
    thr = thresholds(xf, norm, phrases)[1]
    clean, _, _ = run(x, phrases, thr, max_hits=90, Lmax=16)
    check(clean, xf, norm, phrases, thr, what="clean")
    poisoned = x.copy()
    poisoned[:, 16:] = np.nan
    for fill in (-1, V + 7):  # tokens behind the lengths
        got, _, _ = run(x, phrases, thr, max_hits=90, Lmax=16, fill=fill, given=poisoned)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, clean)), fill
    # a one-label phrase reads no blank: with the blank's column NaN as well it is unchanged
    poisoned[:, BLANK] = np.nan
    got, _, _ = run(x, phrases[:1], thr, max_hits=90, Lmax=16, fill=-1, given=poisoned)
    assert all(np.array_equal(bits(a[:1]), bits(b[:1])) for a, b in zip(got, clean))


# ---------------------------------------------------------------- ids outside the vocabulary
def test_ids_outside_the_vocabulary(device):
    x = logits_for(12, 30)
    for bad in (V, -1):
        phrases = [[3, bad, 5], [bad], [3, 5]]
        out, xf, norm = run(x, phrases, ALL, max_hits=30)
        check(out, xf, norm, phrases, ALL, what=f"id {bad}")
        assert out[0].tolist()[:2] == [0, 0] and out[0][2] > 0
        assert (out[4][:2] == -np.inf).all() and (out[5][:2] == -1).all()
    for blank in (V, -1):  # a blank outside: one-label phrases work, a repeat has no path, other phrases take the step over the blank
        phrases = [[3], [4, 4], [3, 5]]
        out, xf, norm = run(x, phrases, ALL, blank=blank, max_hits=30)
        hits = check(out, xf, norm, phrases, ALL, blank=blank, what=f"blank {blank}")
        assert len(hits[0]) > 0 and out[0][1] == 0 and (out[4][1] == -np.inf).all() and len(hits[2]) > 0


# ---------------------------------------------------------------- degenerate and refused
def test_no_phrases_and_no_frames(device):
    out, _, _ = run(logits_for(1, 10), [], ALL, Lmax=1)  # K = 0
    assert out[0].shape == (0, ) and out[1].shape == (0, 16) and out[4].shape == (0, 10)
    out, _, _ = run(np.zeros((0, V), dtype=np.float32), [[3], [4, 5]], ALL)  # T = 0: the counts are zeroed, nothing else is written
    assert out[0].tolist() == [0, 0] and (out[1] == SENT).all() and (out[3] == SENT).all() and out[4].shape == (2, 0)


def test_limits_and_nulls_are_refused(device):
    from joeys2t_amd import ops
    from joeys2t_amd._lib import lib
    T, K, Lmax, room = 6, 2, 3, 4
    lg = torch.zeros((T, V), device=device)
    norm = torch.zeros((T, ), device=device)
    tok = torch.ones((K, Lmax), dtype=torch.int64, device=device)
    length = torch.ones((K, ), dtype=torch.int32, device=device)
    out = [torch.full(shape, SENT, dtype=dt, device=device) for shape, dt in (
        ((K, ), torch.int32), ((K, room), torch.int32), ((K, room), torch.int32), ((K, room), torch.float32), ((K, T), torch.float32),
        ((K, T), torch.int32))]
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    good = dict(logits=p(lg), dt=0, norm=p(norm), tokens=p(tok), lengths=p(length), K=K, Lmax=Lmax, count=p(out[0]), start=p(out[1]),
                end=p(out[2]), score=p(out[3]), max_hits=room, fscore=p(out[4]), fstart=p(out[5]), T=T, V=V, blank=0, thr=-1.0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cases = [(dict(T=2**31), "bad shape"), (dict(T=-1), "bad shape"), (dict(V=0), "bad shape"), (dict(K=-1), "bad shape"),
             (dict(K=65536), "bad shape"), (dict(Lmax=0), "bad shape"), (dict(Lmax=33), "exceeds"), (dict(max_hits=0), "bad shape"),
             (dict(dt=7), "dtype"), (dict(thr=float("nan")), "finite"), (dict(thr=float("inf")), "finite"),
             (dict(thr=float("-inf")), "finite"), (dict(logits=None), "null"), (dict(norm=None), "null"), (dict(tokens=None), "null"),
             (dict(lengths=None), "null"), (dict(count=None), "null"), (dict(start=None), "null"), (dict(end=None), "null"),
             (dict(score=None), "null")]
    for change, word in cases:
        a = {**good, **change}
        rc = lib().js2t_ctc_spot(*a.values(), stream)
        assert rc != 0 and word in lib().js2t_last_error().decode(), (change, lib().js2t_last_error())
    torch.cuda.synchronize()
    assert all((o == SENT).all() for o in out)  # nothing was launched
    for change in (dict(), dict(fscore=None), dict(fstart=None), dict(fscore=None, fstart=None)):  # (the two frame_* may be NULL)
        assert lib().js2t_ctc_spot(*{**good, **change}.values(), stream) == 0
    torch.cuda.synchronize()
    assert out[0].tolist() == [1, 1] and out[1][0, 0].item() == 0 and out[2][0, 0].item() == T and out[3][0, 0].item() == 0.0
    length32 = length.clone()
    with pytest.raises(ops.Js2tError, match="CPU tensor"):
        ops.ctc_spot(lg.cpu(), norm, tok, length, 0, -1.0)
    with pytest.raises(ops.Js2tError, match="CPU tensor"):
        ops.ctc_spot(lg, norm, tok.cpu(), length, 0, -1.0)
    with pytest.raises(ops.Js2tError, match=r"\[T, V\]"):
        ops.ctc_spot(lg[None], norm, tok, length, 0, -1.0)
    with pytest.raises(ops.Js2tError, match="norm"):
        ops.ctc_spot(lg, norm[:3], tok, length, 0, -1.0)
    with pytest.raises(ops.Js2tError, match="int64"):
        ops.ctc_spot(lg, norm, tok.int(), length, 0, -1.0)
    with pytest.raises(ops.Js2tError, match="int64"):
        ops.ctc_spot(lg, norm, tok[0], length, 0, -1.0)
    with pytest.raises(ops.Js2tError, match="int32"):
        ops.ctc_spot(lg, norm, tok, length32.long(), 0, -1.0)
    with pytest.raises(ops.Js2tError, match="int32"):
        ops.ctc_spot(lg, norm, tok, length[:1], 0, -1.0)
    with pytest.raises(ops.Js2tError, match="out ="):
        ops.ctc_spot(lg, norm, tok, length, 0, -1.0, max_hits=room, out=tuple(out[:3]) + (out[3][:, :2], None, None))
    with pytest.raises(ops.Js2tError, match="exceeds"):
        ops.ctc_spot(lg, norm, torch.ones((K, 33), dtype=torch.int64, device=device), length, 0, -1.0)
    with pytest.raises(ops.Js2tError, match="bad shape"):
        ops.ctc_spot(lg, norm, tok, length, 0, -1.0, max_hits=0)
    with pytest.raises(ops.Js2tError, match="finite"):
        ops.ctc_spot(lg, norm, tok, length, 0, float("nan"))


# ---------------------------------------------------------------- determinism, capture
def test_two_calls_and_a_replayed_capture_give_the_same_bits(device):
    from joeys2t_amd import ops
    x, _ = planted(0)
    phrases = list(RS.PHRASES) + [phrase_of(np.random.RandomState(4), 32)]
    lg = torch.from_numpy(x).to(device)
    norm = lg.max(dim=1).values.contiguous()
    tok, length = (torch.from_numpy(a).to(device) for a in pack(phrases))
    thr = math.log(0.5)
    first = [o.clone() for o in ops.ctc_spot(lg, norm, tok, length, BLANK, thr, max_hits=8, frame_scores=True)]
    out = ops.ctc_spot(lg, norm, tok, length, BLANK, thr, max_hits=8, frame_scores=True)
    torch.cuda.synchronize()
    assert first[0].tolist()[:4] == [6, 6, 6, 6]
    n = [min(int(c), 8) for c in first[0].tolist()]

    def same(got):
        dense = all(np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())) for a, b in zip((first[0], *first[4:]), (got[0], *got[4:])))
        return dense and all(np.array_equal(bits(a[k, :n[k]].cpu().numpy()), bits(b[k, :n[k]].cpu().numpy()))
                             for a, b in zip(first[1:4], got[1:4]) for k in range(len(n)))

    assert same(out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ctc_spot(lg, norm, tok, length, BLANK, thr, max_hits=8, frame_scores=True, out=out)  # first launch outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one launch on the capturing stream
        ops.ctc_spot(lg, norm, tok, length, BLANK, thr, max_hits=8, frame_scores=True, out=out)
    for fill in (7, 11):
        for o in out:
            o.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert same(out)
        assert all((o[k, n[k]:] == fill).all() for o in out[1:4] for k in range(len(n)))  # behind the hits: untouched


# ---------------------------------------------------------------- end to end with the golden model
@functools.lru_cache(maxsize=None)
def golden_model():
    from test_hip_model import build
    model, _ = build("model_pre", torch.device("cuda:0"))
    model.eval()
    return model


def test_spot_long_on_the_golden_model(device):
    import joeys2t_amd
    from joeys2t_amd import alignment, long_form
    model = golden_model()
    feat = np.random.RandomState(3).randn(96, 8).astype(np.float32)  # 5 windows of 32 feature frames, 24 encoder frames
    kw = dict(window=32, overlap=8, batch_size=2)
    st, _, am, _ = long_form.stitch_posteriors(model, feat, **kw)
    xf, am = st.cpu().numpy(), am.cpu().numpy()
    T, Vm = xf.shape
    blank = int(model.bos_index)
    norm = xf[np.arange(T), am]
    labels = [v for v in range(Vm) if v != blank]
    phrases = [[v] for v in labels] + [[5, 6], [5, 6, 6, 7]]
    thr = np.float32(math.log(1e-4))
    want = []
    for k, p in enumerate(phrases):
        want += [(k, a, e, float(sc)) for a, e, sc in RS.pick(*RS.spot(xf, norm, p, blank, np.float32), thr)]
    want.sort(key=lambda w: (w[1], w[0]))
    hits = joeys2t_amd.spot_long(model, feat, phrases, threshold=1e-4, **kw)
    assert [(h.phrase, h.start_frame, h.end_frame, h.score) for h in hits] == want and len(hits) > 0
    sec = alignment.frame_seconds(model)
    assert all(h.start == h.start_frame * sec and h.end == h.end_frame * sec for h in hits)
    spoken = [t for t in range(T) if am[t] != blank]
    print(f"golden model: T {T} V {Vm} hits {len(hits)}, {len(spoken)} frames whose arg-max is a label")
    for t in spoken:  # every frame whose arg-max is a label lies inside a hit of that label's phrase
        k = labels.index(int(am[t]))
        assert any(h.phrase == k and h.start_frame <= t < h.end_frame and h.score == 0.0 for h in hits), t
    assert joeys2t_amd.spot_long(model, feat, phrases, threshold=1e-4, max_hits=1, **kw) == hits  # (the rerun with room for all)
    with pytest.raises(ValueError, match="empty"):
        joeys2t_amd.spot_long(model, feat, [[]], **kw)
    with pytest.raises(ValueError, match="threshold"):
        joeys2t_amd.spot_long(model, feat, [[5]], threshold=float("nan"), **kw)


def test_spot_long_refuses_a_model_without_a_ctc_layer(device):
    import joeys2t_amd
    from types import SimpleNamespace
    model = SimpleNamespace(decoder=SimpleNamespace(), encoder=SimpleNamespace(), bos_index=2)
    with pytest.raises(ValueError, match="no CTC output layer"):
        joeys2t_amd.spot_long(model, np.zeros((40, 8), dtype=np.float32), [[5]], window=32, overlap=8)
