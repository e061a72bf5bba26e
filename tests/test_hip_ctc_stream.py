"""GPU: js2t_ctc_stream_step (ops.ctc_stream_step), the resumable CTC prefix beam search with its endpoint rule.

The yardstick for bits is the one-shot kernel: however a stream's rows are cut into calls, every final record must be what
ops.ctc_beam_search_ctx returns for the record's rows alone - the segments taken from tests/ctc_stream_reference.py, packed by hand -
and the state must end as the same bytes.  Against the float64 reference itself (segments and ids exact, scores within its TOL) on
the streams test_ctc_stream_cpu.py shows to be decidable.  Shapes: T <= 300, V = 12, B <= 3."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import ctc_beam_reference as R
import ctc_stream_reference as S

pytestmark = pytest.mark.gpu

BLANK, BOS, EOS, PAD, V = S.BLANK, S.BLANK, 3, 1, S.V
NAMES = ("a", "b", "c")
CUTS = {"at once": ([10**9], [10**9], [10**9]), "1 / 7 / 63": ([1], [7], [63]), "64 / 65 / empty calls": ([64], [65], [0, 5, 0, 0, 33])}
PHRASES = [(4, 5), (6, 7, 8), (9, 4), (10, 11, 5, 6)]


def bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def device_rows(name, C):
    """the pinned stream's rows on the device, once: (logits, lse, argmax, cand_id, cand_lp); do not modify"""
    from joeys2t_amd import ops
    st = torch.from_numpy(S.stream_case(name)).to("cuda:0")
    cand_id, cand_lp, lse = ops.ctc_beam_candidates(st, C, BLANK)
    _, am = ops.row_lse(st, want_argmax=True)
    return st, lse, am, cand_id, cand_lp


@functools.lru_cache(maxsize=None)
def fusion(kind):
    """the LM / context arguments of a step and of the one-shot search: none, tiny_lm.arpa fused, a small graph on top"""
    from joeys2t_amd.biasing import ContextGraph
    from joeys2t_amd.lm import NGramLM
    from joeys2t_amd.vocabulary import Vocabulary
    if kind == "zero":
        return dict(lm=None, lm_weight=0.0, length_bonus=0.0, context=None, context_weight=0.0)
    vocab = Vocabulary(list("abcdefgh"))  # 4 specials + 8: the 12 ids of the logits
    lm = NGramLM.from_arpa(Path(__file__).resolve().parent / "golden" / "tiny_lm.arpa", vocab, device="cuda:0")
    if kind == "lm":
        return dict(lm=lm, lm_weight=0.5, length_bonus=0.25, context=None, context_weight=0.0)
    return dict(lm=lm, lm_weight=0.3, length_bonus=0.0, context=ContextGraph.from_phrases(PHRASES, V, device="cuda:0"), context_weight=0.7)


def drive(names, cuts, search, kind="zero", max_finals=8, rule=S.RULE):
    """the streams `names` through ops.ctc_stream_step in one launch per call, stream i cut by cuts[i] (cycled; what a call does not
    consume comes first in the next one), flushed by the call that reaches its end.  One host read per call.  Returns (finals per
    stream, the state's bytes, the partial results per stream and call, the number of calls)."""
    from joeys2t_amd import ops
    s, B = S.SEARCHES[search], len(names)
    rows = [device_rows(n, s["C"]) for n in names]
    T = [r[0].shape[0] for r in rows]
    state = ops.ctc_stream_state(B, s["K"], rule["max_len"], "cuda:0")
    out = ops.ctc_stream_outputs("cuda:0", B, s["n_best"], max_finals, rule["max_len"])
    pos, turn, done = [0] * B, [0] * B, [False] * B
    finals, partials, calls = [[] for _ in range(B)], [[] for _ in range(B)], 0
    while not all(done):
        size = []
        for b in range(B):
            size.append(min(cuts[b][turn[b] % len(cuts[b])], T[b] - pos[b]) if pos[b] < T[b] else 0)
            turn[b] += 1
        flush = [int(not done[b] and pos[b] + size[b] == T[b]) for b in range(B)]
        packed = tuple(torch.cat([r[k][pos[b]:pos[b] + size[b]] for b, r in enumerate(rows)]) for k in range(5))
        off = torch.tensor(np.concatenate([[0], np.cumsum(size)]), dtype=torch.int32, device="cuda:0")
        ops.ctc_stream_step(state, packed, off, torch.tensor(flush, dtype=torch.int32, device="cuda:0"), beam=s["K"], n_best=s["n_best"],
                            max_finals=max_finals, max_len=rule["max_len"], blank=BLANK, pad=PAD, bos=BOS, eos=EOS,
                            log_threshold=rule["log_threshold"], min_silence=rule["min_silence"], out=out, **fusion(kind))
        h = ops.ctc_stream_outputs(out["buf"].cpu(), B, s["n_best"], max_finals, rule["max_len"])  # the one host read
        h = {k: v.numpy() for k, v in h.items()}
        calls += 1
        assert calls < 2000
        for b in range(B):
            used, nf = int(h["consumed"][b]), int(h["n_final"][b])
            assert 0 <= used <= size[b] and 0 <= nf <= max_finals and (used == size[b] or nf == max_finals)
            for i in range(nf):
                n = h["fin_len"][b, i]
                finals[b].append(dict(start=int(h["fin_start"][b, i]), n=int(h["fin_n"][b, i]), why=int(h["fin_why"][b, i]), len=n.copy(),
                                      ids=[h["fin_ids"][b, i, k, :n[k]].copy() for k in range(s["n_best"])],
                                      pad_ok=all((h["fin_ids"][b, i, k, n[k]:] == PAD).all() for k in range(s["n_best"])),
                                      **{k: h["fin_" + k][b, i].copy() for k in ("score", "ctc", "lm", "ctx")}))
            partials[b].append(dict(ids=h["part_ids"][b, :h["part_len"][b]].copy(), stable=int(h["stable_len"][b]), start=int(h["part_start"][b]),
                                    finals=len(finals[b])))
            pos[b] += used
            done[b] = done[b] or bool(flush[b] and used == size[b])
    return finals, state.cpu().numpy(), partials, calls


@functools.lru_cache(maxsize=None)
def one_shot(name, search, kind):
    """ops.ctc_beam_search_ctx over the reference's segments of the stream as a hand-built PackedRows: once per case"""
    from joeys2t_amd import ops
    s = S.SEARCHES[search]
    segs = S.segments(S.stream_reference(name, "k6"))  # (the segments do not depend on the search)
    st, lse, am, cand_id, cand_lp = device_rows(name, s["C"])
    seg = torch.tensor([a for a, _, _ in segs] + [segs[-1][1]], dtype=torch.int32, device="cuda:0")
    pack = ops.PackedRows(seg, len(segs), max(b - a for a, b, _ in segs), st.shape[0])
    in_len = torch.tensor([b - a for a, b, _ in segs], dtype=torch.int64, device="cuda:0")
    f = fusion(kind)
    res = ops.ctc_beam_search_ctx(st, lse, cand_id, cand_lp, in_len, s["K"], s["n_best"], BLANK, PAD, f["lm"], BOS, EOS, f["lm_weight"],
                                  f["length_bonus"], f["context"], f["context_weight"], pack=pack)
    plain = ops.ctc_beam_search(st, lse, cand_id, cand_lp, in_len, s["K"], s["n_best"], BLANK, PAD, pack=pack) if kind == "zero" else None
    return segs, [t.cpu().numpy() for t in res], None if plain is None else [t.cpu().numpy() for t in plain]


def check_finals(finals, name, search, kind, label):
    segs, (ids, n, score, ctc, lm, ctx), plain = one_shot(name, search, kind)
    assert [(r["start"], r["start"] + r["n"], r["why"]) for r in finals] == segs, label
    for i, r in enumerate(finals):
        assert r["pad_ok"] and np.array_equal(r["len"], n[i]), (label, i)
        for k in range(len(r["ids"])):
            assert np.array_equal(r["ids"][k], ids[i, k, :n[i, k]]), (label, i, k)
        for key, want in (("score", score), ("ctc", ctc), ("lm", lm), ("ctx", ctx)):
            assert np.array_equal(bits(r[key]), bits(want[i])), (label, i, key, r[key], want[i])
        if plain is not None:  # all weights 0: the plain search's bits as well
            assert np.array_equal(r["len"], plain[1][i]) and np.array_equal(bits(r["score"]), bits(plain[2][i])), (label, i)
            assert all(np.array_equal(r["ids"][k], plain[0][i, k, :n[i, k]]) for k in range(len(r["ids"])))


@pytest.mark.parametrize("kind", ["zero", "lm", "ctx"])
@pytest.mark.parametrize("search", list(S.SEARCHES))
def test_every_cutting_gives_the_one_shot_bits_and_one_state(device, search, kind):
    states = {}
    for label, cuts in CUTS.items():
        finals, state, _, calls = drive(NAMES, cuts, search, kind)
        for b, name in enumerate(NAMES):
            check_finals(finals[b], name, search, kind, f"{label}: stream {name}")
        states[label] = state
        print(f"{search} / {kind} / {label}: {calls} calls, {[len(f) for f in finals]} finals")
    assert all(np.array_equal(st, states["at once"]) for st in states.values())
    if kind != "zero":  # the fusion is not a no-op on these streams
        zero = drive(NAMES, CUTS["at once"], search, "zero")[0]
        got = drive(NAMES, CUTS["at once"], search, kind)[0]
        assert any(not np.array_equal(bits(a["score"]), bits(b["score"])) for x, y in zip(zero, got) for a, b in zip(x, y))


@pytest.mark.parametrize("name,search", S.REF_CASES)
def test_against_the_numpy_reference(device, name, search):
    want = S.stream_reference(name, search)
    assert min(r["margin"] for r in want) >= R.DECIDABLE  # (test_ctc_stream_cpu.py asserts it too: nothing is skipped here)
    (finals, ), _, _, _ = drive((name, ), ([37], ), search)
    assert [(r["start"], r["start"] + r["n"], r["why"]) for r in finals] == S.segments(want)
    worst = 0.0
    for got, ref in zip(finals, want):
        assert [tuple(y.tolist()) for y in got["ids"]] == [y for y, _ in ref["hyps"]]
        worst = max([worst] + [abs(float(a) - b) / R.bound(b) for a, (_, b) in zip(got["score"], ref["hyps"])])
    print(f"{name} / {search}: {len(finals)} segments, worst score error / tolerance {worst:.4f}")
    assert worst <= 1.0


def test_full_record_slots_stop_the_stream_and_the_rest_is_sent_again(device):
    want, want_state, _, few = drive(NAMES, CUTS["at once"], "k6", "lm")
    got, state, _, calls = drive(NAMES, CUTS["at once"], "k6", "lm", max_finals=1)
    assert calls > few and calls >= max(len(f) for f in want)  # a call ends at its first final
    for b, name in enumerate(NAMES):
        check_finals(got[b], name, "k6", "lm", f"max_finals 1: stream {name}")
    assert np.array_equal(state, want_state)
    got, state, _, _ = drive(NAMES, CUTS["1 / 7 / 63"], "k6", "lm", max_finals=2)
    assert all(len(x) == len(y) for x, y in zip(got, want)) and np.array_equal(state, want_state)


def test_stable_prefix(device):
    """stable_len never exceeds the partial; inside a segment the stable prefix only grows and never changes; with all weights 0 it
    is a prefix of the final's best; and the partial is the reference's while the segment is open"""
    (finals, ), _, (partials, ), _ = drive(("b", ), ([7], ), "k6")
    seen, grew = {}, 0
    for p in partials:
        assert 0 <= p["stable"] <= len(p["ids"])
        if p["start"] < 0:
            assert len(p["ids"]) == 0 and p["stable"] == 0
            continue
        prev = seen.get(p["start"])
        if prev is not None:
            assert p["stable"] >= prev["stable"] and p["ids"][:prev["stable"]].tolist() == prev["ids"][:prev["stable"]].tolist()
            grew += p["stable"] > prev["stable"]
        seen[p["start"]] = p
        final = finals[p["finals"]] if p["finals"] < len(finals) else None  # the record that will close this segment
        if final is not None:
            assert final["start"] == p["start"] and final["ids"][0][:p["stable"]].tolist() == p["ids"][:p["stable"]].tolist()
    assert len(seen) >= 3 and grew >= 3 and max(p["stable"] for p in partials) >= 3
    # the reference's partial after the same rows: the same open segment; its labels are printed, not asserted - the stream is
    # decidable under this search where its segments end, not at every frame, and slot 0 may differ where two prefixes nearly tie
    ref = S.Stream(blank=BLANK, **S.SEARCHES["k6"], **S.RULE)
    x, agree = S.stream_case("b"), 0
    for i, p in enumerate(partials[:len(x) // 7]):
        ref.step(x[7 * i:7 * i + 7], flush=7 * i + 7 >= len(x))
        ids, stable, start = ref.partial()
        assert start == p["start"]
        agree += list(ids) == p["ids"].tolist() and stable == p["stable"]
    print(f"partial labels and stable length equal the reference's after {agree} of {len(x) // 7} calls")


def test_a_captured_step_replays_over_consecutive_chunks(device):
    from joeys2t_amd import ops
    s, rule, n = S.SEARCHES["k6"], S.RULE, 48
    rows = device_rows("c", s["C"])
    kw = dict(beam=s["K"], n_best=s["n_best"], max_finals=4, max_len=rule["max_len"], blank=BLANK, pad=PAD, bos=BOS, eos=EOS,
              log_threshold=rule["log_threshold"], min_silence=rule["min_silence"], **fusion("lm"))
    off = torch.tensor([0, n], dtype=torch.int32, device=device)
    eager_state = ops.ctc_stream_state(1, s["K"], rule["max_len"], device)
    eager = [ops.ctc_stream_step(eager_state, tuple(r[i * n:(i + 1) * n].contiguous() for r in rows), off, None, **kw)["buf"].clone() for i in (0, 1)]
    torch.cuda.synchronize()
    assert int(ops.ctc_stream_outputs(eager[0], 1, s["n_best"], 4, rule["max_len"])["n_final"][0]) >= 1
    static = tuple(torch.zeros_like(r[:n]) for r in rows)
    state = ops.ctc_stream_state(1, s["K"], rule["max_len"], device)
    out = ops.ctc_stream_outputs(device, 1, s["n_best"], 4, rule["max_len"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ctc_stream_step(state, static, off, None, out=out, **kw)
    state.zero_()  # (the capture itself launches nothing; a fresh stream either way)
    for i in (0, 1):
        for dst, src in zip(static, rows):
            dst.copy_(src[i * n:(i + 1) * n])
        out["buf"].fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        got = ops.ctc_stream_outputs(out["buf"], 1, s["n_best"], 4, rule["max_len"])
        want = ops.ctc_stream_outputs(eager[i], 1, s["n_best"], 4, rule["max_len"])
        nf = int(want["n_final"][0])
        for k in want:
            if k == "buf":
                continue
            a, b = (got[k], want[k]) if not k.startswith("fin_") else (got[k][:, :nf], want[k][:, :nf])  # (the other slots keep their fill)
            if k == "part_ids":
                a, b = a[:, :int(want["part_len"][0])], b[:, :int(want["part_len"][0])]
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), (i, k)
    assert torch.equal(state, eager_state)


def test_refusals_launch_nothing(device):
    """every limit and every NULL of the header: an error return with a message, the state and the outputs keep their bytes"""
    import ctypes as C

    from joeys2t_amd import ops
    from joeys2t_amd._lib import lib
    K, nb, F, L, n = 4, 2, 2, 16, 8
    rows = tuple(t[:n].contiguous() for t in device_rows("c", 3))
    state = ops.ctc_stream_state(2, K, L, device)
    state.fill_(0x11)
    out = ops.ctc_stream_outputs(device, 2, nb, F, L)
    out["buf"].fill_(7)
    off = torch.tensor([0, 4, n], dtype=torch.int32, device=device)
    flush = torch.zeros(2, dtype=torch.int32, device=device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    names = ["logits", "lse", "argmax", "cand_id", "cand_lp", "row_offsets", "flush", "uni", "table", "capacity", "max_probe", "lm_order",
             "ctx_nodes", "ctx_edges", "ctx_capacity", "ctx_max_probe", "ctx_n_nodes", "ctx_max_fail", "state", "fin_ids", "fin_len", "fin_score",
             "fin_ctc", "fin_lm", "fin_ctx", "fin_start", "fin_n", "fin_why", "consumed", "n_final", "part_ids", "part_len", "stable_len",
             "part_start", "B", "rows", "V", "beam", "n_cand", "n_best", "max_finals", "max_len", "blank", "pad", "bos", "eos", "lm_weight",
             "context_weight", "length_bonus", "log_threshold", "min_silence", "stream"]
    good = dict(zip(names[:5], map(p, rows)), row_offsets=p(off), flush=p(flush), uni=None, table=None, capacity=0, max_probe=1, lm_order=1,
                ctx_nodes=None, ctx_edges=None, ctx_capacity=0, ctx_max_probe=1, ctx_n_nodes=0, ctx_max_fail=0, state=p(state),
                **{k: p(out[k]) for k in names[19:34]}, B=2, rows=n, V=V, beam=K, n_cand=3, n_best=nb, max_finals=F, max_len=L, blank=BLANK,
                pad=PAD, bos=BOS, eos=EOS, lm_weight=0.0, context_weight=0.0, length_bonus=0.0, log_threshold=-0.1, min_silence=2,
                stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert list(good) == names
    bad = [dict(beam=0),dict(beam=33), dict(n_cand=0), dict(n_cand=9), dict(n_best=0), dict(n_best=K + 1), dict(max_finals=0), dict(max_len=0),
           dict(max_len=2**31 // 32), dict(min_silence=-1), dict(log_threshold=float("nan")), dict(blank=-1), dict(blank=V), dict(rows=-1),
           dict(rows=2**31), dict(V=0), dict(V=70000), dict(bos=V), dict(eos=-1), dict(lm_weight=float("inf")), dict(lm_weight=0.5),
           dict(context_weight=float("nan")), dict(context_weight=0.5), dict(length_bonus=float("inf")), dict(B=-1)]
    bad += [{k: None} for k in names[:6] + names[18:34]]
    for change in bad:
        rc = lib().js2t_ctc_stream_step(*{**good, **change}.values())
        msg = lib().js2t_last_error().decode()
        assert rc != 0 and "ctc_stream_step" in msg, (change, rc, msg)
    assert ops.ctc_stream_state.__doc__ and lib().js2t_ctc_stream_state_bytes(1, 33, 10) == 0 and lib().js2t_ctc_stream_state_bytes(1, 4, 0) == 0
    torch.cuda.synchronize()
    assert bool((state == 0x11).all()) and bool((out["buf"] == 7).all())
    # what the binding refuses itself, and one good call: rows = 0 with NULL row arrays, B = 0
    with pytest.raises(ops.Js2tError, match="state"):
        ops.ctc_stream_step(state, rows, off, flush, beam=K + 1, n_best=nb, max_finals=F, max_len=L, blank=BLANK, pad=PAD)
    with pytest.raises(ops.Js2tError, match="row_offsets"):
        ops.ctc_stream_step(state, rows, off[:2], flush, beam=K, n_best=nb, max_finals=F, max_len=L, blank=BLANK, pad=PAD)
    assert lib().js2t_ctc_stream_step(*{**good, "B": 0}.values()) == 0
    state.zero_()
    empty = {**good, **{k: None for k in names[:5]}, "rows": 0}
    assert lib().js2t_ctc_stream_step(*empty.values()) == 0
    torch.cuda.synchronize()
    assert bool((state == 0).all()) and out["consumed"].tolist() == [0, 0] and out["part_start"].tolist() == [-1, -1]
