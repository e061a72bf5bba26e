"""The update tail (joeys2t_amd/csrc/optim.hip: gradient norm + clip coefficient, fused AdamW, the table-driven AdamW that also
writes the transposed bf16 shadow and the LayerNorm-fold weights; js2t_fold_ln_weights of csrc/norm_softmax.hip) against plain fp64
references, at the block, unit and grid edges, between sentinels (tests/update_reference.py).

Every comparison goes through update_reference.verdict(), whose numeric checks are elementwise_reference.judge(): an element passes
when |got - ref| <= u_out |ref| + K 2^-24 cond + floor (u_out = 2^-24, cond = the sum of |terms added|, floor = 2^-126).  Every K is
derived from the kernel's operation count (update_reference.K_DERIVED, the count stands next to each number); none is measured.
Exact, bit for bit: lp = the RNE rounding of the p the same launch stored, lp_t = the transpose of lp, a cleared gradient is +0.0, a
kept one keeps its bits, g = m = v = 0 gives exactly the decay, and everything outside the pieces keeps its sentinel in p, g, m, v, lp,
lp_t, Wf, bias_f and partial.  The kernels are called through joeys2t_amd._lib.lib() on buffers, tables and sentinels of the test's own.

CPU (no GPU needed): test_emulation_passes_at_every_case judges an op-for-op float32 emulation of every kernel by the same verdict();
test_judge_rejects_every_mutant shows that it fails each slip of update_reference.MUTANTS at every case the slip applies to.

Measured on MI355X: the largest err / allowed per kernel and output over its cases, the two large ones included (the rule allows 1), and
the largest measured K = max (err - u_out |ref| - floor) / (2^-24 cond) next to the K the rule uses.
    kernel                                output          err / allowed   measured K   K used
    js2t_grad_norm_clip                   partial         0.10            1.81         28  derived
                                          norm            0.04            0.20         27  derived
                                          coefficient     0.03            0            30  derived   (exactly 1 above the norm / clipping off)
    js2t_sumsq_ranges + js2t_norm_clip    partial         0.05            0.43         28  derived
                                          norm            0.04            0.06         27  derived
                                          coefficient     0.05            0.63         30  derived
    js2t_adamw                            m'              0.49            1.46         4   derived
                                          v'              0.50            3.01         7   derived
                                          p'              0.43            2.85         8   derived
    js2t_adamw_items                      m'              0.49            1.47         4   derived
                                          v'              0.52            3.18         7   derived
                                          p'              0.27            1.74         8   derived
                                          bias_f          0.07            0.77         14  derived
                                          Wf element      0.87       )  bounds derived in update_reference.verdict_fold from the bf16
                                          Wf group sum    0.96       )  rounding with feedback (a carry is at most 2^-8 of the group's largest
                                          Wf row sum      0.42       )  target), not from K
    js2t_fold_ln_weights                  bias_f          0.07            0.77         14  derived
                                          Wf element / group sum / row sum     0.87 / 0.96 / 0.42; the same bits as js2t_adamw_items
    lp, lp_t, cleared and kept gradients, g = m = v = 0, everything outside the pieces: bit-exact.
The float32 emulation on the CPU gives the same maxima to two digits (m' 0.49, v' 0.52, p' 0.32, Wf group sum 0.95).  No test exposed a
bug in the kernels.

Which GPU case fails if a slip of MUTANTS were put into the kernel (the CPU self-check shows verdict() rejects it there):
    coupled_decay                 test_adamw_small, every case with weight_decay 0.01 (m', v' and p')
    sqrt_bc2_missing              test_adamw_small at step 1, 2 and (betas 0.9, 0.999) step 1000: p'
    eps_inside_sqrt               test_adamw_small, n >= 1020: p' of the blocks whose gradient is 0.01 x
    step_size_without_bc1         test_adamw_small at step 1 and 2: p'
    gscale_dropped, gscale_dev_dropped, v_from_unscaled_gradient      the cases with gscale 0.5 and *gscale_dev 0.8: m' / v'
    device_step_ignored, lr_dev_ignored       the device-schedule cases: the host's lr is 7 x and its step 1 (3 at step 1)
    lp_truncated                  every case with lp: bit for bit against RNE of the stored p
    zero_grad_ignored             every case with zero_grad 1: the gradient must read +0.0
    keep_flag_ignored             test_adamw_items nine / mixed / folds: the kept pieces must keep their bits
    grid_stride_stops             test_adamw_second_grid_trip: the last 12 elements keep their old values
    last_partial_block_dropped    test_grad_norm_clip / test_sumsq_ranges: the partial of the last block stays a sentinel
    tail_dropped                  n % 4 != 0: the last element weighs > 1 % of the sum
    block_range_off_by_one        test_sumsq_ranges with 2, 5, 8 ranges: the first partial of every later range
    p0_ignored                    test_sumsq_ranges with p0 = 37: partial[0, 37) changes, partial[37 + ..) stays a sentinel
    clip_without_1e-6             test_grad_norm_clip, norm 1e-4: the coefficient moves by 1 %
    clip_not_capped               test_grad_norm_clip, max_norm above the norm: the coefficient must be exactly 1
    lpt_not_transposed, lpt_tail_rows_dropped (rows 20, 63, 65, 130), lpt_second_half_dropped (cols > 256), lpt_c0_ignored
    (cols 516, 1028), lpt_r0_ignored (rows 65, 72, 130)       test_adamw_items with lp_t: bit for bit / sentinels left in lp_t
    fold_not_centred, fold_no_feedback, fold_bias_missing     test_adamw_items folds, test_fold_ln_weights
    fold_old_gamma                test_adamw_items folds: gamma is updated by the 1-D launch first
"""
import ctypes as C

import numpy as np
import pytest
import torch

import update_reference as UR
from attn_reference import poison, sentinel_bf16, sentinel_f32, untouched

gpu = pytest.mark.gpu
LEAD = UR.LEAD
_CACHE = {}


def geo():
    if "geo" not in _CACHE:
        _CACHE["geo"] = UR.geometry()
    return _CACHE["geo"]


def the_plan():
    if "plan" not in _CACHE:
        _CACHE["plan"] = UR.plan(geo())
    return _CACHE["plan"]


def inputs_of(case):
    """the inputs of a case, computed once and shared (nothing changes them: simulate() and the runners copy)"""
    key = ("inp", id(case))
    if key not in _CACHE:
        _CACHE[key] = UR.inputs(case, geo())
    return _CACHE[key]


def cases(op, big=False, **kw):
    return [c for c in the_plan() if c.op == op and bool(c.big) == big and all(getattr(c, k, None) == v for k, v in kw.items())]


# ================================================================================================================ CPU
def test_sentinel_helpers_agree():
    """the numpy sentinels of update_reference are attn_reference's: untouched() accepts them"""
    assert untouched(torch.from_numpy(UR.sent32(9).copy()), []) and untouched(torch.from_numpy(UR.sent16(9).view(np.int16).copy()).view(torch.bfloat16), [])
    assert torch.equal(sentinel_f32(5).view(torch.int32), torch.from_numpy(UR.sent32(5).copy()).view(torch.int32))
    assert torch.equal(sentinel_bf16(1, 5).view(torch.int16).flatten(), torch.from_numpy(UR.sent16(5).view(np.int16).copy()))


def test_bf16_rounding_twin_matches_torch():
    """bf16_rne is torch's round-to-nearest-even, ties both ways; bf16_trunc differs from it"""
    bits = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x00000000, 0x80000000, 0x3F800000, 0x3F7FFFFF], dtype=np.uint32)
    x = np.concatenate([bits.view(np.float32), poison(1, 4096, 7).float().numpy().flatten() * np.float32(1.001)])
    want = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert (UR.bf16_rne(x) == want).all() and (UR.bf16_trunc(x) != want).any()
    assert UR.bf16_rne(bits.view(np.float32))[:4].tolist() == [0x3F80, 0x3F82, 0xBF80, 0xBF82]


def test_reference_matches_torch_adamw_fp64():
    """A guard against a wrong reference: three updates of ref_moments / ref_param against torch.optim.AdamW on fp64 tensors, with the
    gradient scale applied before torch sees the gradient."""
    rng = np.random.default_rng(5)
    n = 64
    for betas, wd, step0 in (((0.9, 0.98), 0.01, 1), ((0.9, 0.999), 0.0, 1)):
        h = UR.Hyper(betas=betas, wd=wd, step=step0, gscale=0.5, gsd=0.8)
        c = UR.consts(h)
        p = rng.standard_normal(n)
        tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
        opt = torch.optim.AdamW([tp], lr=c.lr, betas=(c.b1, c.b2), eps=c.eps, weight_decay=c.wd)
        m, v = np.zeros(n), np.zeros(n)
        for k in range(3):
            g = rng.standard_normal(n)
            tp.grad = torch.from_numpy(g * c.gs)
            opt.step()
            m, _, v, _ = UR.ref_moments(p, g, m, v, h.at(k))
            p, cond = UR.ref_param(p, m, v, h.at(k))
            assert (cond >= np.abs(p) * (1 - 1e-12)).all()
            np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=1e-14)
            st = opt.state[tp]
            np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-15)


def test_plan_reaches_every_edge():
    """the sizes of the plan against the kernels' unit sizes as the library reports them"""
    g = geo()
    SQ, FL, UR_, UC = g["sq"], g["flat"], g["rows"], g["cols"]
    ns = {c.n for c in cases("clip")}
    assert {1, 3, 4, 5, SQ - 1, SQ, SQ + 1, 3 * SQ + 7} <= ns
    big, = cases("clip", big=True)
    assert -(-big.n // SQ) > 1024 and big.n % SQ and big.n % 4
    assert {len(c.lens) for c in cases("ranges")} == {1, 2, 5, 8} and {c.p0 for c in cases("ranges")} == {0, 37}
    for c in cases("ranges"):
        assert all(lo % 4 == 0 for lo, _, _ in inputs_of(c)["pieces"])  # the kernel's alignment contract
    bigw, = cases("adamw", big=True)
    assert bigw.n > 8192 * 256 * 4 and bigw.n % 4 == 0  # the launcher caps the grid at 8192 blocks of 256 threads x 4 elements
    small = cases("adamw")
    for field, values in (("n", {4, 8, 1020, 1024, 1028}), ("lp", {True, False}), ("zg", {0, 1}), ("wd", {0.0, 0.01}), ("step", {1, 2, 1000, 100000}),
                          ("dev", {True, False}), ("gsd", {True, False}), ("betas", {(0.9, 0.98), (0.9, 0.999)})):
        assert {getattr(c, field) for c in small} == values
        for n in () if field == "n" else (4, 8, 1020, 1024, 1028):
            assert {getattr(c, field) for c in small if c.n == n} == values, (n, field)  # every size sees every value of every switch
    c = next(c for c in small if c.n == 1024 and c.wd == 0.0 and c.lp)  # no decay: p' = p where g = m = v = 0, ties of the bf16 rounding
    at = LEAD + np.flatnonzero(inputs_of(c)["zero"])[:4]
    assert UR.bits32(inputs_of(c)["p"][at]).tolist() == [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000]
    assert UR.simulate(c, inputs_of(c), g, "emul")[0]["lp"][at].tolist() == [0x3F80, 0x3F82, 0xBF80, 0xBF82]
    shapes = {(s["rows"], s["cols"]) for c in cases("items") for s in c.launches[-1] if s["kind"] == 1}
    assert {(1, 4), (20, 16), (UR_ - 1, UC - 4), (UR_, UC), (UR_ + 1, UC + 4), (UR_ + 8, UC // 2 + 4), (2 * UR_ + 2, 2 * UC + 4), (UR_, UC // 2)} <= shapes
    for c in cases("items"):
        for rows in inputs_of(c)["lay"]["launches"]:
            for s in rows:
                assert s["off"] % 4 == 0 and s["size"] % 4 == 0
                if s["kind"] == 1:
                    assert s["off"] % 8 == (4 if s["off4"] else 0)


def test_elements_that_could_be_dropped_weigh_enough():
    """the last element and the first element of the last block of every piece: leaving one out moves its block's partial and the norm
    by at least 4 x what the rule allows"""
    for case in cases("clip") + cases("clip", big=True) + cases("ranges"):
        w = UR.weights_sumsq(inputs_of(case), geo())
        assert w >= 4.0, (case, w)


def test_emulation_passes_at_every_case():
    """A correct fp32 implementation stays inside the rule: the op-for-op float32 emulation of every kernel passes verdict() at every
    case of the plan (and so does the fp64 reference rounded to the stored types)."""
    stats = UR.Stats()
    for case in the_plan():
        inp = inputs_of(case)
        fails = UR.verdict(case, inp, geo(), UR.simulate(case, inp, geo(), "emul"), stats)
        assert not fails, (case, fails)
        if not case.big:
            fails = UR.verdict(case, inp, geo(), UR.simulate(case, inp, geo(), "ref"))
            assert not fails, (case, "the rounded reference", fails)
    print({k: (round(a, 3), round(b, 2)) for k, (a, b) in stats.worst.items()})


def test_judge_rejects_every_mutant():
    """verdict() fails every applicable slip, at every case of the plan; every slip applies somewhere."""
    muts = UR.mutants(geo())
    assert [m for m, _ in muts] == UR.MUTANTS
    applied = set()
    for case in the_plan():
        inp = inputs_of(case)
        rejected = []
        for mutant, applies in muts:
            if not applies(case):
                continue
            fails = UR.verdict(case, inp, geo(), UR.simulate(case, inp, geo(), "ref", mutant))
            assert fails, f"{case}: mutant {mutant} passes the criterion"
            rejected.append(mutant)
        applied.update(rejected)
        print(f"{case.id}: rejected {' '.join(rejected) or '-'}")
    assert applied == set(UR.MUTANTS), set(UR.MUTANTS) - applied


# ================================================================================================================ GPU
def _api():
    from joeys2t_amd import _lib, ops
    return _lib, _lib.lib(), ops._stream()


def up(a, device):
    """a numpy buffer (float32, or uint16 bf16 bits) -> the device, bit for bit"""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16).copy() if a.dtype == np.uint16 else a.copy()).to(device)


def down(t):
    if t is None:
        return None
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def clean(t, payload):
    """attn_reference.untouched() on a device buffer (bf16 bits travel as int16): only `payload` (slices) may have changed"""
    if t is None:
        return True
    return untouched(t.view(torch.bfloat16) if t.dtype == torch.int16 else t, [(sl, ) for sl in payload])


def ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())


STATS = {}  # per kernel family: the largest err / allowed and measured K of every output, for the table above


def stats_of(what):
    return STATS.setdefault(what, UR.Stats())


def settle(case, inp, got):
    fails = UR.verdict(case, inp, geo(), got, stats_of(case.op))
    assert not fails, (case.id, fails)


def report(what):
    print(what, {k: (round(a, 3), round(b, 2)) for k, (a, b) in stats_of(what).worst.items()})


def run_sumsq(case, inp, device):
    _lib, L, st = _api()
    p0, nb = inp["p0"], inp["n_blocks"]
    g = up(inp["g"], device)
    part = UR.sent32(p0 + nb + 2 * LEAD)
    part[LEAD:LEAD + p0] = inp["pre"]
    part, out2 = up(part, device), up(UR.sent32(2 + 2 * LEAD), device)
    if case.op == "clip":
        assert L.js2t_sumsq_partials(case.n) == nb
        _lib.check(L.js2t_grad_norm_clip(ptr(g, LEAD), case.n, inp["max_norm"], ptr(part, LEAD), ptr(out2, LEAD), st), "grad_norm_clip")
    else:
        assert nb == sum(L.js2t_sumsq_partials(n) for _, n, _ in inp["pieces"])
        table = torch.tensor([list(row) for row in inp["pieces"]], dtype=torch.int64, device=device)
        _lib.check(L.js2t_sumsq_ranges(ptr(g), ptr(table), len(inp["pieces"]), nb, ptr(part, LEAD), st), "sumsq_ranges")
        _lib.check(L.js2t_norm_clip(ptr(part, LEAD), p0 + nb, inp["max_norm"], ptr(out2, LEAD), st), "norm_clip")
    torch.cuda.synchronize()
    assert clean(part, [slice(LEAD, LEAD + p0 + nb)]) and clean(out2, [slice(LEAD, LEAD + 2)]), "a write outside the partials / out2"
    return dict(partial=down(part), out2=down(out2))


def schedule(h, device):
    """the optional device scalars of a launch and the host arguments that go with them"""
    f = lambda v: torch.tensor([v], dtype=torch.float32, device=device)  # noqa: E731
    gsd = None if h.gsd is None else f(h.gsd)
    lr_dev = f(h.lr) if h.dev else None
    step_dev = torch.tensor([h.step], dtype=torch.int64, device=device) if h.dev else None
    return gsd, lr_dev, step_dev


def run_adamw(case, inp, device):
    _lib, L, st = _api()
    p, m, v, lp = (up(inp[k], device) for k in ("p", "m", "v", "lp"))
    states = []
    for k in range(case.updates):
        h = inp["h"].at(k)
        g = up(inp["gs"][k], device)
        gsd, lr_dev, step_dev = schedule(h, device)
        _lib.check(L.js2t_adamw(ptr(p, LEAD), ptr(g, LEAD), ptr(m, LEAD), ptr(v, LEAD), ptr(lp, LEAD), case.n, h.host_lr, h.b1, h.b2, h.eps, h.wd, h.host_step,
                                ptr(gsd), h.gscale, case.zg, ptr(lr_dev), ptr(step_dev), st), "adamw")
        torch.cuda.synchronize()
        assert all(clean(t, [slice(LEAD, LEAD + case.n)]) for t in (p, g, m, v, lp)), "adamw: a write outside the payload"
        states.append(dict(p=down(p), g=down(g), m=down(m), v=down(v), lp=down(lp)))
    return states


def fold_table(rows, device):
    return torch.tensor(rows, dtype=torch.int64, device=device)


def run_items(case, inp, device):
    """-> (what the launches of js2t_adamw_items left, the same folds written by js2t_fold_ln_weights from the updated buffers)"""
    _lib, L, st = _api()
    lay, h = inp["lay"], inp["h"]
    buf = {k: up(inp[k], device) for k in ("p", "g", "m", "v", "lp", "lp_t")}
    fb = [(up(wf, device), up(bf, device)) for wf, bf in inp["fold_bufs"]]
    fb2 = [(up(wf, device), up(bf, device)) for wf, bf in inp["fold_bufs"]]
    base = buf["p"].data_ptr()

    def rows_of(bufs):
        return [[base + 4 * f["mat"]["off"], base + 4 * f["gamma"], base + 4 * f["beta"], 0 if f["bias"] is None else base + 4 * f["bias"],
                 wf.data_ptr() + 2 * LEAD, bf.data_ptr() + 4 * LEAD, f["N"], f["K"]] for f, (wf, bf) in zip(lay["folds"], bufs)]

    folds = fold_table(rows_of(fb), device) if fb else None
    gsd, lr_dev, step_dev = schedule(h, device)
    for rows, n_units in zip(lay["launches"], lay["n_units"]):
        table = torch.tensor([s["row"] for s in rows], dtype=torch.int64, device=device)
        _lib.check(L.js2t_adamw_items(ptr(buf["p"]), ptr(buf["g"]), ptr(buf["m"]), ptr(buf["v"]), ptr(buf["lp"]), ptr(buf["lp_t"]), ptr(table), len(rows),
                                      n_units, ptr(folds), h.host_lr, h.b1, h.b2, h.eps, h.wd, h.host_step, ptr(gsd), h.gscale, case.zg, ptr(lr_dev),
                                      ptr(step_dev), st), "adamw_items")
    torch.cuda.synchronize()
    pieces = [slice(r["off"], r["off"] + r["size"]) for rows in lay["launches"] for r in rows]
    assert all(clean(buf[k], pieces) for k in ("p", "g", "m", "v", "lp")), "adamw_items: a write outside the pieces"
    assert clean(buf["lp_t"], [slice(r["off"], r["off"] + r["size"]) for r in lay["launches"][-1] if r["kind"] == 1]), "adamw_items: lp_t outside the matrices"
    got = {k: down(t) for k, t in buf.items()}
    got["folds"] = [(down(wf), down(bf)) for wf, bf in fb]
    again = None
    if fb:
        t2 = fold_table(rows_of(fb2), device)
        _lib.check(L.js2t_fold_ln_weights(ptr(t2), len(fb2), max(f["N"] for f in lay["folds"]), st), "fold_ln_weights")
        torch.cuda.synchronize()
        again = [(down(wf), down(bf)) for wf, bf in fb2]
    return got, again


def run_fold(case, inp, device):
    _lib, L, st = _api()
    held, rows = [], []
    fb = [(up(wf, device), up(bf, device)) for wf, bf in inp["fold_bufs"]]
    for e, (wf, bf) in zip(inp["entries"], fb):
        ops_ = [up(e[k], device) for k in ("W", "gamma", "beta", "bias")]
        held.append(ops_)
        rows.append([ops_[0].data_ptr(), ops_[1].data_ptr(), ops_[2].data_ptr(), 0 if ops_[3] is None else ops_[3].data_ptr(), wf.data_ptr() + 2 * LEAD,
                     bf.data_ptr() + 4 * LEAD, e["N"], e["K"]])
    table = fold_table(rows, device)
    max_rows = max(e["N"] for e in inp["entries"])
    assert max_rows % 4 != 0 and len({e["N"] for e in inp["entries"]}) > 1
    _lib.check(L.js2t_fold_ln_weights(ptr(table), len(rows), max_rows, st), "fold_ln_weights")
    torch.cuda.synchronize()
    return dict(folds=[(down(wf), down(bf)) for wf, bf in fb])


@gpu
@pytest.mark.parametrize("clip", ["above", "below", "tiny", "off"])
def test_grad_norm_clip(device, clip):
    """js2t_grad_norm_clip at n around the vector and block edges: every block's partial against the fp64 sum of its block, the norm,
    the coefficient (exactly 1 above the norm and with clipping off; the + 1e-6 visible at a norm of 1e-4)."""
    for case in cases("clip", clip=clip):
        settle(case, inputs_of(case), run_sumsq(case, inputs_of(case), device))
    report("clip")


@gpu
def test_grad_norm_clip_second_stride_trip(device):
    """more than 1024 partials: norm_clip_kernel's stride loop takes a second trip; the last block holds 5 elements"""
    case, = cases("clip", big=True)
    settle(case, inputs_of(case), run_sumsq(case, inputs_of(case), device))
    report("clip")


@gpu
@pytest.mark.parametrize("n_ranges", [1, 2, 5, 8])
def test_sumsq_ranges(device, n_ranges):
    """js2t_sumsq_ranges + js2t_norm_clip over tables of ranges with 1e18 in the gaps, p0 = 0 and 37: each partial against its own
    block, partial[0, p0) (what other kernels left) and everything behind the last partial unchanged."""
    for case in (c for c in cases("ranges") if len(c.lens) == n_ranges):
        settle(case, inputs_of(case), run_sumsq(case, inputs_of(case), device))
    report("ranges")


@gpu
@pytest.mark.parametrize("n", [4, 8, 1020, 1024, 1028])
def test_adamw_small(device, n):
    """js2t_adamw, three successive updates per case: with / without lp, zero_grad, weight decay, both beta pairs, steps 1 .. 100000,
    host and device schedule (the host's lr and step wrong on purpose), with / without *gscale_dev."""
    for case in cases("adamw", n=n):
        settle(case, inputs_of(case), run_adamw(case, inputs_of(case), device))
    report("adamw")


@gpu
def test_adamw_second_grid_trip(device):
    """8192 * 256 * 4 + 12 elements: the grid-stride loop of adamw_kernel takes a second trip of three float4s"""
    case, = cases("adamw", big=True)
    settle(case, inputs_of(case), run_adamw(case, inputs_of(case), device))
    report("adamw")


@gpu
@pytest.mark.parametrize("group", ["flat", "mat", "nine", "mixed", "folds"])
def test_adamw_items(device, group):
    """js2t_adamw_items over tables of flat and matrix items between sentinels: the update of every piece, lp, lp_t = the transpose of
    lp, kept and cleared gradients, the folds from the NEW gamma / beta / bias (the 1-D launch runs first), a fold on a matrix wider
    than a unit untouched; js2t_fold_ln_weights on the updated buffers writes the same bits."""
    for case in (c for c in cases("items") if c.name.startswith(group)):
        inp = inputs_of(case)
        got, again = run_items(case, inp, device)
        settle(case, inp, got)
        for i, f in enumerate(inp["lay"]["folds"]):
            N, K = f["N"], f["K"]
            wf2, bf2 = again[i]
            if f["written"]:
                assert (wf2 == got["folds"][i][0]).all() and (UR.bits32(bf2) == UR.bits32(got["folds"][i][1])).all(), (i, N, K)
            fails = []
            W, gamma, beta, bias = UR._fold_operands(got["p"], f)
            UR.verdict_fold(fails, stats_of("fold"), W, gamma, beta, bias, wf2[LEAD:LEAD + N * K].reshape(N, K), bf2[LEAD:LEAD + N], f" (fold_ln_weights {N} x {K})")
            assert not fails, fails
    report("items")


@gpu
def test_fold_ln_weights(device):
    """js2t_fold_ln_weights, six entries of different N and K (up to five trips of the k loop) in one launch, max_rows = 65"""
    case, = cases("fold")
    settle(case, inputs_of(case), run_fold(case, inputs_of(case), device))
    report("fold")
