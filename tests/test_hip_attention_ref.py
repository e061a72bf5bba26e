"""The fused attention kernels (joeys2t_amd/csrc/attention.hip: flash_fwd_kernel, flash_dq_kernel, flash_dkv_kernel and the merged
flash_bwd_kernel) against exact fp64 attention, at the tile edges, on poisoned inputs (tests/attn_reference.py).

Every comparison goes through attn_reference.judge(): per output row and head the relative L2 error may be 2.5 x what the fp64
emulation of the kernels' own roundings misses (E), or one bf16 ulp (2^-8) where that is larger; lse within 1e-4.  What a kernel
must not read is large (padded keys, guard rows, neighbouring columns), what it must not count twice weighs much (last live key,
last query row), and every output buffer carries sentinels around its payload.  test_reference_criterion_rejects_every_mutant
shows on the CPU that this rule fails each of the plausible slips of attn_reference.MUTANTS at every case.

Measured on MI355X: the largest err / E per kernel over the cases of a family, both head sizes (the rule allows 2.5).  E is
1.2e-3 .. 3.4e-3 for out, 3.1e-3 .. 4.6e-3 for dv, 3.6e-3 .. 0.1 for dq and 3.2e-3 .. 1.8e-2 for dk (the upper ends: rows whose
softmax sits on the planted last key, where the rounding of `out` inside delta = rowsum(dO * O) is the whole error; 0.53 / 0.32 in
case B under dropout, whose second entry has ONE live key and a 16-fold d_out row), 3e-4 .. 3.6e-2 for d_rel (0.52 for the band
of case F with R = 1, where nearly every pair falls into one bin and the bin's true sum cancels).
                                          flash_fwd_kernel      flash_dq_kernel   flash_dkv_kernel     flash_dq_kernel
                                          out    |lse err|      dq                dk       dv          d_rel
    cases A - H, p = 0                    1.02   5e-6           1.00              1.00     1.00
    cases B, D, E, F, p = 0.25            1.00   5e-6           1.00              1.00     1.00
    relative bias, R = 1, 5, 255          1.11   6e-6           1.00              1.00     1.00        1.00  (also deterministic)
    packed rows / packed keys             1.00   3e-6           1.00              1.00     1.00
    chained, delta_partial one grid / two launches (flash_bwd_kernel / the two kernels), case F, p = 0.25:
                                                                1.00              1.00     1.00
The ratios are 1.00 because emulate() rounds where the kernels round: both miss the reference by the same bf16 roundings, fp32
against fp64 arithmetic changes a result bit here and there.  Where the emulation is exact (E = 0: one live key - case A, the
one-key entries of the packed layouts) the printed ratio is inf and the kernels sit within 2^-8 of the median row.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import attn_reference as AR

gpu = pytest.mark.gpu
SITE, SEED = 5, 11


def plan():
    """(case, head size, dropout p, clipping distance R) of every GPU run; the CPU self-check walks the same list."""
    runs = []
    for dh in (128, 64):
        runs += [(n, dh, 0.0, 0) for n in AR.case_names(dh)]
        runs += [(n, dh, 0.25, 0) for n in ("B", "D", "E", "F")]
        runs += [(n, dh, p, R) for n in ("D", "F") for R in (1, 5, 255) for p in (0.0, 0.25)]
    return runs


PLAIN = [r for r in plan() if r[3] == 0]
REL = [r for r in plan() if r[3] != 0]
ids = lambda runs: [f"{n}-dh{dh}-p{p}-R{R}" for n, dh, p, R in runs]  # noqa: E731


# ================================================================================================================ CPU
def test_reference_criterion_rejects_every_mutant():
    """The rule of judge(), fed a mutant of the reference in place of a kernel, fails in at least one row or lse entry - for every
    case of the plan and every mutant that applies to it - while emulate() itself passes everywhere."""
    for name, dh, p, R in plan():
        case = AR.build_case(name, dh, R)
        keep = AR.cpu_keep(case, p) if p else None
        ref = AR.reference(case, case.d_out, keep, p)
        emu = AR.emulate(case, case.d_out, keep, p, o_given=ref["out"].bfloat16())
        names = ["out", "lse", "dq", "dk", "dv"] + (["d_rel"] if R else [])
        ok, ratios, bad = AR.judge_all(emu, ref, emu, case.H, names)
        assert ok, (name, dh, p, R, bad)
        rejected = []
        for mutant, applies in AR.MUTANTS:
            if not applies(case, p):
                continue
            wrong = AR.reference(case, case.d_out, keep, p, mutant=mutant)
            ok, ratios, bad = AR.judge_all(wrong, ref, emu, case.H, names)
            assert not ok, f"{name} dh={dh} p={p} R={R}: mutant {mutant} passes the criterion: {ratios}"
            rejected.append(f"{mutant}[{','.join(b.split(':')[0] for b in bad)}]")
        print(f"{name:5s} dh={dh:3d} p={p:4.2f} R={R:3d}: rejected {' '.join(rejected)}")


def test_reference_matches_torch_sdpa_fp64():
    """A guard against a wrong reference: torch's own attention in fp64 on an unmasked case, forward and gradients."""
    case = AR.build_case("C", 64)
    ref = AR.reference(case, case.d_out)
    B, H, dh = case.B, case.H, case.dh
    heads = lambda x: x.double().view(B, -1, H, dh).transpose(1, 2).detach().requires_grad_(True)  # noqa: E731
    q, k, v = heads(case.q), heads(case.k), heads(case.v)
    out = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, case.Tq, H * dh)
    out.backward(case.d_out.double())
    merge = lambda x: x.transpose(1, 2).reshape(B, -1, H * dh)  # noqa: E731
    torch.testing.assert_close(ref["out"], out.detach(), rtol=1e-11, atol=1e-11)
    for n, t in (("dq", q), ("dk", k), ("dv", v)):
        torch.testing.assert_close(ref[n], merge(t.grad), rtol=1e-10, atol=1e-10)
    lse = torch.logsumexp((q @ k.transpose(2, 3)).detach() / math.sqrt(dh), -1)
    torch.testing.assert_close(ref["lse"], lse, rtol=1e-12, atol=1e-12)


# ================================================================================================================ GPU
def _ops():
    from joeys2t_amd import _lib, ops
    return _lib, ops


class Buffers:
    """The operands of one problem on the device, inside fused buffers (attn_reference.input_buffers)."""

    def __init__(self, cases, device, qrows=None, krows=None):
        cases = cases if isinstance(cases, (list, tuple)) else [cases]
        host = AR.input_buffers(cases)
        self.d = cases[0].d
        self.qrows = qrows or host["qbuf"].shape[0] - AR.GUARD  # packed layouts: the rounded row count
        self.krows = krows or host["kvbuf"].shape[0] - AR.GUARD
        if qrows or krows:  # rows between the last entry and the rounded row count: poison, like the guard rows
            grow = lambda t, rows: torch.cat([t, AR.poison(rows + AR.GUARD - t.shape[0], t.shape[1], 7)]) if rows + AR.GUARD > t.shape[0] else t  # noqa: E731
            host["qbuf"], host["gobuf"] = grow(host["qbuf"], self.qrows), grow(host["gobuf"], self.qrows)
            host["kvbuf"] = grow(host["kvbuf"], self.krows)
        self.q_off, self.k_off, self.v_off = host["q_off"], host["k_off"], host["v_off"]
        self.qbuf, self.kvbuf, self.gobuf = (host[n].to(device) for n in ("qbuf", "kvbuf", "gobuf"))
        self.q, self.kv = self.qbuf[:self.qrows], self.kvbuf[:self.krows]
        self.go = self.gobuf[:self.qrows, 8:8 + self.d]
        self.device = device


def gpu_keep(device, case, p):
    """The kernels' own dropout decisions of (B, H, Tq, Tk, rng, site): the unfused softmax on all-zero scores draws the same mask
    (header; pinned by test_dropout_consistency and test_dropout_rng_statistics).  The keep rate must sit within 3 sigma."""
    _, ops = _ops()
    rng = ops.DropoutRng(device, seed=SEED)
    B, H, Tq, Tk = case.B, case.H, case.Tq, case.Tk
    S = torch.zeros(B * H, Tq, Tk, device=device)
    _, Pd = ops.softmax_fwd(S, None, B, H, Tq, Tk, Tk, p, rng, SITE)
    keep = (Pd != 0).view(B, H, Tq, Tk).cpu()
    q = 1.0 - float(int(p * 65536.0)) / 65536.0
    rate, sigma = keep.double().mean().item(), math.sqrt(q * (1 - q) / keep.numel())
    assert abs(rate - q) <= 3 * sigma, (rate, q, sigma)
    return keep


_PREPARED = {}


def prepared(device, run):
    """case, keep mask, reference and emulation of a run: computed once, shared by every test, never modified."""
    if run not in _PREPARED:
        name, dh, p, R = run
        case = AR.build_case(name, dh, R)
        keep = gpu_keep(device, case, p) if p else None
        go = None if name == "Fdead" else case.d_out
        ref = AR.reference(case, go, keep, p)
        emu = AR.emulate(case, go, keep, p, o_given=ref["out"].bfloat16())
        _PREPARED[run] = (case, keep, ref, emu)
    return _PREPARED[run]


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def forward(buf, geo, mask, p, rng, rel=None, seg=None, seg_keys=False):
    """js2t_flash_attn_fwd into sentinel-filled buffers of the test's own (ops.flash_attn_fwd allocates tight ones): out at column 8
    of a [rows + GUARD, d + 16] buffer, lse with 8 guard floats behind it."""
    _lib, ops = _ops()
    B, H, Tq, Tk, dh = geo
    d, rows = H * dh, buf.qrows
    obuf, lbuf = AR.sentinel_bf16(rows + AR.GUARD, d + 16, buf.device), AR.sentinel_f32(B * H * Tq + 8, buf.device)
    desc = ops._attn_desc(buf.q, buf.q_off, buf.kv, buf.k_off, buf.kv, buf.v_off, B, H, Tq, Tk, dh, mask, p, rng, SITE, rel)
    desc.o, desc.ldo, desc.lse = obuf.data_ptr() + 16, obuf.stride(0), lbuf.data_ptr()
    if seg is not None:
        desc.seg, desc.seg_rows, desc.seg_keys = seg.seg.data_ptr(), seg.rows, int(seg_keys)
    _lib.check(_lib.lib().js2t_flash_attn_fwd(C.byref(desc), ops._stream()), "js2t_flash_attn_fwd")
    torch.cuda.synchronize()
    return obuf, lbuf


def backward(buf, geo, mask, p, rng, out16, lse32, rel=None, d_rel=None, delta_partial=None, seg=None, seg_keys=False):
    """ops.flash_attn_bwd into sentinel-filled fused buffers: dq where q sits in a [rows, 3d + 8] buffer, dk / dv where k / v sit in a
    [rows, 2d + 8] buffer; out16 (bf16 [rows, d], device) travels inside a poisoned buffer of a wider pitch, like d_out."""
    _, ops = _ops()
    B, H, Tq, Tk, dh = geo
    d = H * dh
    obuf = AR.poison(buf.qrows + AR.GUARD, d + 16, 5).to(buf.device)
    obuf[:buf.qrows, 8:8 + d] = out16
    dqbuf = AR.sentinel_bf16(buf.qrows + AR.GUARD, 3 * d + 8, buf.device)
    dkvbuf = AR.sentinel_bf16(buf.krows + AR.GUARD, 2 * d + 8, buf.device)
    ops.flash_attn_bwd(buf.go, obuf[:buf.qrows, 8:8 + d], lse32, buf.q, buf.q_off, buf.kv, buf.k_off, buf.kv, buf.v_off,
                       dqbuf[:buf.qrows], buf.q_off, dkvbuf[:buf.krows], buf.k_off, dkvbuf[:buf.krows], buf.v_off, B, H, Tq, Tk, dh, mask,
                       p, rng, SITE, rel_bias=rel, d_rel_bias=d_rel, delta_partial=delta_partial, seg=seg, seg_keys=seg_keys)
    torch.cuda.synchronize()
    return dqbuf, dkvbuf


def out_payload(buf):
    return [(slice(0, buf.qrows), slice(8, 8 + buf.d))]


def grads_of(buf, dqbuf, dkvbuf):
    """-> dq, dk, dv as float CPU [rows, d] after the sentinel check of both buffers"""
    d = buf.d
    assert AR.untouched(dqbuf, [(slice(0, buf.qrows), slice(buf.q_off, buf.q_off + d))]), "dq: a write outside the head columns / rows"
    assert AR.untouched(dkvbuf, [(slice(0, buf.krows), slice(buf.k_off, buf.k_off + d)), (slice(0, buf.krows), slice(buf.v_off, buf.v_off + d))]), \
        "dk / dv: a write outside the head columns / rows"
    return (dqbuf[:buf.qrows, buf.q_off:buf.q_off + d].float().cpu(), dkvbuf[:buf.krows, buf.k_off:buf.k_off + d].float().cpu(),
            dkvbuf[:buf.krows, buf.v_off:buf.v_off + d].float().cpu())


def geo_of(case):
    return case.B, case.H, case.Tq, case.Tk, case.dh


def dev_mask(case, device):
    return None if case.mask is None else case.mask.to(device)


def report(what, run, ratios):
    print(f"{what} {run}: err/E " + " ".join(f"{k} {v:.2f}" for k, v in ratios.items()))


def check_forward(case, obuf, lbuf, buf, ref, emu, skip=None):
    assert AR.untouched(obuf, out_payload(buf)), "out: a write outside the head columns / rows"
    n = case.B * case.H * case.Tq
    assert AR.untouched(lbuf, [(slice(0, n), )]), "lse: a write behind the last row"
    got = dict(out=obuf[:buf.qrows, 8:8 + buf.d].float().cpu().view(case.B, case.Tq, buf.d), lse=lbuf[:n].cpu().view(case.B, case.H, case.Tq))
    ok, ratios, bad = AR.judge_all(got, ref, emu, case.H, ["out", "lse"], skip)
    assert ok, bad
    return got, ratios


def check_backward(case, buf, dqbuf, dkvbuf, ref, emu, names=("dq", "dk", "dv")):
    dq, dk, dv = grads_of(buf, dqbuf, dkvbuf)
    got = dict(dq=dq.view(case.B, case.Tq, buf.d), dk=dk.view(case.B, case.Tk, buf.d), dv=dv.view(case.B, case.Tk, buf.d))
    dead = ~case.key_live()
    # P is exactly 0 at a masked key and the poison is finite: nothing may reach these rows
    assert (got["dk"][dead] == 0).all() and (got["dv"][dead] == 0).all(), "dk / dv of a masked key is not exactly zero"
    ok, ratios, bad = AR.judge_all(got, ref, emu, case.H, list(names))
    assert ok, bad
    return got, ratios


@gpu
@pytest.mark.parametrize("run", PLAIN + [("Fdead", 128, 0.0, 0), ("Fdead", 64, 0.0, 0)], ids=ids(PLAIN) + ["Fdead-dh128", "Fdead-dh64"])
def test_forward_against_fp64(device, run):
    """out and lse of both forms of the forward kernel (double- and single-buffered: bit-equal) and of ops.flash_attn_fwd."""
    _lib, ops = _ops()
    case, keep, ref, emu = prepared(device, run)
    p = run[2]
    buf, mask = Buffers(case, device), dev_mask(case, device)
    rng = ops.DropoutRng(device, seed=SEED) if p else None
    res = []
    try:
        for mode in (0, 1):
            _lib.lib().js2t_debug_attn_fwd_sb(mode)
            res.append(forward(buf, geo_of(case), mask, p, rng))
    finally:
        _lib.lib().js2t_debug_attn_fwd_sb(-1)
    skip = ~case.live.any(2) if run[0] == "Fdead" else None
    for obuf, lbuf in res:
        got, ratios = check_forward(case, obuf, lbuf, buf, ref, emu, skip)
        if skip is not None:  # a row without live keys: NaN and -inf, as the kernels' header documents
            assert skip.sum() == 2 and got["out"][skip].isnan().all()
            assert (got["lse"].transpose(1, 2)[skip] == float("-inf")).all()
    report("fwd", run, ratios)
    assert torch.equal(bits(res[0][0]), bits(res[1][0])) and torch.equal(bits(res[0][1]), bits(res[1][1]))
    out, lse = ops.flash_attn_fwd(buf.q, buf.q_off, buf.kv, buf.k_off, buf.kv, buf.v_off, *geo_of(case), mask, p, rng, SITE)
    n = case.B * case.H * case.Tq
    assert torch.equal(bits(out), bits(res[0][0][:buf.qrows, 8:8 + buf.d].contiguous())) and torch.equal(bits(lse.flatten()), bits(res[0][1][:n]))


@gpu
@pytest.mark.parametrize("run", PLAIN, ids=ids(PLAIN))
def test_backward_against_fp64(device, run):
    """dq, dk, dv from bf16(reference out) and fp32(reference lse): the backward kernels judged independently of the forward one."""
    _, ops = _ops()
    case, keep, ref, emu = prepared(device, run)
    p = run[2]
    buf, mask = Buffers(case, device), dev_mask(case, device)
    rng = ops.DropoutRng(device, seed=SEED) if p else None
    out16 = ref["out"].bfloat16().view(-1, buf.d).to(device)
    lse32 = ref["lse"].float().view(case.B * case.H, case.Tq).contiguous().to(device)
    dqbuf, dkvbuf = backward(buf, geo_of(case), mask, p, rng, out16, lse32)
    got, ratios = check_backward(case, buf, dqbuf, dkvbuf, ref, emu)
    report("bwd", run, ratios)


@gpu
@pytest.mark.parametrize("dh", [128, 64])
def test_chained_forward_backward_and_delta_partial(device, dh):
    """forward -> backward on the kernel's own out and lse; then delta handed over as partial sums per 64 columns: the one-grid form
    and the two launches each within tolerance and bit-equal to each other."""
    _lib, ops = _ops()
    run = ("F", dh, 0.25, 0)
    case, keep, ref, emu = prepared(device, run)
    buf, mask = Buffers(case, device), dev_mask(case, device)
    rng = ops.DropoutRng(device, seed=SEED)
    obuf, lbuf = forward(buf, geo_of(case), mask, 0.25, rng)
    got, _ = check_forward(case, obuf, lbuf, buf, ref, emu)
    out16 = obuf[:buf.qrows, 8:8 + buf.d].contiguous()
    lse32 = lbuf[:case.B * case.H * case.Tq].view(case.B * case.H, case.Tq).contiguous()
    emu_own = AR.emulate(case, case.d_out, keep, 0.25, o_given=out16.cpu().view(case.B, case.Tq, buf.d))  # delta from the out the backward is handed
    part = (buf.go.float() * out16.float()).view(buf.qrows, buf.d // 64, 64).sum(-1).contiguous()
    res = [backward(buf, geo_of(case), mask, 0.25, rng, out16, lse32), backward(buf, geo_of(case), mask, 0.25, rng, out16, lse32, delta_partial=part)]
    _lib.lib().js2t_debug_attn_bwd_merge(0)
    try:
        res.append(backward(buf, geo_of(case), mask, 0.25, rng, out16, lse32, delta_partial=part))
    finally:
        _lib.lib().js2t_debug_attn_bwd_merge(1)
    for what, (dqbuf, dkvbuf) in zip(("chained", "one grid", "two launches"), res):
        _, ratios = check_backward(case, buf, dqbuf, dkvbuf, ref, emu_own)
        report(f"bwd {what}", run, ratios)
    assert torch.equal(bits(res[1][0]), bits(res[2][0])) and torch.equal(bits(res[1][1]), bits(res[2][1]))


@gpu
@pytest.mark.parametrize("run", REL, ids=ids(REL))
def test_relative_bias_against_fp64(device, run):
    """Relative-position bias, R = 1 (every pair clipped) .. 255 (none): out, lse, dq, dk, dv and the table's gradient, ADDED into a
    non-zero tensor, against the reference exactly - also under dropout, also in deterministic mode."""
    _lib, ops = _ops()
    case, keep, ref, emu = prepared(device, run)
    p = run[2]
    buf, mask, rel = Buffers(case, device), dev_mask(case, device), case.rel.to(device)
    rng = ops.DropoutRng(device, seed=SEED) if p else None
    obuf, lbuf = forward(buf, geo_of(case), mask, p, rng, rel=rel)
    _, ratios = check_forward(case, obuf, lbuf, buf, ref, emu)
    report("fwd rel", run, ratios)
    out16 = ref["out"].bfloat16().view(-1, buf.d).to(device)
    lse32 = ref["lse"].float().view(case.B * case.H, case.Tq).contiguous().to(device)
    pre = torch.randn(case.rel.shape, generator=torch.Generator().manual_seed(8))
    try:
        for det in (0, 1):
            _lib.lib().js2t_set_deterministic(det)
            d_rel = pre.to(device)
            dqbuf, dkvbuf = backward(buf, geo_of(case), mask, p, rng, out16, lse32, rel=rel, d_rel=d_rel)
            _, ratios = check_backward(case, buf, dqbuf, dkvbuf, ref, emu)
            ok, ratio, text = AR.judge("table", d_rel.cpu().double() - pre.double(), ref["d_rel"], emu["d_rel"])
            assert ok, f"d_rel (deterministic {det}): {text}"
            ratios["d_rel"] = ratio
            report(f"bwd rel det={det}", run, ratios)
    finally:
        _lib.lib().js2t_set_deterministic(0)


def _packed_check(cases, got, ref_names, H):
    """every entry against the reference of that entry ALONE"""
    worst = {}
    for c, g in zip(cases, got):
        ref = AR.reference(c, c.d_out)
        emu = AR.emulate(c, c.d_out, o_given=ref["out"].bfloat16())
        ok, ratios, bad = AR.judge_all(g, ref, emu, H, ref_names)
        assert ok, (c.name, bad)
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


@gpu
@pytest.mark.parametrize("dh", [128, 64])
def test_packed_self_attention(device, dh):
    """Self-attention over packed rows (js2t_attn_desc.seg), lengths [KT+1, 1, 64, 17]: rows no entry owns come out exactly zero."""
    _, ops = _ops()
    KT, H = AR.key_tile(dh), 2
    lens, T = [KT + 1, 1, 64, 17], KT + 1
    cases = [AR.make_case(f"packed{n}", dh, 40 + i, 1, H, n, n) for i, n in enumerate(lens)]
    seg = ops.PackedRows.from_lengths(lens, T, device, round_to=64)
    assert seg.rows > sum(lens)
    buf = Buffers(cases, device, qrows=seg.rows, krows=seg.rows)
    # self-attention: q, k, v of a row live in ONE buffer in the product; here k / v rows sit in the second buffer at the same rows
    geo, d, B = (len(lens), H, T, T, dh), H * dh, len(lens)
    obuf, lbuf = forward(buf, geo, None, 0.0, None, seg=seg)
    assert AR.untouched(obuf, out_payload(buf))
    out = obuf[:seg.rows, 8:8 + d].float().cpu()
    lse = lbuf[:B * H * T].cpu().view(B, H, T)
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    # lse of positions behind an entry's length is not written
    assert AR.untouched(lbuf, [(slice((b * H + h) * T, (b * H + h) * T + n), ) for b, n in enumerate(lens) for h in range(H)])
    out16 = torch.zeros(seg.rows, d, dtype=torch.bfloat16)
    lse32 = torch.zeros(B * H, T)
    refs = [AR.reference(c) for c in cases]
    for b, (c, r) in enumerate(zip(cases, refs)):
        out16[off[b]:off[b + 1]] = r["out"][0].bfloat16()
        lse32.view(B, H, T)[b, :, :lens[b]] = r["lse"][0].float()
    dqbuf, dkvbuf = backward(buf, geo, None, 0.0, None, out16.to(device), lse32.to(device), seg=seg)
    dq, dk, dv = grads_of(buf, dqbuf, dkvbuf)
    for t in (out, dq, dk, dv):
        assert (t[off[-1]:] == 0).all(), "rows behind the last entry are not exactly zero"
    got = [dict(out=out[off[b]:off[b + 1]][None], lse=lse[b:b + 1, :, :lens[b]], dq=dq[off[b]:off[b + 1]][None], dk=dk[off[b]:off[b + 1]][None],
                dv=dv[off[b]:off[b + 1]][None]) for b in range(B)]
    report("packed self", dh, _packed_check(cases, got, ["out", "lse", "dq", "dk", "dv"], H))
    o2, l2 = ops.flash_attn_fwd(buf.q, buf.q_off, buf.kv, buf.k_off, buf.kv, buf.v_off, *geo, None, 0.0, None, SITE, seg=seg)
    assert torch.equal(bits(o2), bits(obuf[:seg.rows, 8:8 + d].contiguous()))


@gpu
@pytest.mark.parametrize("dh", [128, 64])
def test_packed_keys_cross_attention(device, dh):
    """Cross-attention over packed KEYS (seg_keys), key lengths [1, KT, KT+1], padded queries: dk / dv rows no entry owns exactly zero."""
    _, ops = _ops()
    KT, H, Tq = AR.key_tile(dh), 2, 17
    lens, Tk = [1, KT, KT + 1], KT + 1
    cases = [AR.make_case(f"cross{n}", dh, 60 + i, 1, H, Tq, n) for i, n in enumerate(lens)]
    seg = ops.PackedRows.from_lengths(lens, Tk, device, round_to=64)
    assert seg.rows > sum(lens)
    buf = Buffers(cases, device, krows=seg.rows)
    geo, d, B = (len(lens), H, Tq, Tk, dh), H * dh, len(lens)
    obuf, lbuf = forward(buf, geo, None, 0.0, None, seg=seg, seg_keys=True)
    assert AR.untouched(obuf, out_payload(buf)) and AR.untouched(lbuf, [(slice(0, B * H * Tq), )])
    out = obuf[:B * Tq, 8:8 + d].float().cpu().view(B, Tq, d)
    lse = lbuf[:B * H * Tq].cpu().view(B, H, Tq)
    refs = [AR.reference(c) for c in cases]
    out16 = torch.cat([r["out"][0] for r in refs]).bfloat16().to(device)
    lse32 = torch.cat([r["lse"][0] for r in refs]).float().contiguous().to(device)
    dqbuf, dkvbuf = backward(buf, geo, None, 0.0, None, out16, lse32, seg=seg, seg_keys=True)
    dq, dk, dv = grads_of(buf, dqbuf, dkvbuf)
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    assert (dk[off[-1]:] == 0).all() and (dv[off[-1]:] == 0).all(), "dk / dv rows behind the last entry are not exactly zero"
    got = [dict(out=out[b:b + 1], lse=lse[b:b + 1], dq=dq.view(B, Tq, d)[b:b + 1], dk=dk[off[b]:off[b + 1]][None], dv=dv[off[b]:off[b + 1]][None])
           for b in range(B)]
    report("packed keys", dh, _packed_check(cases, got, ["out", "lse", "dq", "dk", "dv"], H))
