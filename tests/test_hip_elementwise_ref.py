"""The element-wise and data-movement kernels (joeys2t_amd/csrc/elementwise.hip) against plain fp64 references, at the vector and
grid edges, on poisoned inputs (tests/elementwise_reference.py).

Every comparison goes through elementwise_reference.judge(): an element passes when |got - ref| <= u_out |ref| + K 2^-24 cond + floor
(u_out = 2^-8 bf16 / 2^-24 fp32, cond = the sum of |terms added|, floor = 2^-126); rounding and move kernels must match bit for
bit.  K is derived from the kernel's operation count (K_DERIVED, the count stands next to each number) or, for the kernels that
call __expf / erff / tanhf, measured on the MI355X and asserted at twice that, rounded up to a power of two (K_MEASURED).  Outputs
live between sentinels in buffers of the test's own, and untouched() is asserted after every launch; what a kernel must not read is
large, what it must not drop or count twice weighs 16 x the rest.  test_judge_rejects_every_mutant shows on the CPU that the rule
fails each slip of elementwise_reference.MUTANTS at every case it applies to.

Measured on MI355X: the largest err / allowed per kernel over its cases, small and second-trip (the rule allows 1), and the largest
measured K = max (err - u_out |ref| - floor) / (2^-24 cond) next to the K the rule uses.
    kernel                       err / allowed      measured K (f32 cases)   K used
                                 f32      bf16
    axpby                        0.46     1.00      0.85                     3   derived
    glu_fwd                      0.52     1.00      7.82                     16  = 2 x measured, rounded up
    glu_bwd                      0.32     1.00      9.70                     32  = 2 x measured, rounded up
    add_pe_dropout               0.56     1.00      2.36                     5   derived
    dropout_bwd                  0.44     0.88      0.75                     3   derived
    act_bwd relu                 0.33     0.98      0                        2   derived
    act_bwd hardswish            0.36     0.98      1.52                     6   derived
    act_bwd gelu                 0.38     1.00      2.41                     8   = 2 x measured, rounded up
    act_bwd swish                0.34     0.95      4.98                     16  = 2 x measured, rounded up
    act_bwd tanh                 0.52     0.96      0.87                     2   = 2 x measured, rounded up
    embed_fwd, scale 16.25       0.50     1.00      0                        1   derived       (scale 1: bit-exact)
    embed_bwd atomic / ordered   0.36               3.51                     1 + multiplicity  (30 in the 600-id case)
    colsum                       0.06               0.97                     24  derived       (both bf16 routes bit-equal)
    col2im                       0.45     1.00      0.80                     3   derived       (both bf16 kernels bit-equal)
    conv_weight_unpack_grad      0.50               0                        1   derived       (without accumulate: bit-exact)
    cast, im2col, conv_weight_pack, transpose_groups, absmax, quantize_fp8 (bytes): bit-exact; quantize_fp8 scale: 0 (K 2)
bf16: 1.00 (0.996) is a correctly rounded store just above a power of two - the rounding alone may use all of 2^-8 |ref|.  The
measured K of the __expf kernels grows with the gate: v_exp_f32 sees b log2(e) rounded to fp32, an error of |b| 2^-24 relative to
the exponential (7.8 at |b| = 8).

Which GPU case fails if a slip of MUTANTS were put into the kernel (the CPU self-check shows the rule rejects it there):
    bf16_store_truncates            every bf16 case; bit for bit at cast f32 -> bf16 (ties both ways), conv_weight_pack, embed_fwd scale 1
    glu_halves_swapped              glu_fwd / glu_bwd, every C with valid_t > 0
    glu_crop_le                     valid_t in {0, 1, 6}: position t == valid_t holds poison and must come out exactly 0
    glu_crop_by_row                 valid_t in {1, 6, 7}, B = 3: the second and third entry would come out all zero
    pe_by_row                       add_pe_dropout with pe, B = 3: rows >= T of the pe buffer are poison
    extra_dropped                   add_pe_dropout with extra
    dropout_scale_missing           add_pe_dropout / dropout_bwd, p in {0.1, 0.25}: every kept value off by 1 / (1 - p)
    keep_bits_reversed              the same cases: zeros where the twin keeps (exact check of the mask against the twin)
    mask_as_if_cols_multiple_of_4   dropout_bwd, cols in {5, 258}, and the second-trip case (cols = 199875)
    swish_without_z_term            act_bwd swish;   gelu_tanh_approx: act_bwd gelu, f32
    embed_fwd_without_scale         embed_fwd at scale 16.25
    embed_oob_reads_row0            ids -1 and `vocab`: table row 0 is poison, the output rows must be 0
    embed_bwd_adds_pad_row          dout rows of the pad id are poison, table row PAD must keep its value (both modes)
    embed_bwd_last_duplicate_only   about 15 positions per id, the last one 16 x (both modes); id 45 at positions 3 and 515
    colsum_drops_partial_slab       rows in {1, 3, 63, 65, 257, 833}: the last row weighs 16 x
    colsum_drops_a_row_lane         every rows >= 4;   colsum_ignores_accumulate: accumulate into a non-zero out
    col2im_no_stride_test           the stride-2 geometries;   col2im_pad_off_by_one: every col2im case
    col2im_no_tout_test             e.g. (K, stride, pad) = (3, 2, 1), tin = 36: t == tout reads the next entry's first row (100 x) / the guard
    im2col_tau_le_tin               the geometries with a tap on tau == tin, e.g. (5, 2, 2) at tin = 36: the next entry's row instead of 0
    grid_stride_stops               test_second_grid_stride_trip: the sentinels (NaN) stay in the payload behind work item 4096 * 256
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import elementwise_reference as ER
from attn_reference import poison, sentinel_bf16, sentinel_f32, untouched

gpu = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
PLAN = ER.plan()
SMALL = [c for c in PLAN if not c.big]
BIGS = [c for c in PLAN if c.big]
OPS = sorted({c.op for c in SMALL})
LEAD = 64  # elements in front of every payload: keeps 16-byte alignment for both types; `shift` then breaks it on purpose


# ================================================================================================================ CPU
def test_judge_rejects_every_mutant():
    """judge() passes the reference rounded to the output type and fails every applicable mutant, at every case of the plan."""
    for case in PLAN:
        inp = ER.inputs(case)
        outs = ER.reference(case, inp)
        for name, out in outs.items():
            ok, ratio, text = ER.judge(ER.as_stored(out), out)
            assert ok, (case, name, text)
        rejected = []
        for mutant, applies in ER.MUTANTS:
            if not applies(case):
                continue
            wrong = ER.reference(case, inp, mutant=mutant)
            bad = [n for n, out in outs.items() if not ER.judge(ER.as_stored(wrong[n], mutant == "bf16_store_truncates"), out)[0]]
            assert bad, f"{case}: mutant {mutant} passes the criterion"
            rejected.append(mutant)
        print(f"{case.id}: rejected {' '.join(rejected) or '-'}")
    applied = {m for m, applies in ER.MUTANTS if any(applies(c) for c in PLAN)}
    assert applied == {m for m, _ in ER.MUTANTS}, "a mutant applies to no case of the plan"


def test_reference_matches_closed_forms_fp64():
    """A guard against a wrong reference: the gradients the reference takes from autograd of F.glu / F.silu / F.gelu / torch.tanh /
    F.hardswish against their closed forms, written out independently, in fp64 (also at the kinks)."""
    z = torch.cat([torch.linspace(-8, 8, 4001, dtype=torch.float64), torch.tensor([0.0, 3.0, -3.0], dtype=torch.float64)])
    s, t = torch.sigmoid(z), torch.tanh(z)
    closed = {"relu": (z > 0).double(), "swish": s * (1 + z * (1 - s)), "tanh": 1 - t * t,
              "gelu": 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi),
              "hardswish": torch.where(z <= -3, torch.zeros_like(z), torch.where(z >= 3, torch.ones_like(z), (2 * z + 3) / 6))}
    for act, want in closed.items():
        grad, terms = ER.act_grad_ref(z, act)
        torch.testing.assert_close(grad, want, rtol=1e-12, atol=1e-14)
        assert (terms >= grad.abs() * (1 - 1e-12)).all(), act  # the sum of |terms| bounds the |sum|
    assert closed["hardswish"][-2:].tolist() == [1.0, 0.0] and closed["relu"][-3] == 0
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(21, 10, generator=g, dtype=torch.float64), torch.randn(21, 5, generator=g, dtype=torch.float64)
    y, dx, _, _ = ER.glu_ref(x, dy, 3, 7, 7)
    a, b = x[:, :5], x[:, 5:]
    sb = torch.sigmoid(b)
    torch.testing.assert_close(y, a * sb, rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(dx, torch.cat([dy * sb, dy * a * sb * (1 - sb)], 1), rtol=1e-13, atol=1e-14)
    y, dx, _, _ = ER.glu_ref(x, dy, 3, 7, 2)
    live = (torch.arange(21) % 7 < 2)
    assert (y[~live] == 0).all() and (dx[~live] == 0).all() and (y[live] != 0).all()


def test_reference_im2col_matches_unfold_and_col2im_is_its_adjoint():
    g = torch.Generator().manual_seed(4)
    for K, stride, pad in ER.GEOS + ((7, 1, 3), ):
        for tin in (1, 2, 36, 37):
            B, Cc = 3, 8
            x = torch.randn(B, tin, Cc, generator=g, dtype=torch.float64)
            col = ER.im2col_ref(x, K, stride, pad)  # [B, tout, K, C]
            tout = ER.tout_of(tin, K, stride, pad)
            unf = F.unfold(x.transpose(1, 2).unsqueeze(-1), (K, 1), padding=(pad, 0), stride=(stride, 1))  # [B, C * K, tout]
            assert torch.equal(col, unf.view(B, Cc, K, tout).permute(0, 3, 2, 1))
            d = torch.randn(B, tout, K, Cc, generator=g, dtype=torch.float64)
            dx, cond = ER.col2im_ref(d, tin, K, stride, pad)
            torch.testing.assert_close((col * d).sum(), (x * dx).sum(), rtol=1e-12, atol=1e-12)  # <im2col x, d> = <x, col2im d>
            torch.testing.assert_close(dx, F.fold(d.permute(0, 3, 2, 1).reshape(B, Cc * K, tout), (tin, 1), (K, 1), padding=(pad, 0),
                                                  stride=(stride, 1)).squeeze(-1).transpose(1, 2), rtol=1e-12, atol=1e-12)
            assert (cond >= dx.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("p", [0.1, 0.25])
def test_rng_twin_keep_rate(p):
    """The numpy twin of the dropout generator keeps within 3 sigma of 1 - floor(p 65536) / 65536."""
    keep = ER.keep_mask(512, 1027, p)
    q = 1.0 - float(int(p * 65536.0)) / 65536.0
    rate, sigma = keep.double().mean().item(), math.sqrt(q * (1 - q) / keep.numel())
    assert abs(rate - q) <= 3 * sigma, (rate, q, sigma)
    assert not torch.equal(keep, ER.keep_mask(512, 1027, p, site=ER.SITE + 1)) and not torch.equal(keep, ER.keep_mask(512, 1027, p, offset=ER.OFFSET + 1))


# ================================================================================================================ GPU
def _ops():
    from joeys2t_amd import _lib, ops
    return _lib, ops


def code(dt):
    return 1 if dt == BF16 else 0


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def in_buf(t, device, shift=0, behind=None, seed=31):
    """a contiguous operand inside a poisoned buffer (`behind`: given rows right after it) -> the device view of the operand"""
    if t is None:
        return None
    flat = t.reshape(-1)
    tail = [poison(1, 512, seed + 1).flatten().to(t.dtype)] if behind is None else [behind.reshape(-1).to(t.dtype)]
    buf = torch.cat([poison(1, LEAD + shift, seed).flatten().to(t.dtype), flat] + tail).to(device)
    return buf[LEAD + shift:LEAD + shift + flat.numel()]


class OutBuf:
    """n elements between sentinels: 8 + 3 guard rows in front (LEAD + shift elements in all) and behind"""

    def __init__(self, n, dtype, device, cols=8, shift=0, fill=None):
        self.lo, self.n = LEAD + shift, n
        total = self.lo + n + 8 + 3 * min(cols, 2048)
        self.buf = sentinel_bf16(1, total, device).flatten() if dtype == BF16 else sentinel_f32(total, device)
        self.view = self.buf[self.lo:self.lo + n]
        if fill is not None:
            self.view.copy_(fill.reshape(-1).to(device))

    def result(self, what):
        torch.cuda.synchronize()
        assert untouched(self.buf, [(slice(self.lo, self.lo + self.n), )]), f"{what}: a write outside the payload"
        return self.view.cpu()


def rng_state(device):
    return torch.tensor([ER.SEED, ER.OFFSET], dtype=torch.int64, device=device)


def run(case, inp, device, shift=0):
    """One launch of the case's C entry point into sentinel-guarded buffers -> {output name: CPU tensor}"""
    _lib, ops = _ops()
    L, st, op = _lib.lib(), ops._stream(), case.op
    dt = getattr(case, "dt", F32)
    I = lambda t, **kw: in_buf(t, device, **kw)  # noqa: E731, E741
    if op == "cast":
        src = I(inp["src"], shift=shift)
        n = src.numel()
        o = OutBuf(n, case.dst, device)
        _lib.check(L.js2t_cast(ptr(src), code(case.src), ptr(o.view), code(case.dst), n, st), op)
        return dict(dst=o.result(op))
    if op == "axpby":
        x, y, o = I(inp["x"]), I(inp["y"]), OutBuf(case.n, dt, device)
        _lib.check(L.js2t_axpby(ptr(x), inp["a"], ptr(y), inp["b"], ptr(o.view), case.n, code(dt), st), op)
        return dict(out=o.result(op))
    if op in ("glu_fwd", "glu_bwd"):
        rows, Cc = case.B * case.T, case.C
        x, dy, vt = I(inp["x"]), I(inp["dy"]), torch.tensor([case.vt], dtype=torch.int64, device=device)
        if op == "glu_fwd":
            o = OutBuf(rows * Cc, dt, device, Cc)
            _lib.check(L.js2t_glu_fwd_crop(ptr(x), ptr(o.view), rows, Cc, case.T, ptr(vt), code(dt), st), op)
            return dict(y=o.result(op).view(rows, Cc))
        o = OutBuf(rows * 2 * Cc, dt, device, 2 * Cc)
        _lib.check(L.js2t_glu_bwd_crop(ptr(x), ptr(dy), ptr(o.view), rows, Cc, case.T, ptr(vt), code(dt), st), op)
        return dict(dx=o.result(op).view(rows, 2 * Cc))
    if op == "add_pe_dropout":
        B, T, D = case.B, case.T, case.D
        x, pe, extra, o = I(inp["x"]), I(inp["pe"]), I(inp["extra"]), OutBuf(B * T * D, dt, device, D)
        state = rng_state(device)
        _lib.check(L.js2t_add_pe_dropout(ptr(x), ptr(pe), ptr(extra), ptr(o.view), B, T, D, code(dt), case.p, ptr(state) if case.p > 0 else None,
                                         ER.SITE, st), op)
        return dict(y=o.result(op).view(B * T, D))
    if op == "dropout_bwd":
        dy, o, state = I(inp["dy"]), OutBuf(case.rows * case.cols, dt, device, case.cols), rng_state(device)
        _lib.check(L.js2t_dropout_bwd(ptr(dy), ptr(o.view), case.rows, case.cols, code(dt), case.p, ptr(state), ER.SITE, st), op)
        return dict(dx=o.result(op).view(case.rows, case.cols))
    if op == "act_bwd":
        dh, z, o = I(inp["dh"]), I(inp["z"]), OutBuf(case.n, dt, device)
        _lib.check(L.js2t_act_bwd(ptr(dh), ptr(z), ptr(o.view), case.n, ER.ACTS[case.act], code(dt), case.scale, st), op)
        return dict(dz=o.result(op))
    if op == "embed_fwd":
        ids, table, o = inp["ids"].to(device), I(inp["table"]), OutBuf(case.n_ids * case.D, case.out, device, case.D)
        _lib.check(L.js2t_embed_fwd(ptr(ids), ptr(table), code(dt), ptr(o.view), code(case.out), case.n_ids, case.D, case.vocab, case.scale, st), op)
        return dict(out=o.result(op).view(case.n_ids, case.D))
    if op == "embed_bwd":
        ids, dout = inp["ids"].to(device), I(inp["dout"])
        o = OutBuf(case.vocab * case.D, F32, device, case.D, fill=inp["pre"])
        _lib.check(L.js2t_embed_bwd(ptr(ids), ptr(dout), code(dt), ptr(o.view), case.n_ids, case.D, case.vocab, case.scale, ER.PAD, st), op)
        return dict(dtable=o.result(op).view(case.vocab, case.D))
    if op == "colsum":
        rows, cols = case.rows, case.cols
        x, o = I(inp["x"], shift=shift), OutBuf(cols, F32, device, cols, fill=inp["pre"])
        part = OutBuf(L.js2t_colsum_partial_rows(rows) * cols, F32, device, cols)
        _lib.check(L.js2t_colsum(ptr(x), code(dt), ptr(o.view), ptr(part.view), rows, cols, int(case.acc), st), op)
        part.result("colsum partial")
        return dict(out=o.result(op))
    if op in ("im2col", "col2im"):
        K, stride, pad = case.geo
        B, tin, Cc = case.B, case.tin, case.C
        tout = ER.tout_of(tin, K, stride, pad)
        if op == "im2col":
            x, o = I(inp["x"], behind=ER.im2col_guard(case)), OutBuf(B * tout * K * Cc, dt, device, K * Cc)
            _lib.check(L.js2t_im2col(ptr(x), ptr(o.view), B, tin, tout, Cc, K, stride, pad, code(dt), st), op)
            return dict(col=o.result(op).view(B, tout, K, Cc))
        x, o = I(inp["x"], shift=shift, behind=ER.col2im_guard(case)), OutBuf(B * tin * Cc, dt, device, Cc, shift=shift)
        _lib.check(L.js2t_col2im(ptr(x), ptr(o.view), B, tin, tout, Cc, K, stride, pad, code(dt), st), op)
        return dict(dx=o.result(op).view(B, tin, Cc))
    if op == "conv_weight_pack":
        cout, cin, k = case.shape
        w, o = I(inp["w"]), OutBuf(cout * cin * k, dt, device, cin * k)
        _lib.check(L.js2t_conv_weight_pack(ptr(w), ptr(o.view), code(dt), cout, cin, k, st), op)
        return dict(wp=o.result(op).view(cout, k, cin))
    if op == "conv_weight_unpack_grad":
        cout, cin, k = case.shape
        src, o = I(inp["dwp_t"]), OutBuf(cout * cin * k, F32, device, cin * k, fill=inp["pre"] if case.acc else None)
        _lib.check(L.js2t_conv_weight_unpack_grad(ptr(src), ptr(o.view), cout, cin, k, int(case.acc), st), op)
        return dict(dw=o.result(op).view(cout, cin, k))
    if op == "quantize":
        n = case.n
        x, mul = I(inp["x"]), inp["mul"].to(device)
        amax, scale = OutBuf(1, F32, device), OutBuf(1, F32, device)
        ybuf = torch.full((LEAD + n + 64, ), 0xA5, dtype=torch.uint8, device=device)
        _lib.check(L.js2t_absmax(ptr(x), code(dt), n, ptr(amax.view), st), "absmax")
        _lib.check(L.js2t_quantize_fp8(ptr(x), code(dt), ptr(ybuf[LEAD:]), n, ptr(amax.view), ptr(mul), ptr(scale.view), st), op)
        torch.cuda.synchronize()
        y = ybuf.cpu()
        assert (y[:LEAD] == 0xA5).all() and (y[LEAD + n:] == 0xA5).all(), "quantize_fp8: a write outside the payload"
        return dict(amax=amax.result("absmax"), y=y[LEAD:LEAD + n], scale=scale.result(op))
    raise KeyError(op)


WORST = {}


def check(case, device, inp=None, outs=None, **kw):
    """run + judge every output + the exact side conditions of the case -> {name: got}"""
    inp = ER.inputs(case) if inp is None else inp
    outs = ER.reference(case, inp) if outs is None else outs
    got = run(case, inp, device, **kw)
    for name, out in outs.items():
        ok, ratio, text = ER.judge(got[name], out)
        key = (case.op + ("-" + case.act if case.op == "act_bwd" else ""), str(out.dtype))
        k = ER.measured_K(got[name], out) if out.K else 0.0
        was = WORST.get(key, (0.0, 0.0))
        WORST[key] = (max(was[0], ratio), max(was[1], k))  # largest err / allowed, largest measured K
        print(f"{case.id} {name}: {text}" + (f", measured K {k:.2f}" if out.K else ""))
        assert ok, f"{case.id} {name}: {text}"
    if case.op in ("glu_fwd", "glu_bwd"):  # cropped positions: exactly 0 whatever the poison there
        dead = (torch.arange(case.B * case.T) % case.T) >= case.vt
        assert (next(iter(got.values()))[dead].float() == 0).all(), f"{case.id}: a cropped position is not exactly zero"
    if case.op in ("add_pe_dropout", "dropout_bwd") and case.p > 0:  # the mask is the twin's, bit for bit
        (name, g), = got.items()
        keep = ER.keep_mask(g.shape[0], g.shape[1], case.p)
        live = keep & (outs[name].ref != 0)  # (x + extra cancels exactly at a few bf16 elements)
        assert (g[~keep].float() == 0).all() and (g[live].float() != 0).all(), f"{case.id}: keep mask differs from the twin's"
    return got


@gpu
@pytest.mark.parametrize("op", OPS)
def test_small_cases_against_fp64(device, op):
    """Every small case of the plan (odd sizes, every argument form, both types) of one kernel family."""
    for case in (c for c in SMALL if c.op == op):
        check(case, device)
    print({k: v for k, v in WORST.items() if k[0].startswith(op)})


@gpu
@pytest.mark.parametrize("case", BIGS, ids=[c.id for c in BIGS])
def test_second_grid_stride_trip(device, case):
    """4096 * 256 + 773 work items: the grid-stride loop takes a second, partial trip (cast: + 3 elements for the scalar tail)."""
    check(case, device)
    print({k: v for k, v in WORST.items() if k[0].startswith(case.op)})


@gpu
@pytest.mark.parametrize("dt", ER.DTS, ids=["f32", "bf16"])
def test_dropout_bwd_draws_the_forward_mask(device, dt):
    """dropout_bwd at the state and site of add_pe_dropout with cols == D zeroes the same elements."""
    for p in (0.1, 0.25):
        fwd = ER.Case("add_pe_dropout", dt=dt, B=3, T=5, D=260, pe=False, extra=False, p=p)
        bwd = ER.Case("dropout_bwd", dt=dt, rows=15, cols=260, p=p)
        y = check(fwd, device)["y"]
        dx = check(bwd, device)["dx"]
        assert torch.equal(y != 0, dx != 0)


@gpu
@pytest.mark.parametrize("dt", ER.DTS, ids=["f32", "bf16"])
def test_embed_bwd_atomic_and_ordered(device, dt):
    """embed_bwd adds into a non-zero table, with atomics and in deterministic mode; the ordered form twice is bit-equal."""
    _lib, _ = _ops()
    case = next(c for c in SMALL if c.op == "embed_bwd" and c.dt == dt)
    inp = ER.inputs(case)
    outs = ER.reference(case, inp)
    assert int(torch.bincount(inp["ids"][(inp["ids"] >= 2) & (inp["ids"] < 50)]).max()) > 8 and (inp["ids"] == 45).nonzero().flatten().tolist() == [3, 515]
    check(case, device, inp, outs)
    try:
        _lib.lib().js2t_set_deterministic(1)
        a = check(case, device, inp, outs)["dtable"]
        b = check(case, device, inp, outs)["dtable"]
    finally:
        _lib.lib().js2t_set_deterministic(0)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@gpu
def test_colsum_bf16_vector_and_scalar_routes_bit_equal(device):
    """bf16, cols % 8 == 0: the payload at a 16-byte aligned offset (8 columns per thread) and at one that is not (scalar kernel)."""
    for case in (c for c in SMALL if c.op == "colsum" and c.dt == BF16 and c.cols % 8 == 0):
        inp = ER.inputs(case)
        outs = ER.reference(case, inp)
        a = check(case, device, inp, outs, shift=8)["out"]
        b = check(case, device, inp, outs, shift=1)["out"]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), case


@gpu
def test_col2im_bf16_vector_and_scalar_kernels_bit_equal(device):
    for case in (c for c in SMALL if c.op == "col2im" and c.dt == BF16):
        inp = ER.inputs(case)
        outs = ER.reference(case, inp)
        a = check(case, device, inp, outs, shift=8)["dx"]
        b = check(case, device, inp, outs, shift=1)["dx"]
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), case


@gpu
@pytest.mark.parametrize("src,dst", [(s, d) for s in ER.DTS for d in ER.DTS], ids=lambda d: "bf16" if d == BF16 else "f32")
def test_cast_from_a_view_that_starts_anywhere(device, src, dst):
    """js2t_cast of a view that starts at element 1 / 2 of an aligned buffer (and into one): all scalar, same bits."""
    _lib, ops = _ops()
    for n in (5, 1027):
        case = ER.Case("cast", src=src, dst=dst, n=n)
        inp = ER.inputs(case)
        outs = ER.reference(case, inp)
        for shift in (1, 2):
            check(case, device, inp, outs, shift=shift)
            s = in_buf(inp["src"], device)
            o = OutBuf(n, dst, device, shift=shift)
            _lib.check(_lib.lib().js2t_cast(ptr(s), code(src), ptr(o.view), code(dst), n, ops._stream()), "cast")
            assert ER.judge(o.result("cast"), outs["dst"])[0]
            base = inp["src"].to(device)
            assert ER.same_bits(ops.cast(torch.cat([base[:shift], base])[shift:], dst).cpu(), outs["dst"].expected)


@gpu
@pytest.mark.parametrize("dt", ER.DTS, ids=["f32", "bf16"])
def test_add_pe_dropout_rejects_misaligned_pointers(device, dt):
    """x, extra, y or pe not aligned to four elements: JS2T_ERR_INVALID like D % 4 != 0, nothing is launched."""
    _lib, ops = _ops()
    B, T, D = 2, 3, 8
    mk = lambda t, shift: in_buf(t, device, shift=shift)  # noqa: E731
    x, e, pe = torch.randn(B * T, D).to(dt), torch.randn(B * T, D).to(dt), torch.randn(T, D)
    for bad in ("x", "extra", "y", "pe", None):
        o = OutBuf(B * T * D, dt, device, D, shift=1 if bad == "y" else 0)
        held = [mk(x, bad == "x"), mk(pe, bad == "pe"), mk(e, bad == "extra")]
        args = (*(ptr(t) for t in held), ptr(o.view), B, T, D, code(dt), 0.0, None, ER.SITE, ops._stream())
        if bad is None:
            _lib.check(_lib.lib().js2t_add_pe_dropout(*args), "add_pe_dropout")
            assert not untouched(o.buf, [])
            continue
        with pytest.raises(_lib.Js2tError, match="aligned"):
            _lib.check(_lib.lib().js2t_add_pe_dropout(*args), "add_pe_dropout")
        torch.cuda.synchronize()
        assert untouched(o.buf, []), bad


@gpu
def test_transpose_groups_vector_and_scalar_paths(device):
    """One launch over groups (64, 64), (72, 136), (7, 65), (1, 1), (130, 3) with poisoned gaps: the odd-shaped groups take the scalar
    path; then the multiple-of-8 groups at an offset that is not a multiple of 8.  Bit-equal to .t(), gaps untouched."""
    _lib, ops = _ops()
    for shapes, first in ((((64, 64), (72, 136), (7, 65), (1, 1), (130, 3)), 16), (((64, 64), (72, 136)), 13)):
        groups, off, tiles, table = [], first, 0, []
        for R, Cc in shapes:
            groups.append((off, R, Cc))
            table.append([off, R, Cc, tiles])
            tiles += -(-R // 64) * -(-Cc // 64)
            off += R * Cc + (11 if first == 13 else 24)  # gaps: 24 keeps the next offset a multiple of 8
        src = poison(1, off + 64, 41).flatten()
        dsrc, dst = src.to(device), sentinel_bf16(1, off + 64, device).flatten()
        tab = torch.tensor(table, dtype=torch.int64, device=device)
        _lib.check(_lib.lib().js2t_transpose_groups(ptr(dsrc), ptr(dst), ptr(tab), len(groups), tiles, ops._stream()), "transpose_groups")
        torch.cuda.synchronize()
        assert untouched(dst, [(slice(o, o + R * Cc), ) for o, R, Cc in groups]), "a write into a gap"
        for (o, R, Cc), (_, want) in zip(groups, ER.transpose_groups_ref(src, groups)):
            assert ER.same_bits(dst[o:o + R * Cc].cpu().view(Cc, R), want), (R, Cc)
