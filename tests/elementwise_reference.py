"""Plain fp64 references of the element-wise kernels (joeys2t_amd/csrc/elementwise.hip) for tests/test_hip_elementwise_ref.py:
CPU only, no kernels.

plan()        every case of the test plan: Case(op, dt, shape ...); GPU tests and the CPU self-check walk the same list.
inputs()      the "loud" operands of a case: what a kernel must not read is large (100 x randn: cropped GLU positions, pe rows >= T,
              table rows no id names, dout rows of pad ids, the neighbouring batch entries of im2col / col2im), what it must not
              drop or count twice weighs 16 x the rest (last row, last column, last duplicate).
reference()   {output name: Out(ref, cond, dtype, K, expected)}: the operation from its definition in fp64 on the inputs as stored
              (bf16 / f32), cond = the sum of the absolute values of the terms that are added (|ref| for products).  K None: a
              rounding or move kernel, `expected` holds the bits the kernel must produce (torch's round-to-nearest-even).
              With mutant=...: what a plausible slip of the kernel computes instead (MUTANTS).
keep_mask()   numpy twin of the counter-based dropout generator of csrc/common.hpp.
judge()       the ONE tolerance rule: |got - ref| <= u_out |ref| + K 2^-24 cond + floor.

Conventions at the kinks, shared by the kernels and torch's autograd (the reference takes them from autograd): relu'(0) = 0;
hardswish'(-3) = 0 and hardswish'(3) = 1 (the middle branch (2z + 3) / 6 holds on the OPEN interval (-3, 3)).  act_grad of
csrc/common.hpp used the closed interval (-1/2 and 3/2 at the kinks) until these tests: a bf16 pre-activation hits 3.0 exactly
about once in 2^7 values near it.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from attn_reference import poison

GRID = 4096 * 256      # work items of one trip of a grid-stride kernel (ew_grid: at most 4096 blocks of 256 threads)
BIG = GRID + 773       # a second, partial trip
F32_EPS = 2.0 ** -24   # unit roundoff of the fp32 arithmetic inside the kernels
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
FLOOR = 2.0 ** -126    # smallest normal number of bf16 and of fp32
PAD = 1                # pad id of the embedding cases
SEED, OFFSET, SITE = 11, 3, 5  # dropout state {seed, offset} and call site of every dropout case
ACTS = {"relu": 1, "gelu": 2, "swish": 3, "tanh": 4, "hardswish": 5}

# K of the rule, per kernel.  DERIVED: the fp32 roundings on the longest chain to one output, read off the kernel (the final
# rounding to the output type is the u_out term and is not counted).
K_DERIVED = {
    "axpby": 3,            # a*x, b*y, their sum
    "add_pe_dropout": 5,   # x + pe, + extra, 1 - p, 1 / (1 - p), * sc
    "dropout_bwd": 3,      # 1 - p, 1 / (1 - p), g * sc
    "embed_fwd": 1,        # table * scale
    # embed_bwd: scale * dout, then one add per occurrence of the id (onto the table's value): 1 + the largest multiplicity, per case
    "colsum": 24,          # stage 1: 16 adds per row lane of a 64-row slab + 2 to join the four lanes; stage 2 (<= 16 slabs): 2 adds
                           # per accumulator, s0 + s1, 2 to join the lanes, 1 onto `out`
    "col2im": 3,           # one add per contributing tap: at most ceil(K / stride) = 3 in every geometry of the plan
    "conv_weight_unpack_grad": 1,  # dw + v
    "act_relu": 2,         # dh * grad, * scale
    "act_hardswish": 6,    # 2z, + 3, the rounded constant 1/6, * 1/6, dh * grad, * scale
    "scale_out": 2,        # quantiser's scale: amax / 448, * mul
}
# MEASURED on the MI355X against this reference at the plan's inputs (kernels that call __expf / erff / tanhf); asserted: twice the
# measured value rounded up to a power of two.  The measured values are in the docstring of tests/test_hip_elementwise_ref.py.
K_MEASURED = {"glu_fwd": 16, "glu_bwd": 32, "act_gelu": 8, "act_swish": 16, "act_tanh": 2}


class Case:
    def __init__(self, op, **kw):
        self.op = op
        self.big = False
        self.__dict__.update(kw)

    @property
    def id(self):
        skip = ("op", )
        def short(v):
            if isinstance(v, torch.dtype):
                return {torch.float32: "f32", torch.bfloat16: "bf16"}[v]
            if isinstance(v, (tuple, list)):
                return "x".join(str(e) for e in v)
            return str(v)
        return self.op + "-" + "-".join(f"{k}{short(v)}" for k, v in self.__dict__.items() if k not in skip and v is not False and v is not None)

    def __repr__(self):
        return self.id


class Out:
    """One output of a case: ref / cond fp64; dtype of the stored result; K (None: bit-exact against `expected`)."""

    def __init__(self, ref, cond=None, dtype=torch.float32, K=None, expected=None):
        self.ref, self.dtype, self.K = ref, dtype, K
        self.cond = ref.abs() if cond is None else cond
        self.expected = expected


DTS = (torch.float32, torch.bfloat16)
GEOS = ((5, 2, 2), (3, 2, 1), (3, 1, 1))  # (K, stride, pad) of im2col / col2im


def tout_of(tin, K, stride, pad):
    return (tin + 2 * pad - K) // stride + 1


# ------------------------------------------------------------------------------------------------------------------ the plan
def plan():
    P = []
    add = lambda op, **kw: P.append(Case(op, **kw))  # noqa: E731
    for s in DTS:
        for d in DTS:
            for n in (1, 3, 4, 5, 1027):
                add("cast", src=s, dst=d, n=n)
            add("cast", src=s, dst=d, n=4 * BIG + 3, big=True)
    add("cast", src=torch.float32, dst=torch.bfloat16, n=0, special=True)
    for dt in DTS:
        for with_y in (True, False):
            add("axpby", dt=dt, n=1027, with_y=with_y)
            add("axpby", dt=dt, n=BIG, with_y=with_y, big=True)
        for op in ("glu_fwd", "glu_bwd"):
            for C in (1, 5, 64):
                for vt in (0, 1, 6, 7):
                    add(op, dt=dt, B=3, T=7, C=C, vt=vt)
            add(op, dt=dt, B=3, T=7, C=BIG // 21, vt=6, big=True)
        for D in (4, 260):
            for pe in (True, False):
                for extra in (True, False):
                    for p in (0.0, 0.1, 0.25):
                        add("add_pe_dropout", dt=dt, B=3, T=5, D=D, pe=pe, extra=extra, p=p)
        add("add_pe_dropout", dt=dt, B=3, T=7, D=4 * (BIG // 21), pe=True, extra=True, p=0.1, big=True)
        for cols in (1, 3, 5, 258, 4, 260):
            add("dropout_bwd", dt=dt, rows=15, cols=cols, p=0.25 if cols in (3, 258) else 0.1)
        add("dropout_bwd", dt=dt, rows=21, cols=4 * (BIG // 21) - 1, p=0.1, big=True)
        for act in ACTS:
            add("act_bwd", dt=dt, act=act, n=1027, scale=0.75)
        add("act_bwd", dt=dt, act="gelu", n=BIG, scale=0.75, big=True)
        for out_dt in DTS:
            for scale in (1.0, 16.25):
                add("embed_fwd", dt=dt, out=out_dt, n_ids=600, D=264, vocab=50, scale=scale)
        add("embed_fwd", dt=dt, out=dt, n_ids=2247, D=467, vocab=3000, scale=16.25, big=True)
        add("embed_bwd", dt=dt, n_ids=600, D=264, vocab=50, scale=16.25)
        add("embed_bwd", dt=dt, n_ids=2247, D=467, vocab=3000, scale=16.25, big=True)
        for rows in (1, 3, 63, 64, 65, 257, 833):
            for cols in (1, 37, 64, 65, 8, 520):
                for acc in (False, True):
                    add("colsum", dt=dt, rows=rows, cols=cols, acc=acc)
        for geo in GEOS:
            for tin in (1, 2, 36, 37):
                for C in (8, 24):
                    add("im2col", dt=dt, B=3, tin=tin, C=C, geo=geo)
                    add("col2im", dt=dt, B=3, tin=tin, C=C, geo=geo)
                if dt == torch.float32:
                    add("col2im", dt=dt, B=3, tin=tin, C=4, geo=geo)
        vec = 8 if dt == torch.bfloat16 else 4
        add("im2col", dt=dt, B=3, tin=467, C=107 * vec, geo=(7, 1, 3), big=True)   # B * tout * K * C / vec = 3 * 467 * 7 * 107 = BIG
        add("col2im", dt=dt, B=3, tin=749, C=467, geo=(3, 2, 1), big=True)           # scalar kernel: B * tin * C = BIG
        for shape in ((1, 1, 1), (3, 5, 3), (16, 80, 5)):
            add("conv_weight_pack", dt=dt, shape=shape)
        add("conv_weight_pack", dt=dt, shape=(107, 467, 21), big=True)
        for n in (1, 7, 9, 512 * 256 * 8 + 3):
            for where in ("first", "last", "negative"):
                add("quantize", dt=dt, n=n, where=where)
        add("quantize", dt=dt, n=9, where="zero")
    add("col2im", dt=torch.bfloat16, B=3, tin=749, C=467 * 8, geo=(3, 2, 1), big=True)  # vector kernel: B * tin * C / 8 = BIG
    for shape in ((1, 1, 1), (3, 5, 3), (16, 80, 5)):
        for acc in (False, True):
            add("conv_weight_unpack_grad", shape=shape, acc=acc)
    add("conv_weight_unpack_grad", shape=(107, 467, 21), acc=True, big=True)
    return P


# ---------------------------------------------------------------------------------------------------------------- the inputs
def _gen(case):
    return torch.Generator().manual_seed(sum(map(ord, case.id)) * 7919 % (2 ** 31))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _poison(n, seed, dt=torch.float32):
    return poison(1, n, seed).flatten().to(dt)


def embed_ids(case, g):
    """ids of an embedding case.  Small: ids from rows 2 .. 39 (about 15 duplicates each), -1 and `vocab` (out of range), the pad
    id twice, id 45 ONLY at positions 3 and 515, id 44 only at 300 and 590 (the ordered kernel's scan finds the earlier one on its
    second trip); rows 0, 40 .. 43, 46 .. 49 of the table are named by no id."""
    n, V = case.n_ids, case.vocab
    if case.big:
        ids = torch.randint(2, V - 100, (n, ), generator=g)
    else:
        ids = torch.randint(2, 40, (n, ), generator=g)
        ids[3] = ids[515] = 45
        ids[300] = ids[590] = 44
    ids[10], ids[20], ids[30], ids[n - 200] = -1, V, PAD, PAD
    return ids


def _named(case, ids):
    ok = ids[(ids >= 0) & (ids < case.vocab)]
    named = torch.zeros(case.vocab, dtype=torch.bool)
    named[ok] = True
    return named


def inputs(case):
    g, op = _gen(case), case.op
    dt = getattr(case, "dt", torch.float32)
    if op == "cast":
        if getattr(case, "special", False):
            bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,    # ties: 1 + 2^-8 -> 1 (even), 1 + 3 2^-8 -> 1 + 2^-6 (even), both signs
                    0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF,    # just above / below a tie; the largest finite fp32 -> +-inf
                    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345, 0x3F800000, 0x3F7FFFFF]
            return dict(src=torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32))
        return dict(src=(3.0 * _randn(g, case.n)).to(case.src))
    if op == "axpby":
        return dict(x=_randn(g, case.n).to(dt), y=_randn(g, case.n).to(dt) if case.with_y else None, a=0.7, b=-1.3)
    if op in ("glu_fwd", "glu_bwd"):
        rows, C = case.B * case.T, case.C
        x = torch.cat([_randn(g, rows, C), 16.0 * torch.rand(rows, C, generator=g) - 8.0], 1)
        gate = x[:, C:].reshape(-1)
        gate[::7] = 100.0   # saturation: sigmoid = 1 / exp overflows to inf
        gate[3::7] = -100.0
        dy = _randn(g, rows, C)
        dy[-1] *= 16.0
        dy[:, -1] *= 16.0
        dead = (torch.arange(rows) % case.T) >= case.vt
        x[dead] = poison(int(dead.sum()), 2 * C, 21).float()
        dy[dead] = poison(int(dead.sum()), C, 22).float()
        return dict(x=x.to(dt), dy=dy.to(dt), vt=case.vt)
    if op == "add_pe_dropout":
        B, T, D = case.B, case.T, case.D
        pe = None
        if case.pe:  # [B * T, D]: the rows at and beyond T are poison
            pe = poison(B * T, D, 23).float()
            pe[:T] = _randn(g, T, D)
        return dict(x=_randn(g, B * T, D).to(dt), pe=pe, extra=_randn(g, B * T, D).to(dt) if case.extra else None)
    if op == "dropout_bwd":
        dy = _randn(g, case.rows, case.cols)
        dy[-1] *= 16.0
        dy[:, -1] *= 16.0
        return dict(dy=dy.to(dt))
    if op == "act_bwd":
        z = 16.0 * torch.rand(case.n, generator=g) - 8.0
        z[:8] = torch.tensor([0.0, 3.0, -3.0, -0.0, 8.0, -8.0, 2.999, -2.999])
        return dict(dh=_randn(g, case.n).to(dt), z=z.to(dt))
    if op in ("embed_fwd", "embed_bwd"):
        ids = embed_ids(case, g)
        V, D, n = case.vocab, case.D, case.n_ids
        if op == "embed_fwd":
            table = _randn(g, V, D)
            table[:, -1] *= 16.0
            unnamed = ~_named(case, ids)
            table[unnamed] = poison(int(unnamed.sum()), D, 24).float()
            return dict(ids=ids, table=table.to(dt))
        dout = _randn(g, n, D)
        last = torch.zeros(n, dtype=torch.bool)
        for v in torch.unique(ids):
            last[int((ids == v).nonzero().max())] = True
        dout[last] *= 16.0   # the last duplicate of every id
        dout[:, -1] *= 16.0
        skip = (ids < 0) | (ids >= V) | (ids == PAD)
        dout[skip] = poison(int(skip.sum()), D, 25).float()
        return dict(ids=ids, dout=dout.to(dt), pre=_randn(g, V, D))
    if op == "colsum":
        x = _randn(g, case.rows, case.cols)
        x[-1] *= 16.0
        x[:, -1] *= 16.0
        return dict(x=x.to(dt), pre=_randn(g, case.cols))
    if op in ("im2col", "col2im"):
        K, stride, pad = case.geo
        B, tin, C = case.B, case.tin, case.C
        rows = tin if op == "im2col" else tout_of(tin, K, stride, pad)
        width = C if op == "im2col" else K * C
        x = _randn(g, B, rows, width)
        x[:, -1] *= 16.0
        x[:, :, -1] *= 16.0
        x[0] *= 100.0   # the neighbours of the middle entry are hostile
        x[2] *= 100.0
        return dict(x=x.to(dt))
    if op == "conv_weight_pack":
        return dict(w=_randn(g, *case.shape))
    if op == "conv_weight_unpack_grad":
        cout, cin, k = case.shape
        return dict(dwp_t=_randn(g, k * cin, cout), pre=_randn(g, cout, cin, k))
    if op == "quantize":
        x = 3.0 * _randn(g, case.n)
        if case.where == "zero":
            x.zero_()
        else:
            x[{"first": 0, "last": -1, "negative": case.n // 2}[case.where]] = -41.5 if case.where == "negative" else 41.5
        return dict(x=x.to(dt), mul=torch.tensor([1.75]))
    raise KeyError(op)


# ------------------------------------------------------------------------------------------- the dropout generator's numpy twin
_M32 = np.uint64(0xFFFFFFFF)


def _u(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def hash32(x):
    x = _u(x)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def hash32w(x):
    x = (_u(x) * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    return (x * np.uint64(0x846CA68B)) & _M32


def dropout_key(seed, offset, site):
    """The call-invariant key of {seed, offset} (the int64 pair of ops.DropoutRng.state, read as uint64) and the call site id."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    return hash32(_u(seed) ^ hash32((seed >> 32) + 0x9E3779B9) ^ hash32(_u(offset) * np.uint64(0x85EBCA6B) + np.uint64(1))
                  ^ hash32(((_u(offset >> 32)) ^ _u(site)) * np.uint64(0xC2B2AE35) + np.uint64(2)))


def dropout_keep4_key(key, row, col4, p):
    """bool [..., 4]: keep decisions of columns 4 col4 .. 4 col4 + 3 of `row`; P(drop) = floor(p * 65536) / 65536."""
    rowkey = hash32(_u(row) ^ key)
    h0, h1 = hash32w(rowkey + np.uint64(2) * _u(col4)), hash32w(rowkey + np.uint64(2) * _u(col4) + np.uint64(1))
    thr = np.uint64(int(np.float32(p) * np.float32(65536.0)))
    lo, sh = np.uint64(0xFFFF), np.uint64(16)
    return np.stack([(h0 & lo) >= thr, (h0 >> sh) >= thr, (h1 & lo) >= thr, (h1 >> sh) >= thr], -1)


def keep_mask(rows, cols, p, seed=SEED, offset=OFFSET, site=SITE, mutant=None):
    """bool [rows, cols]: the keep mask of a [rows, cols] launch (add_pe_dropout with cols = D, dropout_bwd)."""
    c4n = (cols + 3) // 4
    key = dropout_key(seed, offset, site)
    row, col4 = np.arange(rows, dtype=np.uint64)[:, None], np.arange(c4n, dtype=np.uint64)[None, :]
    if mutant == "mask_as_if_cols_multiple_of_4":  # the flat work item index split by cols / 4 instead of ceil(cols / 4)
        flat, wrong = row * np.uint64(c4n) + col4, np.uint64(max(cols // 4, 1))
        row, col4 = flat // wrong, flat % wrong
    keep = dropout_keep4_key(key, row + 0 * col4, col4 + 0 * row, p)
    if mutant == "keep_bits_reversed":
        keep = keep[..., ::-1]
    return torch.from_numpy(np.ascontiguousarray(keep.reshape(rows, 4 * c4n)[:, :cols]))


# ------------------------------------------------------------------------------------------------------------ the mathematics
def truncate_bf16(x32):
    return (x32.float().contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


def _stop(val, per_item=1, unwritten=float("nan"), limit=None):
    """grid_stride_stops: the elements of the work items behind the first trip keep what the buffer held"""
    flat = val.reshape(-1).clone()
    end = flat.numel() if limit is None else limit
    if isinstance(unwritten, torch.Tensor):
        flat[GRID * per_item:end] = unwritten.reshape(-1)[GRID * per_item:end]
    else:
        flat[GRID * per_item:end] = unwritten
    return flat.view(val.shape)


def im2col_index(B, tin, C, K, stride, pad, tau_le=False):
    """-> tau [tout, K] (the input position of every (t, kw)) and its validity"""
    tout = tout_of(tin, K, stride, pad)
    tau = torch.arange(tout)[:, None] * stride - pad + torch.arange(K)[None, :]
    return tau, (tau >= 0) & ((tau <= tin) if tau_le else (tau < tin))


def im2col_ref(x, K, stride, pad, mutant=None, guard=None):
    """x [B, tin, C] -> col [B, tout, K, C]: col[b, t, kw] = x[b, t stride - pad + kw], 0 outside the utterance.  The mutant
    reads the flat buffer: the row behind entry b is entry b + 1's first (the guard row behind the last)."""
    B, tin, C = x.shape
    tau, ok = im2col_index(B, tin, C, K, stride, pad, mutant == "im2col_tau_le_tin")
    flat = torch.cat([x.reshape(B * tin, C), guard if guard is not None else torch.zeros(1, C, dtype=x.dtype)])
    rows = (torch.arange(B)[:, None, None] * tin + tau[None]).clamp(0, B * tin)
    return torch.where(ok[None, :, :, None], flat[rows], torch.zeros((), dtype=x.dtype))


def col2im_ref(dcol, tin, K, stride, pad, mutant=None, guard=None):
    """The adjoint of im2col: dx[b, tau] = the sum of dcol[b, t, kw] over the (t, kw) with t stride - pad + kw == tau.
    -> (dx, cond) [B, tin, C]."""
    B, tout, _, C = dcol.shape
    if mutant is None:
        tau, ok = im2col_index(B, tin, C, K, stride, pad)
        dx, cond = torch.zeros(B, tin + 1, C, dtype=torch.float64), torch.zeros(B, tin + 1, C, dtype=torch.float64)
        idx = torch.where(ok, tau, torch.full_like(tau, tin)).flatten()  # invalid taps land in a row that is cut off
        d = dcol.double().reshape(B, tout * K, C)
        dx.index_add_(1, idx, d)
        cond.index_add_(1, idx, d.abs())
        return dx[:, :tin], cond[:, :tin]
    # the slips are slips of the gather loop: walk it
    p = pad + 1 if mutant == "col2im_pad_off_by_one" else pad
    flat = torch.cat([dcol.double().reshape(B * tout, K, C), (guard.double() if guard is not None else torch.zeros(tin + K, K * C, dtype=torch.float64)).view(-1, K, C)])
    dx = torch.zeros(B, tin, C, dtype=torch.float64)
    tau = torch.arange(tin)
    for kw in range(K):
        num = tau + p - kw
        ok = num >= 0
        if mutant != "col2im_no_stride_test":
            ok &= (num % stride) == 0
        t = torch.div(num.clamp_min(0), stride, rounding_mode="floor")
        if mutant != "col2im_no_tout_test":
            ok &= t < tout
        rows = (torch.arange(B)[:, None] * tout + t[None]).clamp_max(flat.shape[0] - 1)
        dx += torch.where(ok[None, :, None], flat[rows, kw], torch.zeros((), dtype=torch.float64))
    return dx, None


def act_grad_ref(z, act, mutant=None):
    """d act(z) / dz from torch autograd in fp64, and the sum of |terms added| inside it (relative to which fp32 rounds)."""
    z = z.double()
    zz = z.clone().requires_grad_(True)
    fn = {"relu": F.relu, "gelu": F.gelu, "swish": F.silu, "tanh": torch.tanh, "hardswish": F.hardswish}[act]
    if act == "gelu" and mutant == "gelu_tanh_approx":
        fn = lambda v: F.gelu(v, approximate="tanh")  # noqa: E731
    fn(zz).sum().backward()
    grad = zz.grad
    s = torch.sigmoid(z)
    if act == "swish" and mutant == "swish_without_z_term":
        grad = s
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    terms = {"relu": grad.abs(), "gelu": 0.5 + 0.5 * torch.erf(z / math.sqrt(2)).abs() + z.abs() * pdf,
             "swish": s * (1 + z.abs() * (1 + s)), "tanh": 1 + torch.tanh(z) ** 2, "hardswish": torch.where(z.abs() < 3, (2 * z.abs() + 3) / 6, grad.abs())}[act]
    return grad, terms


def glu_ref(x, dy, B, T, vt, mutant=None):
    """F.glu and its autograd in fp64 on x [B T, 2C], positions t >= vt of every entry cropped.  -> y, dx, cond of y, cond of dx"""
    rows, C = x.shape[0], x.shape[1] // 2
    r = torch.arange(rows)
    t = r if mutant == "glu_crop_by_row" else r % T
    live = ((t <= vt) if mutant == "glu_crop_le" else (t < vt)).double()[:, None]
    xx = x.double().clone().requires_grad_(True)
    y = F.glu(torch.cat([xx[:, C:], xx[:, :C]], 1) if mutant == "glu_halves_swapped" else xx, dim=1) * live
    y.backward(dy.double())
    a, b = x.double()[:, :C], x.double()[:, C:]
    s = torch.sigmoid(b)
    g = dy.double() * live
    # dx_a = g s (a product); dx_b = g a s (1 - s): the terms added are 1 and s
    return y.detach(), xx.grad, y.detach().abs(), torch.cat([(g * s).abs(), (g * a * s).abs() * (1 + s)], 1)


def reference(case, inp, mutant=None):
    op = case.op
    dt = getattr(case, "dt", torch.float32)
    f32 = lambda v: float(np.float32(v))  # noqa: E731  (scalar arguments travel as C floats)
    stop = mutant == "grid_stride_stops"
    NAN = float("nan")

    def exact(val, dtype, trunc_ok=True):
        """a rounding / move kernel: the expected bits (torch's round-to-nearest-even; the truncating mutant's)"""
        v32 = val if val.dtype in DTS else val.float()
        e = truncate_bf16(v32) if (mutant == "bf16_store_truncates" and dtype == torch.bfloat16 and v32.dtype == torch.float32) else v32.to(dtype)
        return Out(val.double(), None, dtype, None, e)

    if op == "cast":
        out = exact(inp["src"], case.dst)
        if stop:
            n4 = case.n // 4 * 4
            out.expected = _stop(out.expected.float(), 4, NAN, n4).to(case.dst)
        return dict(dst=out)
    if op == "axpby":
        a, b, x = f32(inp["a"]), f32(inp["b"]), inp["x"].double()
        ref, cond = a * x, (a * x).abs()
        if inp["y"] is not None:
            ref, cond = ref + b * inp["y"].double(), cond + (b * inp["y"].double()).abs()
        return dict(out=Out(_stop(ref) if stop else ref, cond, dt, K_DERIVED["axpby"]))
    if op in ("glu_fwd", "glu_bwd"):
        y, dx, cy, cdx = glu_ref(inp["x"], inp["dy"], case.B, case.T, case.vt, mutant)
        if op == "glu_fwd":
            return dict(y=Out(_stop(y) if stop else y, cy, dt, K_MEASURED["glu_fwd"]))
        if stop:
            C = case.C
            dx = torch.cat([_stop(dx[:, :C].contiguous()), _stop(dx[:, C:].contiguous())], 1)
        return dict(dx=Out(dx, cdx, dt, K_MEASURED["glu_bwd"]))
    if op in ("add_pe_dropout", "dropout_bwd"):
        p = f32(case.p)
        sc = 1.0 / (1.0 - p) if p > 0 and mutant != "dropout_scale_missing" else 1.0
        if op == "add_pe_dropout":
            rows, cols = case.B * case.T, case.D
            v = inp["x"].double()
            cond = v.abs()
            if inp["pe"] is not None:
                row = torch.arange(rows)
                pe = inp["pe"].double()[row if mutant == "pe_by_row" else row % case.T]
                v, cond = v + pe, cond + pe.abs()
            if inp["extra"] is not None and mutant != "extra_dropped":
                v, cond = v + inp["extra"].double(), cond + inp["extra"].double().abs()
            name = "y"
        else:
            rows, cols = case.rows, case.cols
            v = inp["dy"].double()
            cond = v.abs()
            name = "dx"
        keep = keep_mask(rows, cols, p, mutant=mutant).double() if p > 0 else torch.ones(rows, cols, dtype=torch.float64)
        ref, cond = v * keep * sc, cond * keep * sc
        if stop and op == "add_pe_dropout":
            ref = _stop(ref, 4)
        elif stop:  # a work item: 4 columns of a row padded to a multiple of 4
            c4n = (cols + 3) // 4
            padded = torch.zeros(rows, 4 * c4n, dtype=torch.float64)
            padded[:, :cols] = ref
            ref = _stop(padded, 4)[:, :cols]
        return {name: Out(ref, cond, dt, K_DERIVED[op])}
    if op == "act_bwd":
        grad, terms = act_grad_ref(inp["z"], case.act, mutant)
        w = inp["dh"].double() * f32(case.scale)
        ref = w * grad
        K = K_DERIVED.get("act_" + case.act) or K_MEASURED["act_" + case.act]
        return dict(dz=Out(_stop(ref) if stop else ref, w.abs() * terms, dt, K))
    if op == "embed_fwd":
        ids, table, V = inp["ids"], inp["table"], case.vocab
        ok = (ids >= 0) & (ids < V)
        scale = 1.0 if mutant == "embed_fwd_without_scale" else f32(case.scale)
        rows = table[ids.clamp(0, V - 1)]
        if mutant == "embed_oob_reads_row0":
            rows = table[torch.where(ok, ids, torch.zeros_like(ids))]
            ok = torch.ones_like(ok)
        if f32(case.scale) == 1.0:  # a move (and a rounding when the table is f32 and the output bf16)
            out = exact(torch.where(ok[:, None], rows, torch.zeros((), dtype=rows.dtype)), case.out)
            if stop:
                out.expected = _stop(out.expected.float()).to(case.out)
            return dict(out=out)
        ref = torch.where(ok[:, None], rows.double() * scale, torch.zeros((), dtype=torch.float64))
        return dict(out=Out(_stop(ref) if stop else ref, None, case.out, K_DERIVED["embed_fwd"]))
    if op == "embed_bwd":
        ids, V, n = inp["ids"], case.vocab, case.n_ids
        ok = (ids >= 0) & (ids < V)
        if mutant != "embed_bwd_adds_pad_row":
            ok &= ids != PAD
        if mutant == "embed_bwd_last_duplicate_only":
            later = torch.zeros(n, dtype=torch.bool)
            seen = set()
            for i in range(n - 1, -1, -1):
                later[i] = int(ids[i]) in seen
                seen.add(int(ids[i]))
            ok &= ~later
        d = inp["dout"].double() * f32(case.scale)
        if stop:
            d = _stop(d, 1, 0.0)
        ref, cond = inp["pre"].double().clone(), inp["pre"].double().abs()
        ref.index_add_(0, ids[ok], d[ok])
        cond.index_add_(0, ids[ok], d[ok].abs())
        mult = int(torch.bincount(ids[ok]).max())
        return dict(dtable=Out(ref, cond, torch.float32, 1 + mult))
    if op == "colsum":
        x = inp["x"].double()
        r = torch.arange(case.rows)
        if mutant == "colsum_drops_partial_slab":
            x = x[:case.rows // 64 * 64]
        elif mutant == "colsum_drops_a_row_lane":
            x = x[(r % 64) % 4 != 3]
        ref, cond = x.sum(0), x.abs().sum(0)
        if case.acc:
            cond = cond + inp["pre"].double().abs()
            if mutant != "colsum_ignores_accumulate":
                ref = ref + inp["pre"].double()
        return dict(out=Out(ref, cond, torch.float32, K_DERIVED["colsum"]))
    if op == "im2col":
        K, stride, pad = case.geo
        guard = im2col_guard(case)
        col = im2col_ref(inp["x"], K, stride, pad, mutant, guard)
        out = Out(col.double(), None, dt, None, col)
        if stop:
            out.expected = _stop(col.float(), 8 if dt == torch.bfloat16 else 4).to(dt)
        return dict(col=out)
    if op == "col2im":
        K, stride, pad = case.geo
        B, tin, C = case.B, case.tin, case.C
        tout = tout_of(tin, K, stride, pad)
        dcol = inp["x"].view(B, tout, K, C)
        ref, cond = col2im_ref(dcol, tin, K, stride, pad)
        if mutant in ("col2im_no_stride_test", "col2im_no_tout_test", "col2im_pad_off_by_one"):
            ref, _ = col2im_ref(dcol, tin, K, stride, pad, mutant, col2im_guard(case))
        if stop:
            ref = _stop(ref, 8 if (dt == torch.bfloat16 and C % 8 == 0) else 1)
        return dict(dx=Out(ref, cond, dt, K_DERIVED["col2im"]))
    if op == "conv_weight_pack":
        out = exact(inp["w"].permute(0, 2, 1).contiguous(), dt)  # wp[o, kw, c] = w[o, c, kw]
        if stop:
            out.expected = _stop(out.expected.float()).to(dt)
        return dict(wp=out)
    if op == "conv_weight_unpack_grad":
        cout, cin, k = case.shape
        v = inp["dwp_t"].view(k, cin, cout).permute(2, 1, 0).contiguous()  # dw[o, c, kw] = dwp_t[kw cin + c, o]
        if not case.acc:
            return dict(dw=Out(v.double(), None, torch.float32, None, v))
        ref = v.double() + inp["pre"].double()
        if stop:
            ref = _stop(ref, 1, inp["pre"].double())
        return dict(dw=Out(ref, v.double().abs() + inp["pre"].double().abs(), torch.float32, K_DERIVED["conv_weight_unpack_grad"]))
    if op == "quantize":
        x32, mul = inp["x"].float(), inp["mul"]
        amax = x32.abs().max()
        # a rounding kernel: fp32 x * (448 / amax) as the kernel forms it, clamped, to e4m3 by torch's round-to-nearest-even
        inv = torch.tensor(448.0) / amax if amax > 0 else torch.tensor(0.0)
        y = (x32 * inv).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        scale = (amax.double() / 448.0 if amax > 0 else torch.tensor(1.0, dtype=torch.float64)) * mul.double()
        return dict(amax=Out(amax.double().reshape(1), None, torch.float32, None, amax.reshape(1)), y=Out(y.double(), None, torch.uint8, None, y),
                    scale=Out(scale, None, torch.float32, 0 if amax == 0 else K_DERIVED["scale_out"]))
    raise KeyError(op)


def im2col_guard(case):
    """the poison row behind the last entry of x (what `tau <= tin` reads for the last batch entry)"""
    return _poison(case.C, 26, case.dt)[None]


def col2im_guard(case):
    """poison rows behind the last entry of dcol (what a missing `t < tout` test reads for the last batch entry)"""
    K, stride, pad = case.geo
    return poison(case.tin + K, K * case.C, 27).to(case.dt)


def transpose_groups_ref(src, groups):
    """groups: [(offset, rows, cols)] over the flat bf16 buffer `src` -> [(offset, the [cols, rows] block)]"""
    return [(off, src[off:off + R * Cc].view(R, Cc).t().contiguous()) for off, R, Cc in groups]


# ------------------------------------------------------------------------------------------------------------------ mutants
def _no_tout_applies(c):
    K, stride, pad = c.geo
    tout = tout_of(c.tin, K, stride, pad)
    return any((tau + pad - kw) >= 0 and (tau + pad - kw) % stride == 0 and (tau + pad - kw) // stride >= tout for tau in range(c.tin) for kw in range(K))


def _tau_reaches_tin(c):
    K, stride, pad = c.geo
    return any(t * stride - pad + kw == c.tin for t in range(tout_of(c.tin, K, stride, pad)) for kw in range(K))


def _bf16_rounds(c):
    """the cases whose bf16 store rounds: a handful of outputs cannot tell truncation from rounding (it moves a value by less than
    2^-8 |ref| half of the time), so judged outputs count from 64 elements on; exact ones are told apart by inequality"""
    if c.op == "cast":
        return c.src == torch.float32 and c.dst == torch.bfloat16 and (c.n >= 4 or getattr(c, "special", False))
    if c.op == "conv_weight_pack":
        return c.dt == torch.bfloat16 and c.shape != (1, 1, 1)
    if c.op == "embed_fwd":
        return c.out == torch.bfloat16 and (c.dt == torch.float32 or c.scale != 1.0)
    if c.op in ("glu_fwd", "glu_bwd"):
        return c.dt == torch.bfloat16 and c.vt * c.B * c.C >= 64
    if c.op in ("axpby", "act_bwd", "add_pe_dropout", "col2im"):
        # plain dropout of a bf16 tensor at p = 0 is a move; a relu / hardswish-free product still rounds
        return c.dt == torch.bfloat16 and not (c.op == "add_pe_dropout" and not c.pe and not c.extra and c.p == 0) and not (c.op == "col2im" and c.tin < 4)
    if c.op == "dropout_bwd":
        return c.dt == torch.bfloat16 and c.rows * c.cols >= 64
    return False


# (name, applies(case)): a mutant applies where it computes something else than the reference
MUTANTS = [
    ("bf16_store_truncates", _bf16_rounds),
    ("glu_halves_swapped", lambda c: c.op in ("glu_fwd", "glu_bwd") and c.vt > 0),
    ("glu_crop_le", lambda c: c.op in ("glu_fwd", "glu_bwd") and c.vt < c.T),
    ("glu_crop_by_row", lambda c: c.op in ("glu_fwd", "glu_bwd") and c.vt > 0 and c.B > 1),
    ("pe_by_row", lambda c: c.op == "add_pe_dropout" and c.pe and c.B > 1),
    ("extra_dropped", lambda c: c.op == "add_pe_dropout" and c.extra),
    ("dropout_scale_missing", lambda c: c.op in ("add_pe_dropout", "dropout_bwd") and c.p > 0),
    ("keep_bits_reversed", lambda c: c.op in ("add_pe_dropout", "dropout_bwd") and c.p > 0),
    ("mask_as_if_cols_multiple_of_4", lambda c: c.op == "dropout_bwd" and c.cols % 4 != 0 and c.cols > 4),
    ("swish_without_z_term", lambda c: c.op == "act_bwd" and c.act == "swish"),
    ("gelu_tanh_approx", lambda c: c.op == "act_bwd" and c.act == "gelu" and c.dt == torch.float32),
    ("embed_fwd_without_scale", lambda c: c.op == "embed_fwd" and c.scale != 1.0),
    ("embed_oob_reads_row0", lambda c: c.op == "embed_fwd"),
    ("embed_bwd_adds_pad_row", lambda c: c.op == "embed_bwd"),
    ("embed_bwd_last_duplicate_only", lambda c: c.op == "embed_bwd"),
    ("colsum_drops_partial_slab", lambda c: c.op == "colsum" and c.rows % 64 != 0),
    ("colsum_drops_a_row_lane", lambda c: c.op == "colsum" and c.rows >= 4),
    ("colsum_ignores_accumulate", lambda c: c.op == "colsum" and c.acc),
    ("col2im_no_stride_test", lambda c: c.op == "col2im" and c.geo[1] > 1),
    ("col2im_no_tout_test", lambda c: c.op == "col2im" and _no_tout_applies(c)),
    ("col2im_pad_off_by_one", lambda c: c.op == "col2im"),
    ("im2col_tau_le_tin", lambda c: c.op == "im2col" and _tau_reaches_tin(c)),
    ("grid_stride_stops", lambda c: c.big and c.op != "quantize"),
]


# ------------------------------------------------------------------------------------------------------ the tolerance rule
def same_bits(got, expected):
    """bit equality of two tensors of one type; NaN matches NaN whatever its payload"""
    if got.dtype != expected.dtype or got.shape != expected.shape:
        return False
    if got.dtype in DTS:
        nan = expected.isnan()
        if not torch.equal(got.isnan(), nan):
            return False
        view = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
        return bool((got.contiguous().view(view)[~nan] == expected.contiguous().view(view)[~nan]).all())
    return torch.equal(got, expected)


def judge(got, out):
    """THE tolerance rule -> (ok, ratio, text).  Bit-exact outputs (out.K None): same_bits against out.expected.  Else every
    element must satisfy |got - ref| <= u_out |ref| + K 2^-24 cond + floor; ratio = the largest err / allowed."""
    if out.K is None:
        ok = same_bits(got, out.expected)
        return ok, 0.0 if ok else float("inf"), "bit-exact" if ok else "differs from the expected bits"
    got, ref = got.double().reshape(out.ref.shape), out.ref
    allowed = U_OUT[out.dtype] * ref.abs() + out.K * F32_EPS * out.cond + FLOOR
    ratio = ((got - ref).abs() / allowed).nan_to_num(float("inf"), posinf=float("inf"))
    worst = float(ratio.max())
    return worst <= 1.0, worst, f"worst err / allowed {worst:.3g} (K = {out.K})"


def measured_K(got, out):
    """the smallest K at which `got` would pass: max (err - u_out |ref| - floor) / (2^-24 cond)"""
    got, ref = got.double().reshape(out.ref.shape), out.ref
    need = ((got - ref).abs() - U_OUT[out.dtype] * ref.abs() - FLOOR) / (F32_EPS * out.cond).clamp_min(1e-300)
    return max(float(need.max()), 0.0)


def as_stored(out, truncate=False):
    """the reference as a kernel would store it: rounded to the output type (the truncating mutant: cut)"""
    if out.K is None:
        return out.expected
    r32 = out.ref.float()
    return (truncate_bf16(r32) if truncate and out.dtype == torch.bfloat16 else r32.to(out.dtype))
