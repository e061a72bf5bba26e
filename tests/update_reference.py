"""Plain fp64 references of the update tail (joeys2t_amd/csrc/optim.hip; the LayerNorm-fold weights of csrc/norm_softmax.hip and
csrc/common.hpp) for tests/test_hip_update_ref.py: CPU only, numpy, no kernels.

plan(geo)     every case of the test plan, sized from the kernels' own unit sizes (geometry()): Case("clip" | "ranges" | "adamw" |
              "items" | "fold", ...).  GPU tests and the CPU self-checks walk the same list.
inputs()      the buffers of a case as the kernel sees them: payloads between sentinels (NaN bit patterns), gradients that mix
              magnitudes (every block of 4 scaled by 30, 1 or 0.01), blocks with g = m = v = 0, 1e18 wherever a sum of squares must not
              read, and elements that weigh enough wherever one could be dropped.
simulate()    what a kernel leaves in those buffers: mode "emul" = the kernel op for op in numpy float32, in its order of additions
              (the tolerance rule must pass it: test_emulation_passes_at_every_case); mode "ref" = the fp64 formula rounded to the
              stored type, optionally with one slip of MUTANTS put in (the rule must fail it: test_judge_rejects_every_mutant).
verdict()     every check of a case on such buffers -> the list of failed checks (empty: pass).  The GPU tests hand it what the
              kernels wrote, the CPU tests what simulate() wrote.

The rule is elementwise_reference.judge(): |got - ref| <= u_out |ref| + K 2^-24 cond + floor, cond = the sum of |terms added|.  The
references are the documented formulas in fp64 on the fp32 values the kernel reads (scalar arguments as C floats).  Two of them are
staged, like the bf16 shadow, which is the rounding of the p THE SAME LAUNCH stored: p' is judged against the formula on the m' and v'
the launch stored (each judged against its own fp64 reference from the inputs), because the error m' inherits relative to ITS cond
(b1 m and (1 - b1) g may cancel) is not bounded by the cond of p'; the fold weights are judged on the p the launch stored.

K of the rule: all DERIVED - the fp32 roundings on the longest chain to one output, the last one excepted (it is the u_out term);
contraction is off in adam4 / ln_fold_round4, sqrtf and the divisions are correctly rounded, there is no fast intrinsic.
"""
import ctypes as C
import itertools

import numpy as np
import torch

from attn_reference import SENT16, SENT32
from elementwise_reference import F32_EPS, Case, Out, judge, measured_K  # noqa: F401  (the ONE rule, U_OUT and FLOOR are judge's)

f32, f64 = np.float32, np.float64
LEAD = 64          # sentinel elements in front of and behind every payload (keeps 16-byte alignment)
HOSTILE = 1e18     # what a sum of squares must not read (its square is 1e36: one such element swamps everything)
U_BF16 = 2.0 ** -8  # half an ulp of a bf16 value x is at most 2^-8 |x| (8 significant bits)

K_DERIVED = {
    "m": 4,        # 1 - b1, gs = gscale * *gscale_dev, g * gs, (1 - b1) * gk            [b1 * m: 1]; the sum is u_out
    "v": 7,        # 1 - b2, gk twice (2 roundings each), (1 - b2) * gk, * gk             [b2 * v: 1]; the sum is u_out
    "p": 8,        # sqrtf(v'), (float)sqrt(bc2), / bc2_sqrt, + eps, m' / denom, (float)bc1, lr / bc1, step_size * (..)
                   # [p * (1 - lr * wd): 3]; the difference is u_out
    "partial": 28,  # x * x, 2 adds inside the float4, 16 trips onto the thread's sum, 6 butterfly steps, 4 wave sums = 29; the last is u_out
    "norm": 27,    # the sum: 29 (every partial) + 2 trips + 6 butterfly steps + 16 wave sums = 53 relative to the sum; the square root
                   # halves it: 26.5 -> 27; its own rounding is u_out
    "coef": 30,    # norm: 27 + its own rounding, the constant 1e-6f, norm + 1e-6f; the division is u_out
    "bias_f": 14,  # w * beta, 2 adds inside the float4, <= 5 trips (K <= 1280), 6 butterfly steps; + bias is u_out
    "cs": 15,      # the centring term sum(W gamma) / K: as bias_f, + the division
}
K_MEASURED = {}    # none: every K above is derived


def geometry():
    """The kernels' unit sizes, read from the library: {flat, rows, cols: js2t_adamw_items_geometry; sq: elements per block of the
    sums of squares (js2t_sumsq_partials)}.  Both are host functions."""
    from joeys2t_amd import _lib
    L = _lib.lib()
    g = [C.c_int32() for _ in range(3)]
    L.js2t_adamw_items_geometry(*[C.byref(v) for v in g])
    sq = 1
    while L.js2t_sumsq_partials(sq + 1) == 1:  # the largest n one block takes (a power of two today)
        sq *= 2
    assert L.js2t_sumsq_partials(sq) == 1 and L.js2t_sumsq_partials(7 * sq) == 7
    return dict(flat=int(g[0].value), rows=int(g[1].value), cols=int(g[2].value), sq=sq)


# ---------------------------------------------------------------------------------------------------------------- small helpers
def sent32(n):
    return np.full(n, SENT32, dtype=np.uint32).view(f32)


def sent16(n):
    return np.full(n, SENT16, dtype=np.uint16)


def bits32(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.uint32)


def bf16_rne(x32):
    """fp32 -> bf16 bits, round to nearest even (finite values)"""
    b = bits32(x32).astype(np.uint64)
    return ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def bf16_trunc(x32):
    return (bits32(x32) >> np.uint32(16)).astype(np.uint16)


def bf16_val(bits):
    return (bits.astype(np.uint32) << np.uint32(16)).view(f32).astype(f64)


def _judge(got, ref, cond, K):
    with np.errstate(invalid="ignore"):  # (a sentinel left in an output is a NaN: it fails the rule, quietly)
        got = np.ascontiguousarray(got, dtype=f64)
    ok, ratio, _ = judge(torch.from_numpy(np.ascontiguousarray(got, dtype=f64)), Out(torch.from_numpy(np.ascontiguousarray(ref, dtype=f64)),
                                                                                     torch.from_numpy(np.ascontiguousarray(cond, dtype=f64)), torch.float32, K))
    return ok, ratio


def _mk(got, ref, cond, K):
    with np.errstate(invalid="ignore"):
        got = np.ascontiguousarray(got, dtype=f64)
    return measured_K(torch.from_numpy(np.ascontiguousarray(got, dtype=f64)),
                      Out(torch.from_numpy(np.ascontiguousarray(ref, dtype=f64)), torch.from_numpy(np.ascontiguousarray(cond, dtype=f64)), torch.float32, K))


def _rng(case, salt=0):
    return np.random.default_rng((sum(map(ord, case.id)) * 7919 + salt) % (2 ** 31))


def _tree64(s):
    """wave_sum: the butterfly of 64 lanes adds neighbouring halves level by level (last axis a multiple of 64 -> / 64)"""
    s = s.reshape(s.shape[:-1] + (-1, 64))
    for _ in range(6):
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0]


class Stats:
    """largest err / allowed and largest measured K per output name, over everything verdict() has seen"""

    def __init__(self):
        self.worst = {}

    def add(self, name, ratio, k=0.0):
        was = self.worst.get(name, (0.0, 0.0))
        self.worst[name] = (max(was[0], ratio), max(was[1], k))


def _rule(fails, stats, name, got, ref, cond, K, where=""):
    ok, ratio = _judge(got, ref, cond, K)
    if stats is not None:
        stats.add(name, ratio, _mk(got, ref, cond, K))
    if not ok:
        fails.append(f"{name}{where}: err / allowed {ratio:.3g} (K = {K})")


# ------------------------------------------------------------------------------------------------------------------ the plan
class Hyper:
    """The schedule and constants of one AdamW launch.  dev: lr and step travel in device scalars and the HOST arguments are wrong on
    purpose (host_lr, host_step); gsd: *gscale_dev (None: absent)."""

    def __init__(self, lr=1e-3, betas=(0.9, 0.98), eps=1e-8, wd=0.01, step=3, gscale=1.0, gsd=None, dev=False):
        self.lr, self.b1, self.b2, self.eps, self.wd, self.step, self.gscale, self.gsd, self.dev = lr, betas[0], betas[1], eps, wd, step, gscale, gsd, dev

    @property
    def host_lr(self):
        return 7.0 * self.lr if self.dev else self.lr

    @property
    def host_step(self):
        return (3 if self.step == 1 else 1) if self.dev else self.step

    def at(self, k):
        h = Hyper.__new__(Hyper)
        h.__dict__.update(self.__dict__)
        h.step = self.step + k
        return h


def _flat(n, keep=0):
    return dict(kind=0, n=n, keep=keep)


def _mat(rows, cols, keep=0, fold=None, off4=False, big_mean=False):
    """fold: None | dict(bias=bool): a LayerNorm fold reads this matrix; off4: placed at off % 8 == 4"""
    return dict(kind=1, rows=rows, cols=cols, keep=keep, fold=fold, off4=off4, big_mean=big_mean)


def plan(geo):
    SQ, FL, UR, UC = geo["sq"], geo["flat"], geo["rows"], geo["cols"]
    P = []
    add = lambda op, **kw: P.append(Case(op, **kw))  # noqa: E731
    # ---- js2t_grad_norm_clip
    for n in (1, 3, 4, 5, 1023, SQ - 1, SQ, SQ + 1, 3 * SQ + 7):
        for clip in ("above", "below", "tiny", "off"):
            add("clip", n=n, clip=clip)
    add("clip", n=1030 * SQ + 5, clip="below", big=True)  # > 1024 partials: a second stride trip of norm_clip_kernel, a partial last block
    # ---- js2t_sumsq_ranges + js2t_norm_clip
    add("ranges", lens=(SQ + 1, ), p0=0)
    add("ranges", lens=(40000, 6), p0=37)
    add("ranges", lens=(1, 4, 6, SQ, SQ + 1), p0=0)
    add("ranges", lens=(SQ + 1, 1, 40000, 4, SQ, 6, SQ + 1, 40000), p0=37)
    # ---- js2t_adamw: every combination of the switches once, spread over the sizes
    sizes = (4, 8, 1020, 1024, 1028)
    combos = itertools.product((True, False), (0, 1), (0.0, 0.01), ((0.9, 0.98), (0.9, 0.999)), (1, 2, 1000, 100000), (False, True), (False, True))
    for i, (lp, zg, wd, betas, step, dev, gsd) in enumerate(combos):
        add("adamw", n=sizes[(i + i // 5) % 5], lp=lp, zg=zg, wd=wd, betas=betas, step=step, dev=dev, gsd=gsd, updates=3)
    add("adamw", n=8192 * 256 * 4 + 12, lp=True, zg=1, wd=0.01, betas=(0.9, 0.98), step=2, dev=True, gsd=True, updates=1, big=True)
    # ---- js2t_adamw_items
    mats = [(1, 4), (20, 16), (UR - 1, UC - 4), (UR, UC), (UR + 1, UC + 4), (UR + 8, UC // 2 + 4), (2 * UR + 2, 2 * UC + 4)]
    for n in (4, FL - 4, FL, FL + 4, 3 * FL + 4):
        add("items", name=f"flat{n}", launches=[[_flat(n)]], shadows="both", zg=1)
    for R, Cc in mats:
        add("items", name=f"mat{R}x{Cc}", launches=[[_mat(R, Cc)]], shadows="both", zg=1)
    add("items", name=f"mat{UR}x{UC // 2}at4", launches=[[_mat(UR, UC // 2, off4=True)]], shadows="both", zg=1)
    nine = [_flat(4), _mat(20, 16, keep=1), _flat(FL + 4), _mat(UR + 1, UC + 4), _flat(FL, keep=1), _mat(UR + 8, UC // 2 + 4), _mat(UR, UC // 2, keep=1, off4=True),
            _flat(3 * FL + 4), _mat(2 * UR + 2, 2 * UC + 4)]
    for shadows in ("both", "lp", "none"):
        add("items", name="nine", launches=[nine], shadows=shadows, zg=1)
    add("items", name="nine", launches=[nine], shadows="both", zg=0, dev=True)
    add("items", name="mixed", launches=[[_mat(20, 16), _flat(FL - 4), _mat(UR - 1, UC - 4, keep=1), _flat(8)]], shadows="lp", zg=1, dev=True)
    # the host's order: the 1-D items (gamma, beta, bias of every fold among them) in a launch of their own, then the matrices
    fm = [_mat(1, 4, fold=dict(bias=True)), _mat(UR - 1, 16, fold=dict(bias=False)), _mat(UR + 1, UC // 2 + 4, fold=dict(bias=True)),
          _mat(UR - 1, UC, fold=dict(bias=True), big_mean=True), _mat(UR + 1, UC, fold=dict(bias=False), keep=1), _mat(UR + 1, 16, fold=dict(bias=True)),
          _mat(8, 2 * UC + 4, fold=dict(bias=True))]  # wider than a unit: its fold must stay untouched
    for shadows in ("both", "none"):
        add("items", name="folds", launches=[None, fm], shadows=shadows, zg=1)  # None: the 1-D launch, built from the folds' vectors
    # ---- js2t_fold_ln_weights
    add("fold", entries=[(1, 4, True, False), (5, UC // 2, False, False), (UR - 1, UC // 2 + 4, True, False), (UR + 1, UC, True, True), (7, UC + 4, False, False),
                         (3, 2 * UC + 4, True, False)])  # (N, K, bias, large row mean); max_rows = 65
    return P


# ---------------------------------------------------------------------------------------------------------------- the inputs
def _grad(rng, n, zeros=True):
    """mixed magnitudes: each block of 4 scaled by 30, 1 or 0.01; with `zeros` every fifth block (from the fourth) is 0"""
    nb = -(-n // 4)
    scale = np.repeat(np.array([30.0, 1.0, 0.01])[rng.integers(0, 3, nb)], 4)[:n]
    g = rng.standard_normal(n) * scale
    zero = np.repeat(np.arange(nb) % 5 == 3, 4)[:n] if zeros else np.zeros(n, dtype=bool)
    g[zero] = 0.0
    return g.astype(f32), scale, zero


def _state(rng, n, updates=1, big_mean=False):
    """p, m, v and `updates` gradients of n elements; where a block's g is 0, m and v are 0 too (the update is exactly the decay)"""
    gs = []
    g, scale, zero = _grad(rng, n)
    gs.append(g)
    for _ in range(updates - 1):
        gk = (rng.standard_normal(n) * scale).astype(f32)
        gk[zero] = 0.0
        gs.append(gk)
    p = rng.standard_normal(n) + (30.0 if big_mean else 0.0)
    m = 0.1 * scale * rng.standard_normal(n)
    v = (0.1 * scale * rng.standard_normal(n)) ** 2
    m[zero], v[zero] = 0.0, 0.0
    p = p.astype(f32)
    # without weight decay p' = p there: ties of the bf16 rounding, both ways and both signs (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6)
    at = np.flatnonzero(zero)[:8]
    p[at] = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000] * 2, dtype=np.uint32).view(f32)[:at.size]
    return p, m.astype(f32), v.astype(f32), gs, zero


def _between(payload):
    return np.concatenate([sent32(LEAD), payload, sent32(LEAD)])


def _heavy(g, lo, n, SQ):
    """the last element of a piece and the first element of its last block weigh 2 sqrt(n) + 100 (each then carries > 1 % of the sum)"""
    w = 2.0 * np.sqrt(n) + 100.0
    g[lo + n - 1] = w
    g[lo + (n - 1) // SQ * SQ] = -w


def layout(case, geo):
    """The item tables of an "items" case -> dict(launches=[[row, ...]], rows as js2t_adamw_items takes them + the spec), total, folds=
    [dict(mat=row index data, gamma, beta, bias offsets ...)].  Pieces are separated by gaps of 8 sentinel elements."""
    FL, UR, UC = geo["flat"], geo["rows"], geo["cols"]
    pos, launches, folds, n_units = LEAD, [], [], []
    specs = list(case.launches)
    mats = specs[-1]
    if specs[0] is None:  # the 1-D launch of the fold cases: gamma, beta (K), bias (N, padded to a multiple of 4) of every fold matrix
        one = []
        for mi, s in enumerate(mats):
            if s.get("fold"):
                one += [dict(_flat(s["cols"]), role=("gamma", mi)), dict(_flat(s["cols"]), role=("beta", mi))]
                if s["fold"]["bias"]:
                    one.append(dict(_flat(-(-s["rows"] // 4) * 4), role=("bias", mi)))
        specs[0] = one
    for spec in specs:
        rows, unit = [], 0
        for s in spec:
            if s.get("off4"):
                pos += (4 - pos % 8) % 8
            else:
                pos += (-pos) % 8
            if s["kind"] == 0:
                n, units = s["n"], -(-s["n"] // FL)
                row = [0, pos, n, 1, unit, -1, s["keep"], 0]
            else:
                n, units = s["rows"] * s["cols"], -(-s["rows"] // UR) * -(-s["cols"] // UC)
                row = [1, pos, s["rows"], s["cols"], unit, -1, s["keep"], 0]
            rows.append(dict(s, row=row, off=pos, size=n))
            pos, unit = pos + n + 8, unit + units
        launches.append(rows)
        n_units.append(unit)
    if any(s.get("fold") for s in launches[-1]):
        role = {r["role"]: r["off"] for r in launches[0]}
        for mi, s in enumerate(launches[-1]):
            if s.get("fold"):
                s["row"][5] = len(folds)
                folds.append(dict(mat=s, N=s["rows"], K=s["cols"], gamma=role[("gamma", mi)], beta=role[("beta", mi)], bias=role.get(("bias", mi)),
                                  written=s["cols"] <= UC))
    return dict(launches=launches, n_units=n_units, total=pos + LEAD, folds=folds)


def inputs(case, geo):
    SQ = geo["sq"]
    rng = _rng(case)
    if case.op == "clip":
        n = case.n
        g, _, _ = _grad(rng, n, zeros=False)
        _heavy(g, 0, n, SQ)
        if case.clip == "tiny":  # a norm near 1e-4: the + 1e-6 of the denominator is 1 % of it
            g = (g.astype(f64) * (1e-4 / np.sqrt((g.astype(f64) ** 2).sum()))).astype(f32)
        norm = float(np.sqrt((g.astype(f64) ** 2).sum()))
        max_norm = {"above": 2.0 * norm + 1.0, "below": 0.37 * norm, "tiny": 0.5 * norm, "off": -1.0}[case.clip]
        buf = np.full(n + 2 * LEAD, HOSTILE, dtype=f32)
        buf[LEAD:LEAD + n] = g
        return dict(g=buf, pieces=[(LEAD, n, 0)], p0=0, n_blocks=-(-n // SQ), max_norm=float(f32(max_norm)), pre=np.zeros(0, dtype=f32))
    if case.op == "ranges":
        pieces, pos, pb = [], LEAD, case.p0
        for n in case.lens:
            pieces.append((pos, n, pb))
            pos, pb = pos + -(-n // 4) * 4 + 8, pb + -(-n // SQ)
        buf = np.full(pos + LEAD, HOSTILE, dtype=f32)
        for lo, n, _ in pieces:
            buf[lo:lo + n], _, _ = _grad(rng, n, zeros=False)
            _heavy(buf, lo, n, SQ)
        total = sum((buf[lo:lo + n].astype(f64) ** 2).sum() for lo, n, _ in pieces)
        pre = (rng.random(case.p0) * total / max(case.p0, 1) / 4).astype(f32)  # what other kernels left in partial[0, p0)
        return dict(g=buf, pieces=pieces, p0=case.p0, n_blocks=pb - case.p0, max_norm=float(f32(0.37 * np.sqrt(total + pre.astype(f64).sum()))), pre=pre)
    if case.op == "adamw":
        p, m, v, gs, zero = _state(rng, case.n, case.updates)
        h = Hyper(betas=case.betas, wd=case.wd, step=case.step, gscale=0.5 if case.gsd else 1.0, gsd=0.8 if case.gsd else None, dev=case.dev)
        return dict(p=_between(p), m=_between(m), v=_between(v), gs=[_between(g) for g in gs], lp=sent16(case.n + 2 * LEAD) if case.lp else None, h=h,
                    zero=zero)
    if case.op == "items":
        lay = layout(case, geo)
        tot = lay["total"]
        buf = {k: sent32(tot) for k in "pgmv"}
        zero = np.zeros(tot, dtype=bool)
        for rows in lay["launches"]:
            for s in rows:
                p, m, v, gs, z = _state(rng, s["size"], 1, s.get("big_mean", False))
                if s.get("role", ("", 0))[0] == "gamma":  # mixed sign, away from 0
                    p = ((1.0 + 0.3 * rng.standard_normal(s["size"])) * np.where(rng.random(s["size"]) < 0.3, -1.0, 1.0)).astype(f32)
                sl = slice(s["off"], s["off"] + s["size"])
                buf["p"][sl], buf["g"][sl], buf["m"][sl], buf["v"][sl], zero[sl] = p, gs[0], m, v, z
        # (the fold cases: a learning rate at which the step of gamma is well above the bf16 resolution of Wf)
        h = Hyper(lr=1e-2 if case.name == "folds" else 1e-3, gscale=0.5, gsd=0.8, dev=getattr(case, "dev", False))
        out = dict(buf, lay=lay, h=h, zero=zero, lp=sent16(tot) if case.shadows != "none" else None, lp_t=sent16(tot) if case.shadows == "both" else None)
        out["fold_bufs"] = [(sent16(f["N"] * f["K"] + 2 * LEAD), sent32(f["N"] + 2 * LEAD)) for f in lay["folds"]]
        return out
    if case.op == "fold":
        ent = []
        for N, K, has_bias, big_mean in case.entries:
            W = (rng.standard_normal((N, K)) + (30.0 if big_mean else 0.0)).astype(f32)
            gamma = ((1.0 + 0.3 * rng.standard_normal(K)) * np.where(rng.random(K) < 0.3, -1.0, 1.0)).astype(f32)
            ent.append(dict(N=N, K=K, W=W, gamma=gamma, beta=rng.standard_normal(K).astype(f32), bias=rng.standard_normal(N).astype(f32) if has_bias else None))
        return dict(entries=ent, fold_bufs=[(sent16(e["N"] * e["K"] + 2 * LEAD), sent32(e["N"] + 2 * LEAD)) for e in ent])
    raise KeyError(case.op)


# ------------------------------------------------------------------------------------------- sums of squares and the clip
def block_sums_ref(x, SQ):
    """fp64 sum of squares of every block of SQ elements of x"""
    nb = -(-x.size // SQ)
    pad = np.zeros(nb * SQ, dtype=f64)
    pad[:x.size] = x
    return (pad * pad).reshape(nb, SQ).sum(1)


def block_sums_emul(x, SQ):
    """sumsq_partial_kernel / sumsq_ranges_kernel in float32: 256 threads, thread t takes the float4 at 4 t + 1024 trip:
    s += ((xx + yy) + zz) + ww per trip; a piece's last, incomplete float4 goes element by element onto its thread's sum (that thread's
    last contribution); then the butterfly of each wave and the four wave sums in order."""
    nb, n4 = -(-x.size // SQ), x.size // 4 * 4
    pad = np.zeros(nb * SQ, dtype=f32)
    pad[:n4] = x[:n4]
    q = (pad * pad).reshape(nb, SQ // 1024, 256, 4)
    s = np.zeros((nb, 256), dtype=f32)
    for trip in range(SQ // 1024):
        s = s + (((q[:, trip, :, 0] + q[:, trip, :, 1]) + q[:, trip, :, 2]) + q[:, trip, :, 3])
    if n4 < x.size:
        b, t = n4 // SQ, (n4 % SQ // 4) % 256
        for j in range(n4, x.size):
            s[b, t] = s[b, t] + x[j] * x[j]
    w = _tree64(s)  # [nb, 4]
    t = np.zeros(nb, dtype=f32)
    for i in range(4):
        t = t + w[:, i]
    return t


def norm_clip_emul(partial, max_norm):
    """norm_clip_kernel in float32: thread t adds partial[t], partial[t + 1024], ...; 16 butterflies; the wave sums in order"""
    np_ = partial.size
    pad = np.zeros(-(-np_ // 1024) * 1024, dtype=f32)
    pad[:np_] = partial
    s = np.zeros(1024, dtype=f32)
    for row in pad.reshape(-1, 1024):
        s = s + row
    w, t = _tree64(s), f32(0)
    for i in range(16):
        t = t + w[i]
    norm = np.sqrt(t)
    coef = min(f32(1), f32(max_norm) / (norm + f32(1e-6))) if max_norm > 0 else f32(1)
    return np.array([norm, coef], dtype=f32)


def simulate_sumsq(case, inp, geo, mode, mutant=None):
    """-> dict(partial: the workspace between sentinels, as left by the sums of squares; out2: {norm, coef} between sentinels)"""
    SQ, p0, nb = geo["sq"], inp["p0"], inp["n_blocks"]
    partial = sent32(p0 + nb + 2 * LEAD)
    partial[LEAD:LEAD + p0] = inp["pre"]
    for i, (lo, n, pb) in enumerate(inp["pieces"]):
        x = inp["g"][lo:lo + n]
        if mutant == "tail_dropped":
            x = x[:n // 4 * 4]
        sums = block_sums_emul(x, SQ) if mode == "emul" else block_sums_ref(x, SQ).astype(f32)
        sums = np.concatenate([sums, np.zeros(-(-n // SQ) - sums.size, dtype=f32)])
        if mutant == "last_partial_block_dropped" and n % SQ:
            sums = sums[:-1]  # floor instead of ceil: the block is never launched
        if mutant == "block_range_off_by_one" and i > 0:
            sums[0] = 0.0     # `<` for `<=` in the search: the first block of a piece works on the piece before, behind its end
        at = LEAD + pb - (p0 if mutant == "p0_ignored" else 0)
        partial[at:at + sums.size] = sums
    vals = partial[LEAD:LEAD + p0 + nb].copy()
    vals[bits32(vals) == SENT32] = 0.0
    mx = inp["max_norm"]
    if mode == "emul":
        o = norm_clip_emul(vals, mx)
    else:
        norm = np.sqrt(vals.astype(f64).sum())
        coef = mx / (norm + (0.0 if mutant == "clip_without_1e-6" else 1e-6)) if mx > 0 else 1.0
        o = np.array([norm, coef if mutant == "clip_not_capped" else min(1.0, coef)]).astype(f32)
    return dict(partial=partial, out2=_between(o))


def verdict_sumsq(case, inp, geo, got, stats=None):
    SQ, p0, nb = geo["sq"], inp["p0"], inp["n_blocks"]
    fails = []
    part, out2 = got["partial"], got["out2"]
    bits = bits32(part)
    if not ((bits[:LEAD] == SENT32).all() and (bits[LEAD + p0 + nb:] == SENT32).all()):
        fails.append("partial: a write outside [p0, p0 + n_blocks)")
    if not (bits[LEAD:LEAD + p0] == bits32(inp["pre"])).all():
        fails.append("partial: what other kernels left in [0, p0) changed")
    total = inp["pre"].astype(f64).sum()
    for lo, n, pb in inp["pieces"]:  # each partial against the fp64 sum of ITS block
        ref = block_sums_ref(inp["g"][lo:lo + n].astype(f64), SQ)
        total += ref.sum()
        _rule(fails, stats, "partial", part[LEAD + pb:LEAD + pb + ref.size], ref, ref, K_DERIVED["partial"], f" (piece at {lo})")
    ob = bits32(out2)
    if not ((ob[:LEAD] == SENT32).all() and (ob[LEAD + 2:] == SENT32).all()):
        fails.append("out2: a write outside its two elements")
    norm = np.sqrt(total)
    mx = inp["max_norm"]
    coef = min(1.0, mx / (norm + 1e-6)) if mx > 0 else 1.0
    _rule(fails, stats, "norm", out2[LEAD:LEAD + 1], np.array([norm]), np.array([norm]), K_DERIVED["norm"])
    _rule(fails, stats, "coef", out2[LEAD + 1:LEAD + 2], np.array([coef]), np.array([coef]), K_DERIVED["coef"])
    if (mx <= 0 or mx > 1.5 * norm) and not out2[LEAD + 1] == f32(1):
        fails.append(f"coef: {out2[LEAD + 1]} where it must be exactly 1")
    return fails


def weights_sumsq(inp, geo):
    """How much the elements that could be dropped weigh: the smallest (change of the output when one of them is left out) /
    (allowed error of that output), over the last element and the first element of the last block of every piece, for the block's partial
    and for the norm."""
    SQ = geo["sq"]
    u = F32_EPS
    total = inp["pre"].astype(f64).sum() + sum((inp["g"][lo:lo + n].astype(f64) ** 2).sum() for lo, n, _ in inp["pieces"])
    worst = float("inf")
    for lo, n, _ in inp["pieces"]:
        last = block_sums_ref(inp["g"][lo:lo + n].astype(f64), SQ)[-1]
        for idx in {lo + n - 1, lo + (n - 1) // SQ * SQ}:
            w2 = float(inp["g"][idx]) ** 2
            worst = min(worst, w2 / ((1 + K_DERIVED["partial"]) * u * last))
            dn = np.sqrt(total) - np.sqrt(total - w2)
            worst = min(worst, dn / ((1 + K_DERIVED["norm"]) * u * np.sqrt(total)))
    return worst


# ------------------------------------------------------------------------------------------------------------------- AdamW
class Consts:
    pass


def consts(h, mutant=None):
    """the scalars of one launch in fp64 from the C floats that travel (the device scalars where they are given)"""
    c = Consts()
    F = lambda x: float(f32(x))  # noqa: E731
    c.lr = F(h.host_lr if mutant == "lr_dev_ignored" else h.lr)
    c.b1, c.b2, c.eps, c.wd = F(h.b1), F(h.b2), F(h.eps), F(h.wd)
    t = h.host_step if mutant == "device_step_ignored" else h.step
    gsd = 1.0 if (h.gsd is None or mutant == "gscale_dev_dropped") else F(h.gsd)
    c.gs = (1.0 if mutant == "gscale_dropped" else F(h.gscale)) * gsd
    c.bc1, c.bc2 = 1.0 - c.b1 ** t, 1.0 - c.b2 ** t
    return c


def ref_moments(p, g, m, v, h, mutant=None):
    """m' = b1 m + (1 - b1) g gs, v' = b2 v + (1 - b2) (g gs)^2 in fp64 -> m', cond, v', cond"""
    c = consts(h, mutant)
    p, g, m, v = (a.astype(f64) for a in (p, g, m, v))
    gk = g * c.gs
    if mutant == "coupled_decay":  # L2: the decay enters the gradient
        gk = gk + c.wd * p
    a, b = c.b1 * m, (1.0 - c.b1) * gk
    gv = g if mutant == "v_from_unscaled_gradient" else gk
    a2, b2 = c.b2 * v, (1.0 - c.b2) * gv * gv
    return a + b, np.abs(a) + np.abs(b), a2 + b2, np.abs(a2) + np.abs(b2)


def ref_param(p, m2, v2, h, mutant=None):
    """p' = p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps) in fp64 on the STORED m', v' -> p', cond"""
    c = consts(h, mutant)
    p, m2, v2 = (a.astype(f64) for a in (p, m2, v2))
    dec = 1.0 if mutant == "coupled_decay" else 1.0 - c.lr * c.wd
    if mutant == "eps_inside_sqrt":
        denom = np.sqrt(v2 / c.bc2 + c.eps)
    else:
        denom = np.sqrt(v2) / (c.bc2 if mutant == "sqrt_bc2_missing" else np.sqrt(c.bc2)) + c.eps
    step_size = c.lr if mutant == "step_size_without_bc1" else c.lr / c.bc1
    t1, t2 = p * dec, step_size * m2 / denom
    return t1 - t2, np.abs(t1) + np.abs(t2)


def adam_emul(p, g, m, v, h):
    """adam4 op for op in float32 (contraction off), scalars as the launcher / kernel form them -> p', m', v'"""
    one = f32(1)
    lr, b1, b2, eps, wd = f32(h.lr), f32(h.b1), f32(h.b2), f32(h.eps), f32(h.wd)
    bc1 = f32(1.0 - float(b1) ** h.step)
    bc2_sqrt = f32(np.sqrt(1.0 - float(b2) ** h.step))
    gs = f32(h.gscale) * (f32(h.gsd) if h.gsd is not None else one)
    step_size = lr / bc1
    gk = g * gs
    pa = p * (one - lr * wd)
    ma = b1 * m + (one - b1) * gk
    va = b2 * v + (one - b2) * gk * gk
    denom = np.sqrt(va) / bc2_sqrt + eps
    pa = pa - step_size * (ma / denom)
    assert pa.dtype == f32 and ma.dtype == f32 and va.dtype == f32
    return pa, ma, va


def adam_piece(b, sl, h, mode, mutant, zero_grad, keep, lp, out):
    """one piece [sl] of the flat buffers `b` (p, g, m, v before) -> written into `out` (p, g, m, v, lp)"""
    p, g, m, v = (b[k][sl] for k in "pgmv")
    if mode == "emul":
        p2, m2, v2 = adam_emul(p, g, m, v, h)
    else:
        m2, _, v2, _ = ref_moments(p, g, m, v, h, mutant)
        m2, v2 = m2.astype(f32), v2.astype(f32)
        p2 = ref_param(p, m2, v2, h, mutant)[0].astype(f32)
        # where nothing but the decay acts, fp32 leaves no freedom: p * (1 - lr * wd) with both roundings (a slip of lr still shows)
        c = consts(h, mutant)
        z = (m2 == 0) & (v2 == 0)
        p2[z] = (p * (f32(1) - f32(c.lr) * f32(c.wd)))[z] if mutant != "coupled_decay" else p[z]
    out["p"][sl], out["m"][sl], out["v"][sl] = p2, m2, v2
    clear = bool(zero_grad) and mutant != "zero_grad_ignored"
    if keep and mutant != "keep_flag_ignored":
        clear = False
    if clear:
        out["g"][sl] = 0.0
    if lp:
        out["lp"][sl] = bf16_trunc(p2) if mutant == "lp_truncated" else bf16_rne(p2)


def verdict_adam_piece(fails, stats, before, got, sl, h, zero_grad, keep, lp, zero, where=""):
    """the checks of one updated piece: m', v' against fp64 from the inputs, p' against fp64 on the stored m', v', the exact ones"""
    p, g, m, v = (before[k][sl] for k in "pgmv")
    rm, cm, rv, cv = ref_moments(p, g, m, v, h)
    _rule(fails, stats, "m", got["m"][sl], rm, cm, K_DERIVED["m"], where)
    _rule(fails, stats, "v", got["v"][sl], rv, cv, K_DERIVED["v"], where)
    if np.isfinite(got["m"][sl]).all() and np.isfinite(got["v"][sl]).all() and (got["v"][sl] >= 0).all():
        rp, cp = ref_param(p, got["m"][sl], got["v"][sl], h)
        _rule(fails, stats, "p", got["p"][sl], rp, cp, K_DERIVED["p"], where)
    z = zero[sl] if zero is not None else np.zeros(p.size, dtype=bool)
    if z.any():  # g = m = v = 0: the update is exactly the decay
        dec = f32(1) - f32(h.lr) * f32(h.wd)
        if not ((bits32(got["m"][sl])[z] == 0).all() and (bits32(got["v"][sl])[z] == 0).all() and (bits32(got["p"][sl])[z] == bits32(p[z] * dec)).all()):
            fails.append(f"g = m = v = 0{where}: not exactly the decay")
    gb = bits32(got["g"][sl])
    if zero_grad and not keep:
        if not (gb == 0).all():
            fails.append(f"g{where}: a cleared gradient is not +0.0")
    elif not (gb == bits32(g)).all():
        fails.append(f"g{where}: a kept gradient changed")
    if lp and not (got["lp"][sl] == bf16_rne(got["p"][sl])).all():
        fails.append(f"lp{where}: not the RNE rounding of the stored p")


def _untouched(fails, name, buf, payload):
    bits = (bits32(buf) if buf.dtype == f32 else buf).copy()
    sent = SENT32 if buf.dtype == f32 else SENT16
    for sl in payload:
        bits[sl] = sent
    if not (bits == sent).all():
        fails.append(f"{name}: a write outside the pieces")


def simulate_adamw(case, inp, geo, mode, mutant=None):
    """-> the list of states after each update: dict(p, g, m, v, lp), full buffers"""
    sl, h0 = slice(LEAD, LEAD + case.n), inp["h"]
    states, cur = [], dict(p=inp["p"], m=inp["m"], v=inp["v"], lp=inp["lp"])
    for k in range(case.updates):
        b = dict(cur, g=inp["gs"][k])
        out = {key: (None if val is None else val.copy()) for key, val in b.items()}
        if mutant == "grid_stride_stops":
            trip = 8192 * 256 * 4
            adam_piece(b, slice(LEAD, LEAD + min(case.n, trip)), h0.at(k), mode, None, case.zg, 0, case.lp, out)
        else:
            adam_piece(b, sl, h0.at(k), mode, mutant, case.zg, 0, case.lp, out)
        states.append(out)
        cur = out
    return states


def verdict_adamw(case, inp, geo, got, stats=None):
    fails, sl, h0 = [], slice(LEAD, LEAD + case.n), inp["h"]
    before = dict(p=inp["p"], m=inp["m"], v=inp["v"])
    for k, st in enumerate(got):
        b = dict(before, g=inp["gs"][k])
        verdict_adam_piece(fails, stats, b, st, sl, h0.at(k), case.zg, 0, case.lp, np.concatenate([np.zeros(LEAD, bool), inp["zero"], np.zeros(LEAD, bool)]),
                           f" (update {k + 1})")
        for name in "pgmv":
            _untouched(fails, name, st[name], [sl])
        if case.lp:
            _untouched(fails, "lp", st["lp"], [sl])
        before = st
    return fails


# ---------------------------------------------------------------------------------------- LayerNorm-fold weights and bias
def _lanes(A, K):
    """[N, K] -> [N, J, 64, 4]: lane l of the row's wave holds elements 4 l + 256 j (zeros behind K)"""
    N, J = A.shape[0], -(-K // 256)
    pad = np.zeros((N, J * 256), dtype=A.dtype)
    pad[:, :K] = A
    return pad.reshape(N, J, 64, 4)


def fold_emul(W, gamma, beta, bias):
    """fold_ln_weights_kernel (and the fold inside adamw_items_kernel: the same additions) in float32 -> Wf bits [N, K], bias_f [N]"""
    N, K = W.shape
    Wl, gl, bl = _lanes(W, K), _lanes(np.broadcast_to(gamma, W.shape), K), _lanes(np.broadcast_to(beta, W.shape), K)
    J = Wl.shape[1]
    cs, bs = np.zeros((N, 64), dtype=f32), np.zeros((N, 64), dtype=f32)
    for j in range(J):
        w, g, b = Wl[:, j], gl[:, j], bl[:, j]
        cs = cs + ((w[..., 0] * g[..., 0] + w[..., 1] * g[..., 1]) + (w[..., 2] * g[..., 2] + w[..., 3] * g[..., 3]))
        bs = bs + ((w[..., 0] * b[..., 0] + w[..., 1] * b[..., 1]) + (w[..., 2] * b[..., 2] + w[..., 3] * b[..., 3]))
    cs, bs = _tree64(cs)[:, 0] / f32(K), _tree64(bs)[:, 0]
    q = np.zeros((N, J, 64, 4), dtype=np.uint16)
    carry = np.zeros((N, 64), dtype=f32)
    for j in range(J):
        for i in range(4):  # ln_fold_round4: fma(w, g, -cs) (one rounding: the product is exact in fp64) + carry -> bf16, the error carried on
            fma = (Wl[:, j, :, i].astype(f64) * gl[:, j, :, i].astype(f64) - cs[:, None].astype(f64)).astype(f32)
            target = fma + carry
            q[:, j, :, i] = bf16_rne(target)
            carry = target - bf16_val(q[:, j, :, i]).astype(f32)
    bias_f = bs + (bias if bias is not None else f32(0))
    return q.reshape(N, J * 256)[:, :K], bias_f.astype(f32)


def fold_ref(W, gamma, beta, bias, mutant=None):
    """fp64: the targets W gamma - mean_k(W gamma) and bias + W . beta, stored as a correct kernel would (feedback along the lane's
    group) or with a slip -> Wf bits, bias_f"""
    N, K = W.shape
    wg = W.astype(f64) * gamma.astype(f64)
    t = wg if mutant == "fold_not_centred" else wg - wg.mean(1, keepdims=True)
    tl = _lanes(t, K)
    J = tl.shape[1]
    q = np.zeros((N, J, 64, 4), dtype=np.uint16)
    carry = np.zeros((N, 64))
    for j in range(J):
        for i in range(4):
            target = (tl[:, j, :, i] + (0.0 if mutant == "fold_no_feedback" else carry)).astype(f32)
            q[:, j, :, i] = bf16_rne(target)
            carry = target.astype(f64) - bf16_val(q[:, j, :, i])
    bf = (W.astype(f64) * beta.astype(f64)).sum(1)
    if bias is not None and mutant != "fold_bias_missing":
        bf = bf + bias.astype(f64)
    return q.reshape(N, J * 256)[:, :K], bf.astype(f32)


def verdict_fold(fails, stats, W, gamma, beta, bias, Wf_bits, bias_f, where=""):
    """The checks of one fold (W: the fp32 weights the fold read).  With t = W gamma - mean_k(W gamma), T = the largest |t| of a lane's
    group (elements 4 l .. 4 l + 3 + 256 j of a row) and e32 = 2^-24 (K_cs mean_k |W gamma| + 3 T) (the fp32 error of the centring term; the
    roundings of the fma and of `+ carry`, each relative to a target of at most T (1 + 2^-7); one to spare):
      every stored target is t + carry_in + fp32 error with |carry_in| <= 2^-8 |previous target| (half a bf16 ulp), so it is at most
      T (1 + 2^-6) in size and its own rounding moves it by at most 2^-8 of that:
          element:   |Wf - t| <= 2 * 2^-8 T (1 + 2^-6) + e32                              (one rounding + the carried one)
          group:     |sum_group Wf - sum_group t| <= 2^-8 T (1 + 2^-6) + n_group e32        (the sum telescopes to the last carry)
          row:       |sum_row Wf| <= the sum of the group bounds (at most 64 carries)      (the targets of a row sum to 0)
      bias_f by the rule, cond = sum |W beta| + |bias|."""
    N, K = W.shape
    assert -(-K // 256) <= 5  # the trips K_DERIVED counts
    wg = W.astype(f64) * gamma.astype(f64)
    t = wg - wg.mean(1, keepdims=True)
    q = bf16_val(Wf_bits)
    tl, ql, live = _lanes(t, K), _lanes(q, K), _lanes(np.ones((N, K)), K)
    T = np.abs(tl).max(axis=(1, 3))                                                       # [N, 64]
    e32 = F32_EPS * (K_DERIVED["cs"] * np.abs(wg).mean(1)[:, None] + 3.0 * T)
    carry = U_BF16 * T * (1 + 2.0 ** -6) + 2.0 ** -126
    r_el = (np.abs(ql - tl) / (2 * carry + e32)[:, None, :, None]).max()
    n_g = live.sum(axis=(1, 3))
    r_gr = (np.abs((ql - tl).sum(axis=(1, 3))) / (carry + n_g * e32))[n_g > 0].max()
    r_row = (np.abs(q.sum(1)) / ((carry + n_g * e32) * (n_g > 0)).sum(1)).max()
    for name, r in (("Wf element", r_el), ("Wf group sum", r_gr), ("Wf row sum", r_row)):
        if stats is not None:
            stats.add(name, float(r))
        if not r <= 1.0:
            fails.append(f"{name}{where}: err / allowed {r:.3g}")
    wb = W.astype(f64) * beta.astype(f64)
    b64 = bias.astype(f64) if bias is not None else np.zeros(N)
    _rule(fails, stats, "bias_f", bias_f, wb.sum(1) + b64, np.abs(wb).sum(1) + np.abs(b64), K_DERIVED["bias_f"], where)


def simulate_fold(case, inp, geo, mode, mutant=None):
    out = []
    for e, (wf, bf) in zip(inp["entries"], inp["fold_bufs"]):
        wf, bf = wf.copy(), bf.copy()
        q, b = fold_emul(e["W"], e["gamma"], e["beta"], e["bias"]) if mode == "emul" else fold_ref(e["W"], e["gamma"], e["beta"], e["bias"], mutant)
        wf[LEAD:LEAD + q.size], bf[LEAD:LEAD + b.size] = q.reshape(-1), b
        out.append((wf, bf))
    return dict(folds=out)


def verdict_fold_case(case, inp, geo, got, stats=None):
    fails = []
    for i, (e, (wf, bf)) in enumerate(zip(inp["entries"], got["folds"])):
        N, K = e["N"], e["K"]
        _untouched(fails, f"Wf {i}", wf, [slice(LEAD, LEAD + N * K)])
        _untouched(fails, f"bias_f {i}", bf, [slice(LEAD, LEAD + N)])
        verdict_fold(fails, stats, e["W"], e["gamma"], e["beta"], e["bias"], wf[LEAD:LEAD + N * K].reshape(N, K), bf[LEAD:LEAD + N], f" (entry {i}: {N} x {K})")
    return fails


# ------------------------------------------------------------------------------------------------------- js2t_adamw_items
def _lpt_image(lp_piece, R, Cc, geo, mutant, old):
    """the transposed bf16 image [Cc, R] of a matrix's shadow as the kernel's units write it; `old`: what the buffer held"""
    UR, UC = geo["rows"], geo["cols"]
    img = lp_piece.reshape(R, Cc).T.copy()
    if mutant == "lpt_not_transposed":
        return lp_piece.copy()
    keep = np.zeros((Cc, R), dtype=bool)  # True: the slip leaves the element unwritten
    c, r = np.arange(Cc)[:, None], np.arange(R)[None, :]
    if mutant == "lpt_tail_rows_dropped":
        keep |= r >= R // 8 * 8
    if mutant == "lpt_second_half_dropped":
        keep |= (c % UC) >= UC // 2
    if mutant == "lpt_c0_ignored":   # every chunk writes at the first chunk's columns
        keep |= c >= UC
    if mutant == "lpt_r0_ignored":   # every strip writes at the first strip's rows
        keep |= r >= UR
    return np.where(keep, old.reshape(Cc, R), img).reshape(-1)


def _fold_operands(buf, f):
    """W, gamma, beta, bias of a fold as the flat parameter buffer `buf` holds them"""
    s, N, K = f["mat"], f["N"], f["K"]
    W = buf[s["off"]:s["off"] + N * K].reshape(N, K)
    bias = None if f["bias"] is None else buf[f["bias"]:f["bias"] + N]
    return W, buf[f["gamma"]:f["gamma"] + K], buf[f["beta"]:f["beta"] + K], bias


def simulate_items(case, inp, geo, mode, mutant=None):
    """-> dict(p, g, m, v, lp, lp_t: the flat buffers after every launch of the case; folds: [(Wf, bias_f)] between sentinels)"""
    lay, h = inp["lay"], inp["h"]
    out = {k: (None if inp[k] is None else inp[k].copy()) for k in ("p", "g", "m", "v", "lp", "lp_t")}
    folds = [(wf.copy(), bf.copy()) for wf, bf in inp["fold_bufs"]]
    for rows in lay["launches"]:
        for s in rows:
            sl = slice(s["off"], s["off"] + s["size"])
            adam_piece(inp, sl, h, mode, mutant, case.zg, s["keep"], out["lp"] is not None, out)
            if s["kind"] == 1 and out["lp_t"] is not None:
                out["lp_t"][sl] = _lpt_image(out["lp"][sl], s["rows"], s["cols"], geo, mutant, inp["lp_t"][sl])
    for f, (wf, bf) in zip(lay["folds"], folds):
        if not f["written"]:
            continue
        W, gamma, beta, bias = _fold_operands(out["p"], f)
        if mutant == "fold_old_gamma":
            gamma = _fold_operands(inp["p"], f)[1]
        q, b = fold_emul(W, gamma, beta, bias) if mode == "emul" else fold_ref(W, gamma, beta, bias, mutant)
        wf[LEAD:LEAD + q.size], bf[LEAD:LEAD + b.size] = q.reshape(-1), b
    out["folds"] = folds
    return out


def verdict_items(case, inp, geo, got, stats=None):
    fails, lay, h = [], inp["lay"], inp["h"]
    pieces, mats = [], []
    for rows in lay["launches"]:
        for s in rows:
            sl = slice(s["off"], s["off"] + s["size"])
            where = f" ({'flat' if s['kind'] == 0 else 'matrix'} {s['size'] if s['kind'] == 0 else (s['rows'], s['cols'])} at {s['off']})"
            verdict_adam_piece(fails, stats, inp, got, sl, h, case.zg, s["keep"], got["lp"] is not None, inp["zero"], where)
            pieces.append(sl)
            if s["kind"] == 1:
                mats.append(sl)
                if got["lp_t"] is not None and not (got["lp_t"][sl].reshape(s["cols"], s["rows"]) == got["lp"][sl].reshape(s["rows"], s["cols"]).T).all():
                    fails.append(f"lp_t{where}: not the transpose of lp")
    for name in "pgmv":
        _untouched(fails, name, got[name], pieces)
    if got["lp"] is not None:
        _untouched(fails, "lp", got["lp"], pieces)
    if got["lp_t"] is not None:
        _untouched(fails, "lp_t", got["lp_t"], mats)
    for i, (f, (wf, bf)) in enumerate(zip(lay["folds"], got["folds"])):
        N, K = f["N"], f["K"]
        if not f["written"]:  # wider than a unit: the kernel leaves this fold to js2t_fold_ln_weights
            _untouched(fails, f"Wf {i} (matrix wider than a unit)", wf, [])
            _untouched(fails, f"bias_f {i} (matrix wider than a unit)", bf, [])
            continue
        _untouched(fails, f"Wf {i}", wf, [slice(LEAD, LEAD + N * K)])
        _untouched(fails, f"bias_f {i}", bf, [slice(LEAD, LEAD + N)])
        W, gamma, beta, bias = _fold_operands(got["p"], f)  # the NEW weights, gamma, beta and bias, as stored
        verdict_fold(fails, stats, W, gamma, beta, bias, wf[LEAD:LEAD + N * K].reshape(N, K), bf[LEAD:LEAD + N], f" (fold {i}: {N} x {K})")
    return fails


# ------------------------------------------------------------------------------------------------------------------ dispatch
SIMULATE = {"clip": simulate_sumsq, "ranges": simulate_sumsq, "adamw": simulate_adamw, "items": simulate_items, "fold": simulate_fold}
VERDICT = {"clip": verdict_sumsq, "ranges": verdict_sumsq, "adamw": verdict_adamw, "items": verdict_items, "fold": verdict_fold_case}


def simulate(case, inp, geo, mode, mutant=None):
    return SIMULATE[case.op](case, inp, geo, mode, mutant)


def verdict(case, inp, geo, got, stats=None):
    return VERDICT[case.op](case, inp, geo, got, stats)


# ------------------------------------------------------------------------------------------------------------------- mutants
def _small_adam(c):
    return c.op == "adamw" and not c.big


def _bc(c, b):
    return 1.0 - b ** c.step


def _mats(c):
    return [s for s in c.launches[-1] if s["kind"] == 1] if c.op == "items" else []


def mutants(geo):
    """[(name, applies(case))]: a mutant applies where it computes something else than the reference, by more than the rule allows"""
    SQ, UR, UC = geo["sq"], geo["rows"], geo["cols"]
    both = lambda c: c.op == "items" and c.shadows == "both"  # noqa: E731
    has_fold = lambda c: c.op == "fold" or any(s.get("fold") and s["cols"] <= UC for s in _mats(c))  # noqa: E731
    return [
        ("coupled_decay", lambda c: _small_adam(c) and c.wd > 0),
        ("sqrt_bc2_missing", lambda c: _small_adam(c) and _bc(c, c.betas[1]) < 0.99),
        ("eps_inside_sqrt", lambda c: _small_adam(c) and c.n >= 1020),  # moves the elements whose v' is small (the 0.01 blocks)
        ("step_size_without_bc1", lambda c: _small_adam(c) and _bc(c, c.betas[0]) < 0.99),
        ("gscale_dropped", lambda c: _small_adam(c) and c.gsd),
        ("gscale_dev_dropped", lambda c: _small_adam(c) and c.gsd),
        ("v_from_unscaled_gradient", lambda c: _small_adam(c) and c.gsd),
        ("device_step_ignored", lambda c: _small_adam(c) and c.dev),
        ("lr_dev_ignored", lambda c: _small_adam(c) and c.dev),
        ("lp_truncated", lambda c: (_small_adam(c) and c.lp) or (c.op == "items" and c.shadows != "none")),
        ("zero_grad_ignored", lambda c: (_small_adam(c) or c.op == "items") and c.zg),
        ("keep_flag_ignored", lambda c: c.op == "items" and c.zg and any(s["keep"] for rows in c.launches if rows for s in rows)),
        ("grid_stride_stops", lambda c: c.op == "adamw" and c.big),
        ("last_partial_block_dropped", lambda c: (c.op == "clip" and c.n % SQ != 0) or c.op == "ranges"),
        ("tail_dropped", lambda c: (c.op == "clip" and c.n % 4 != 0) or (c.op == "ranges" and any(n % 4 for n in c.lens))),
        ("block_range_off_by_one", lambda c: c.op == "ranges" and len(c.lens) > 1),
        ("p0_ignored", lambda c: c.op == "ranges" and c.p0 != 0),
        ("clip_without_1e-6", lambda c: c.op == "clip" and c.clip == "tiny"),
        ("clip_not_capped", lambda c: c.op == "clip" and c.clip == "above"),
        ("lpt_not_transposed", lambda c: both(c) and any(s["rows"] > 1 for s in _mats(c))),
        ("lpt_tail_rows_dropped", lambda c: both(c) and any(s["rows"] % 8 for s in _mats(c))),
        ("lpt_second_half_dropped", lambda c: both(c) and any(s["cols"] > UC // 2 for s in _mats(c))),
        ("lpt_c0_ignored", lambda c: both(c) and any(s["cols"] > UC for s in _mats(c))),
        ("lpt_r0_ignored", lambda c: both(c) and any(s["rows"] > UR for s in _mats(c))),
        ("fold_not_centred", has_fold),
        ("fold_no_feedback", has_fold),
        ("fold_bias_missing", has_fold),
        ("fold_old_gamma", lambda c: c.op == "items" and has_fold(c)),
    ]


MUTANTS = [name for name, _ in mutants(dict(sq=1, rows=1, cols=1))]  # the names; which cases each applies to depends on the unit sizes
