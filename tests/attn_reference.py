"""Plain fp64 attention for the fused-attention tests (tests/test_hip_attention_ref.py): CPU only, no kernels, no oracle.

reference()  exact fp64 attention (forward and every gradient) on the bf16-rounded inputs - the expected value of every test.
emulate()    the same computation with roundings only where joeys2t_amd/csrc/attention.hip rounds.  It is NEVER the expected
             value: its distance from reference() says how large legitimate rounding error is at a given case.
make_case()  "loud" inputs: whatever a kernel must not read (masked / padded keys, guard rows, neighbouring columns) is large,
             and what it must not count twice (last live key, last query row) weighs much.
MUTANTS      deliberately wrong variants of reference(): what a plausible kernel slip computes.
judge()      the ONE tolerance rule every comparison goes through.
"""
import math

import torch

BF16_ULP = 2.0 ** -8   # one bf16 ulp of a stored result (8 significant bits)
FACTOR = 2.5           # HIP against fp64, measured by what the working-precision computation misses (test_hip_config_width.py)
LSE_TOL = 1e-4         # the project's fp32 parity tolerance
GUARD = 3              # guard rows behind the last row of every buffer
SENT16 = 0x7FA5        # sentinel bit pattern of bf16 output buffers (a NaN: no arithmetic produces it)
SENT32 = 0x7FA5A5A5    # the same for f32 buffers (lse)


def key_tile(dh):
    """Keys per LDS image of the fused kernels (Geo<DH>::KT)."""
    return 8192 // dh


# ----------------------------------------------------------------------------------------------------------------- cases
class Case:
    """One attention problem.  q / d_out [B, Tq, H*dh], k / v [B, Tk, H*dh] bf16; mask: what the kernel is given (bool, broadcasts
    from [B|1, 1|Tq, Tk]) or None; live [B, Tq, Tk]: the same, expanded; rel f32 [H, 2R+1] or None."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def d(self):
        return self.H * self.dh

    def key_live(self):
        """[B, Tk]: keys some query row attends to."""
        return self.live.any(1)

    def last_key(self):
        """index of the last live key of every entry"""
        kl = self.key_live()
        return [int(kl[b].nonzero().max()) for b in range(self.B)]


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def make_case(name, dh, seed, B, H, Tq, Tk, mask=None, R=0):
    g = torch.Generator().manual_seed(seed)
    d = H * dh
    q, k, v, go = (_randn(g, B, T, d) for T in (Tq, Tk, Tk, Tq))
    live = torch.ones(B, Tq, Tk, dtype=torch.bool) if mask is None else mask.expand(B, Tq, Tk).clone()
    dead = ~live.any(1)  # keys nobody attends to (padding): a read of one of them must dominate the row
    k[dead] = 8.0 * _randn(g, int(dead.sum()), d)
    v[dead] = 100.0 * _randn(g, int(dead.sum()), d)
    q = q.bfloat16()
    case = Case(name=name, dh=dh, seed=seed, B=B, H=H, Tq=Tq, Tk=Tk, mask=None if mask is None else mask.contiguous(), live=live, R=R)
    # the last live key of an entry is, head by head, 3 x one of the query rows that see it: that row's probability sits on this
    # key, and a last key counted twice moves its log-sum-exp by log 2.  Where another row can be had it is not the last query row
    # (the one with the 16-fold d_out below), and the key is made orthogonal to that row: a saturated softmax row turns the
    # rounding of `out` inside delta = rowsum(dO * O) into an error of dS that grows with |dO| - legitimate, but it would set the
    # emulation's worst row, and with it the bound of every other row, 16 times higher than need be.  Under a causal or band mask
    # only the last query row sees the last key: nothing is planted there (a key counted twice still moves lse by >= 1 / Tk)
    for b, kl in enumerate(case.last_key()):
        rows = live[b, :, kl].nonzero().flatten()
        if Tq > 1:
            rows = rows[rows != Tq - 1]
        for h in range(H if len(rows) else 0):
            hs = slice(h * dh, (h + 1) * dh)
            r = int(rows[(5 * h + 3 * b) % len(rows)])
            k[b, kl, hs] = 3.0 * q[b, r, hs].float()
            if r != Tq - 1:
                u = q[b, Tq - 1, hs].float()
                k[b, kl, hs] -= (k[b, kl, hs] @ u) / (u @ u) * u
    go[:, Tq - 1] *= 16.0  # a last query row counted twice in dK / dV is loud
    case.q, case.k, case.v, case.d_out = q, k.bfloat16(), v.bfloat16(), go.bfloat16()
    case.rel = (0.7 * _randn(g, H, 2 * R + 1)).contiguous() if R else None
    return case


def pad_mask(Tk, lens):
    return (torch.arange(Tk)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(1)  # [B, 1, Tk]


def causal_mask(B, Tq, Tk):
    """bottom-right aligned: row q sees keys 0 .. q + Tk - Tq (every row sees at least one)"""
    m = torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None] + (Tk - Tq)
    return m.unsqueeze(0).expand(B, -1, -1).contiguous()


def band_mask(Tq, Tk, lens, width):
    """row q of entry b sees `width` keys from lo_b(q) = q (len_b - width) // (Tq - 1): the band walks from key 0 to the entry's
    last key, so the rows of the second half start at or beyond the first key tile; nothing behind len_b is live"""
    qi, ki = torch.arange(Tq)[:, None], torch.arange(Tk)[None, :]
    out = []
    for n in lens:
        lo = qi * (n - width) // (Tq - 1)
        out.append((ki >= lo) & (ki < lo + width) & (ki < n))
    return torch.stack(out)


def case_names(dh):
    return ["A", "B", "C", "D"] + (["D70"] if dh == 64 else []) + ["E", "F", "G1", "G2", "H"]


def build_case(name, dh, R=0):
    """The geometries of the test plan, as Tq x Tk with KT = key_tile(dh); B = 2, H = 2 unless stated."""
    KT = key_tile(dh)
    seed = 1000 * (dh // 64) + 17 * sum(map(ord, name)) + R
    mk = lambda B, H, Tq, Tk, mask=None: make_case(name, dh, seed, B, H, Tq, Tk, mask, R)  # noqa: E731
    if name == "A":
        return mk(2, 2, 1, 1)
    if name == "B":
        return mk(2, 2, 17, KT - 1, pad_mask(KT - 1, [KT - 1, 1]))
    if name == "C":
        return mk(2, 2, 64, KT)  # exactly one tile, every key live
    if name == "D":
        return mk(2, 2, 65, KT + 1, pad_mask(KT + 1, [KT + 1, KT]))
    if name == "D70":
        return mk(2, 2, 65, 70, pad_mask(70, [70, 65]))  # head size 64: the second half of the 128-row image
    if name == "E":
        return mk(2, 2, 63, 2 * KT + 1, causal_mask(2, 63, 2 * KT + 1))
    if name in ("F", "Fdead"):
        Tq, Tk = 129, 3 * KT - 1
        m = band_mask(Tq, Tk, [Tk, Tk - 9], KT - 1)
        if name == "Fdead":  # forward only: two query rows without any live key
            m[0, 70] = False
            m[1, 3] = False
        return mk(2, 2, Tq, Tk, m)
    if name == "G1":  # one key mask for every entry and row
        m = torch.ones(1, 1, 64, dtype=torch.bool)
        m[0, 0, 7] = False
        m[0, 0, 59:] = False
        return mk(2, 2, 130, 64, m)
    if name == "G2":  # one [Tq, Tk] mask for every entry
        m = (torch.arange(64)[None, :] <= torch.arange(130)[:, None] * 63 // 129).unsqueeze(0)
        return mk(2, 2, 130, 64, m)
    if name == "H":
        return mk(2, 3, 33, KT + 17, pad_mask(KT + 17, [KT + 17, KT + 2]))
    raise KeyError(name)


def cpu_keep(case, p, seed=0):
    """A keep mask for the CPU self-check (on the GPU the mask is the kernels' own, fetched through ops.softmax_fwd)."""
    g = torch.Generator().manual_seed(seed + 99)
    return torch.rand(case.B, case.H, case.Tq, case.Tk, generator=g) >= p


# ---------------------------------------------------------------------------------------------- fused buffers, sentinels
def poison(rows, cols, seed):
    return (100.0 * _randn(torch.Generator().manual_seed(seed), rows, cols)).bfloat16()


def input_buffers(cases):
    """Operands as the product holds them - `cases`: one Case, or the entries of a packed batch (each B = 1), stacked row-wise.
    q at column d + 8 of a [rows + GUARD, 3d + 8] buffer, k at column 8 and v at column d + 8 of a [rows + GUARD, 2d + 8] buffer,
    d_out at column 8 of a [rows + GUARD, d + 16] buffer; everything else (other columns, guard rows) is 100 x randn."""
    cases = cases if isinstance(cases, (list, tuple)) else [cases]
    d = cases[0].d
    cat = lambda name: torch.cat([getattr(c, name).reshape(-1, d) for c in cases])  # noqa: E731
    q, k, v, go = cat("q"), cat("k"), cat("v"), cat("d_out")
    return _place(q, k, v, go, q.shape[0], k.shape[0])


def _place(q, k, v, go, qrows, krows):
    d = q.shape[1]
    qbuf, kvbuf, gobuf = poison(qrows + GUARD, 3 * d + 8, 1), poison(krows + GUARD, 2 * d + 8, 2), poison(qrows + GUARD, d + 16, 3)
    qbuf[:q.shape[0], d + 8:2 * d + 8] = q
    kvbuf[:k.shape[0], 8:d + 8] = k
    kvbuf[:v.shape[0], d + 8:2 * d + 8] = v
    gobuf[:go.shape[0], 8:d + 8] = go
    return dict(qbuf=qbuf, q_off=d + 8, kvbuf=kvbuf, k_off=8, v_off=d + 8, gobuf=gobuf, go_off=8)


def sentinel_bf16(rows, cols, device=None):
    return torch.full((rows, cols), SENT16, dtype=torch.int16, device=device).view(torch.bfloat16)


def sentinel_f32(n, device=None):
    return torch.full((n,), SENT32, dtype=torch.int32, device=device).view(torch.float32)


def untouched(buf, payload):
    """True if every element of a sentinel-filled buffer outside `payload` (a list of index tuples) still holds the sentinel."""
    bits = buf.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32).clone()
    sent = SENT16 if buf.dtype == torch.bfloat16 else SENT32
    for idx in payload:
        bits[idx] = sent
    return bool((bits == sent).all())


# ------------------------------------------------------------------------------------------------------------ the mathematics
def _heads(x, H):
    B, T, d = x.shape
    return x.double().view(B, T, H, d // H).permute(0, 2, 1, 3)  # [B, H, T, dh]


def _rel_index(case, mutant):
    qi, ki = torch.arange(case.Tq)[:, None], torch.arange(case.Tk)[None, :]
    R, n = case.R, 2 * case.R + 1
    dist = ki - qi + (1 if mutant == "rel_off_by_one" else 0)
    if mutant == "rel_no_clamp":  # an unclamped index walks into the neighbouring heads' rows of the table
        return None, dist + R
    return dist.clamp(-R, R) + R, None


def _attention(case, d_out=None, keep=None, p=0.0, rounded=False, o_given=None, mutant=None):
    """reference (rounded=False) / emulate (rounded=True) / a mutant of the reference: everything [B, H, Tq, Tk] in fp64."""
    bf = (lambda x: x.bfloat16().double()) if rounded else (lambda x: x)
    B, H, Tq, Tk, dh = case.B, case.H, case.Tq, case.Tk, case.dh
    scale, inv_keep = 1.0 / math.sqrt(dh), 1.0 / (1.0 - p)
    qh, kh, vh = _heads(case.q, H), _heads(case.k, H), _heads(case.v, H)
    live = case.live
    last = case.last_key()
    if mutant == "leak_first_masked_key":
        live = live.clone()
        for b in range(B):
            if last[b] + 1 < Tk:
                live[b, :, last[b] + 1] = True
    elif mutant == "boundary_shifted":
        live = torch.cat([live[:, :, :1], live[:, :, :-1]], 2) & case.key_live()[:, None, :]
    elif mutant == "mask_of_next_entry":
        live = live.roll(-1, 0)
    S = (qh @ kh.transpose(2, 3)) * scale
    idx = None
    if case.rel is not None:
        idx, raw = _rel_index(case, mutant)
        if idx is None:
            flat = case.rel.double().flatten()
            bias = torch.stack([flat[(raw + h * (2 * case.R + 1)) % flat.numel()] for h in range(H)])
            idx = raw.clamp(0, 2 * case.R)
        else:
            bias = case.rel.double()[:, idx]
        S = S + bias.unsqueeze(0)
    if mutant == "last_key_twice":
        for b in range(B):
            S[b, :, :, last[b]] += math.log(2.0)
    S = S.masked_fill(~live[:, None], float("-inf"))
    lse = torch.logsumexp(S, -1)
    if keep is None:
        keep = torch.ones(B, H, Tq, Tk, dtype=torch.bool)
    if mutant == "keep_shifted_by_a_key":
        keep = keep.roll(1, 3)
    elif mutant == "keep_of_next_row":
        keep = keep.reshape(-1, Tk).roll(-1, 0).view(B, H, Tq, Tk)
    kp = keep.double()
    # forward: the kernel rounds the UNNORMALISED probabilities exp(s - max), dropped but not yet scaled, to bf16 for P V; the row sum
    # is taken from the unrounded ones; 1 / ((1 - p) sum) is applied to the fp32 accumulator, the result rounded to bf16
    mx = S.amax(-1, keepdim=True)
    mx = torch.where(mx == float("-inf"), torch.zeros_like(mx), mx)
    Pu = torch.exp(S - mx)
    li = Pu.sum(-1, keepdim=True)
    out = bf((bf(Pu * kp) @ vh) * (inv_keep / li))  # a row without live keys: 0 / 0 = NaN, as the kernels document
    res = dict(out=out.permute(0, 2, 1, 3).reshape(B, Tq, H * dh), lse=lse)
    if d_out is None:
        return res
    # backward
    gh = _heads(d_out, H)
    P = torch.exp(S - lse.unsqueeze(-1))
    o_for_delta = out if o_given is None else _heads(o_given, H)
    delta = (gh * o_for_delta).sum(-1, keepdim=True)  # from the bf16 output the backward is handed (emulate) / the exact one
    if mutant == "delta_without_dropout_scale":
        delta = delta * (1.0 - p)
    dSp = P * (kp * (gh @ vh.transpose(2, 3)) - delta * (1.0 - p))  # x scale / (1 - p) = dS; the kernels round THIS to bf16
    qw = torch.ones(Tq, dtype=torch.float64)
    if mutant == "last_query_twice":
        qw[Tq - 1] = 2.0
    dSb, Pd = bf(dSp), bf(P * kp)
    dq = bf((dSb @ kh) * (scale * inv_keep))
    dk = bf(((dSb * qw[:, None]).transpose(2, 3) @ qh) * (scale * inv_keep))
    dv = bf(((Pd * qw[:, None]).transpose(2, 3) @ gh) * (1.0 if mutant == "dv_without_dropout_scale" else inv_keep))
    merge = lambda x: x.permute(0, 2, 1, 3).reshape(B, x.shape[2], H * dh)  # noqa: E731
    res.update(dq=merge(dq), dk=merge(dk), dv=merge(dv))
    if case.rel is not None:
        d_rel = torch.zeros(H, 2 * case.R + 1, dtype=torch.float64)
        for h in range(H):
            d_rel[h].index_add_(0, idx.flatten(), (dSp[:, h].sum(0) * inv_keep).flatten())
        res["d_rel"] = d_rel
    return res


def reference(case, d_out=None, keep=None, p=0.0, mutant=None):
    """Exact fp64 attention on the bf16-rounded inputs: out [B, Tq, d], lse [B, H, Tq] (log-sum-exp of the masked, biased scores,
    before dropout) and, for a d_out, dq / dk / dv / d_rel."""
    return _attention(case, d_out, keep, p, rounded=False, mutant=mutant)


def emulate(case, d_out=None, keep=None, p=0.0, o_given=None):
    """The same with the kernels' roundings: P (unnormalised, dropped, unscaled) to bf16 in front of P V; out to bf16; delta from
    the bf16 out the backward is given (o_given; default: its own); dS to bf16 in front of the dQ / dK products; P o keep to bf16 in
    front of the dV product; dq / dk / dv to bf16."""
    return _attention(case, d_out, keep, p, rounded=True, o_given=o_given)


def _differs(a, b):
    return a is not None and b is not None and not torch.equal(a, b)


def _clipped_live_pair(c):
    dist = (torch.arange(c.Tk)[None, :] - torch.arange(c.Tq)[:, None]).abs()
    return bool((c.live & (dist > c.R)[None]).any())


# (name, applies(case, p)): a mutant applies where it computes something else than the reference
MUTANTS = [
    ("leak_first_masked_key", lambda c, p: any(k + 1 < c.Tk for k in c.last_key())),                       # (a)
    ("last_key_twice", lambda c, p: True),                                                                  # (b)
    ("boundary_shifted", lambda c, p: c.mask is not None and c.mask.shape[1] == c.Tq and c.Tq > 1),       # (c)
    ("last_query_twice", lambda c, p: True),                                                                # (d)
    ("keep_shifted_by_a_key", lambda c, p: p > 0),                                                          # (e)
    ("keep_of_next_row", lambda c, p: p > 0),                                                               # (f)
    ("rel_off_by_one", lambda c, p: c.rel is not None),                                                     # (g)
    ("rel_no_clamp", lambda c, p: c.rel is not None and _clipped_live_pair(c)),                             # (g)
    ("dv_without_dropout_scale", lambda c, p: p > 0),                                                       # (h)
    ("mask_of_next_entry", lambda c, p: c.mask is not None and c.mask.shape[0] > 1 and _differs(c.live, c.live.roll(-1, 0))),  # (i)
    ("delta_without_dropout_scale", lambda c, p: p > 0),                                                    # (j)
]


# ------------------------------------------------------------------------------------------------------ the tolerance rule
def _row_err(x, ref, H, rho):
    B, T, d = ref.shape
    diff = (x.double() - ref).view(B, T, H, d // H).norm(dim=-1)
    return diff / ref.view(B, T, H, d // H).norm(dim=-1).clamp_min(rho)


def judge(kind, got, ref, emu, H=1, skip=None):
    """THE tolerance rule.  -> (ok, ratio, text) with ratio = worst error of `got` / worst error E of the emulation.
    kind "rows" (out, dq per query row and head; dk, dv per key row and head; [B, T, H*dh]):
        err_row = |got_row - ref_row|_2 / max(|ref_row|_2, rho), rho = the median norm of the tensor's live rows (near-zero rows
        are put on the tensor's own scale; a row counts as live from 2^-8 of the largest row norm on); every row must stay within
        max(2.5 E, 2^-8), E = the largest err_row of emulate().
    kind "table" (d_rel): the same over the whole table, relative to max |ref|.
    kind "lse": |got - ref| <= 1e-4 wherever ref is finite; got == -inf where ref is (emu is not looked at).
    skip [B, T] bool: rows left out (ONLY the fully masked query rows of the forward-only case; their values are asserted apart)."""
    got, ref = got.double(), ref.double()
    if kind == "lse":
        dead = ref == float("-inf")
        ok_dead = bool((got[dead] == float("-inf")).all())
        err = (got[~dead] - ref[~dead]).abs()
        worst = float(err.max()) if err.numel() else 0.0
        fin = bool(torch.isfinite(got[~dead]).all())
        return ok_dead and fin and worst <= LSE_TOL, worst / LSE_TOL, f"lse: worst |got - ref| {worst:.2e} (allowed {LSE_TOL:.0e})"
    emu = emu.double()
    if kind == "table":
        scale = float(ref.abs().max())
        err, E = float((got - ref).abs().max()) / scale, float((emu - ref).abs().max()) / scale
        errs_ok = math.isfinite(err)
    else:
        B, T, d = ref.shape
        use = torch.ones(B, T, dtype=torch.bool) if skip is None else ~skip
        norms = ref.view(B, T, H, d // H).norm(dim=-1)[use]
        # live rows: those with a gradient / output to speak of.  Rows of masked keys are exactly 0, and an entry with ONE live key
        # has dq = dk = 0 up to fp64 noise (case B): neither may drag the median, and with it rho, to nothing
        live = norms[norms > BF16_ULP * norms.max()]
        rho = float(live.median()) if live.numel() else 1.0
        e_got, e_emu = _row_err(got, ref, H, rho)[use], _row_err(emu, ref, H, rho)[use]
        errs_ok = bool(torch.isfinite(e_got).all())
        err, E = float(e_got.nan_to_num(float("inf")).max()), float(e_emu.max())
    bound = max(FACTOR * E, BF16_ULP)
    ratio = err / E if E > 0 else (0.0 if err == 0 else float("inf"))
    return errs_ok and err <= bound, ratio, f"worst {err:.3e}, emulation E {E:.3e}, allowed {bound:.3e}, err/E {ratio:.2f}"


def judge_all(got, ref, emu, H, names, skip=None):
    """judge() over several outputs -> (all ok, {name: ratio}, [text of every failure])"""
    ok, ratios, bad = True, {}, []
    for n in names:
        kind = "lse" if n == "lse" else "table" if n == "d_rel" else "rows"
        o, r, text = judge(kind, got[n], ref[n], None if n == "lse" else emu[n], H, skip if n in ("out", "dq") else None)
        ratios[n] = r
        if not o:
            ok = False
            bad.append(f"{n}: {text}")
    return ok, ratios, bad
