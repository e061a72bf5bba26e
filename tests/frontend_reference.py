"""Plain fp64 references for the audio front-end tests (tests/test_hip_frontend_ref.py, tests/test_frontend_reference_cpu.py): numpy
only, no kernels.  What joeys2t_amd/csrc/fbank.hip computes, written out the slow way:

fbank_frames()   Kaldi log-mel filterbank of frames cut from a float32 buffer, with the conditioning of every element.
judge_fbank()    |got - ref| <= K 2^-24 cond + 2 ulp32(|ref|); log(eps32) within 4 ulp32 where the filter is empty or the frame silent.
cmvn_ref() / judge_cmvn()            utterance statistics from fp64 sums and the bounds of the kernels' documented contract.
finalize_ref() / transform_ref() / judge_affine()   normalise + SpecAugment masks (+ pad to a batch).
MUTANTS          plausible slips, each a variant of a reference; the CPU self-check shows that the judges reject every one.
The case plans (FBANK_GEOS, WALKS, CMVN_*, FIN_*) are shared by the CPU self-check and the GPU tests.

K is not taken from the kernel: the project's float32 oracle (oracle.s2t_oracle.fbank) needs K <= 2 against fbank_frames() over the
plan (K_ORACLE_MAX, recomputed by the self-check); the kernel is held to 4 x that - a radix-2 transform with float32 twiddle tables
over nine or ten stages against numpy's mixed-radix transform, and __logf.
"""
import math

import numpy as np

from joeys2t_amd.helpers_for_audio import fbank_geometry, fbank_tables

EPS32 = float(np.finfo(np.float32).eps)
LOG_EPS32 = math.log(EPS32)
U24 = 2.0**-24
K_ORACLE_MAX = 2.0
K_KERNEL = 4 * K_ORACLE_MAX
SCALE = 2.0**15
PREEMPH = float(np.float32(0.97))  # the kernels are handed a float
VAR_FLOOR = float(np.float32(1e-10))
FB_WAVES, FB_MAX_GRID = 4, 2048     # fbank512_kernel: frames per block, blocks per launch
FIN_ONE_TRIP = 8192 * 256           # feature_finalize_kernel: elements the capped grid covers in one trip
TRF_ONE_TRIP = 16 * 256             # feature_transform_kernel: threads per utterance


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def bf16_bits(x32, truncate=False):
    """float32 -> bf16 bit patterns (uint16): round to nearest even, or the truncation a slip would do"""
    b = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    if not truncate:
        b = b + 0x7FFF + ((b >> 16) & 1)
    return (b >> 16).astype(np.uint16)


# ====================================================================================================== filterbank
def povey(n, denom=None):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / (denom or n - 1)))**0.85


def dense_filters(tab, n_bins, drop_tail=False):
    """[n_mel, n_bins] fp64 from the sparse tables the kernel reads"""
    M = len(tab["mel_start"])
    W = np.zeros((M, n_bins))
    for m in range(M):
        st, ln, wo = int(tab["mel_start"][m]), int(tab["mel_len"][m]), int(tab["mel_woff"][m])
        if drop_tail:
            ln -= ln % 4
        W[m, st:st + ln] = tab["mel_w"][wo:wo + ln].astype(np.float64)
    return W


def fft_radix2(x, flip_stage=None):
    """decimation-in-time radix-2 transform of the rows of x [T, N] (fp64); flip_stage: that stage's twiddles conjugated"""
    T, N = x.shape
    lg = N.bit_length() - 1
    rev = np.array([int(format(i, f"0{lg}b")[::-1], 2) for i in range(N)])
    a = x[:, rev].astype(np.complex128)
    for s in range(1, lg + 1):
        half = 1 << (s - 1)
        w = np.exp(-2j * np.pi * np.arange(half) / (2 * half))
        if s == flip_stage:
            w = w.conj()
        a = a.reshape(T, -1, 2, half)
        top, bot = a[:, :, 0, :], a[:, :, 1, :] * w
        a = np.stack([top + bot, top - bot], 2).reshape(T, N)
    return a


def fbank_frames(buf, starts, win_len, n_fft, tab, mutant=None):
    """buf float32 [N]; starts int64 [T]: the first sample of every frame.  -> (val, cond), fp64 [T, n_mel]:
    val = log(max(E, eps32)), cond = |raw scaled frame|_2 sum_k w[m, k] 2 |X[t, k]| / max(E, eps32): what one float32 rounding of the
    frame norm in every spectrum bin does to log E, to first order."""
    M = len(tab["mel_start"])
    starts = np.asarray(starts, dtype=np.int64)
    if len(starts) == 0:
        return np.zeros((0, M)), np.zeros((0, M))
    with np.errstate(all="ignore"):
        x = buf[starts[:, None] + np.arange(win_len)[None, :]].astype(np.float64) * SCALE                  # 1, 2
        norm = np.sqrt((x * x).sum(1))
        if mutant != "no_dc_removal":
            x = x - x.mean(1, keepdims=True)                                                                # 3
        prev = np.concatenate([x[:, :1], x[:, :-1]], 1)
        if mutant == "preemph_first_sample_zero":
            prev[:, 0] = 0.0
        x = x - PREEMPH * prev                                                                              # 4
        x = x * (povey(win_len, win_len) if mutant == "window_over_n" else tab["window"].astype(np.float64))  # 5
        if mutant == "twiddle_sign":
            X = fft_radix2(np.pad(x, ((0, 0), (0, n_fft - win_len))), flip_stage=n_fft.bit_length() - 1)[:, :n_fft // 2 + 1]
        else:
            X = np.fft.rfft(x, n=n_fft, axis=1)                                                             # 6
        A = np.abs(X)
        A = A[:, 1:n_fft // 2 + 1] if mutant == "nyquist_bin_included" else A[:, :n_fft // 2]               # 7
        W = dense_filters(tab, n_fft // 2, drop_tail=mutant == "filter_tail_dropped")
        E = (A * A) @ W.T                                                                                   # 8
        Ec = np.maximum(E, EPS32)
        val = np.log(E if mutant == "no_log_floor" else Ec)                                                 # 9
        cond = norm[:, None] * ((2.0 * A) @ W.T) / Ec
        if mutant in ("bins_ge_64_dropped", "bins_ge_128_dropped"):
            val[:, 64 if mutant == "bins_ge_64_dropped" else 128:] = np.nan  # never written: the sentinel stays
    return val, cond


def judge_fbank(got, val, cond, floor, K=K_KERNEL):
    """-> (ok, worst err / allowed, K needed, text).  floor [T, n_mel] bool: empty filter or silent frame -> log(eps32) within 4 ulp32."""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return True, 0.0, 0.0, "no frames"
    ref = np.where(floor, LOG_EPS32, val)
    rnd = 2.0 * ulp32(ref)
    tol = np.where(floor, 4.0 * ulp32(LOG_EPS32), K * U24 * cond + rnd)
    err = np.abs(got - ref)
    ratio = np.where(err <= tol, err / tol, np.inf)
    judged = ~floor & (cond > 0)
    with np.errstate(all="ignore"):
        need = np.where(judged, np.maximum(err - rnd, 0.0) / (U24 * cond), 0.0)
    need = float(np.nan_to_num(need, nan=np.inf).max())
    i = np.unravel_index(int(np.argmax(np.nan_to_num(np.where(err <= tol, err / tol, np.inf), posinf=1e300))), err.shape)
    ok = bool((err <= tol).all())
    return ok, float(ratio.max()), need, f"worst at {i}: got {got[i]:.7g} ref {ref[i]:.7g} err {err[i]:.3e} allowed {tol[i]:.3e}; K needed {need:.2f}"


def tolerance_profile(val, cond, floor, K=K_KERNEL):
    """(share of the judged elements whose tolerance is at most 1e-4, the largest tolerance) - the conditions on the inputs"""
    tol = (K * U24 * cond + 2.0 * ulp32(val))[~floor]
    return float((tol <= 1e-4).mean()), float(tol.max())


def signal(n, sample_rate, rng, tone=0.3):
    """0.1 randn + 0.3 sin(2 pi 440 t), clipped: broadband, so that no mel bin is a small difference of large spectrum bins"""
    t = np.arange(n, dtype=np.float64) / sample_rate
    return np.clip(0.1 * rng.standard_normal(n) + tone * np.sin(2.0 * np.pi * 440.0 * t), -1.0, 1.0).astype(np.float32)


class FbankBatch:
    """A ragged batch in ONE buffer: NaN in front, between and behind the utterances, and behind an utterance's last full window."""

    def __init__(self, sample_rate, n_mel, n_samples, silent=(), seed=0, tab=None, tone=0.3):
        self.sample_rate, self.n_mel = sample_rate, n_mel
        self.win_len, self.shift, self.n_fft = fbank_geometry(sample_rate)
        self.tab = tab if tab is not None else fbank_tables(sample_rate, n_mel)
        rng = np.random.default_rng(seed)
        w, s = self.win_len, self.shift
        parts, self.sample_off, self.n_samples, self.frames, self.silent_utt = [np.full(5, np.nan, np.float32)], [], [], [], []
        pos = 5
        for u, n in enumerate(n_samples):
            T = 0 if n < w else 1 + (n - w) // s
            x = np.zeros(n, np.float32) if u in silent else signal(n, sample_rate, rng, tone)
            x[(w + (T - 1) * s if T else 0):] = np.nan
            self.sample_off.append(pos), self.n_samples.append(n), self.frames.append(T), self.silent_utt.append(u in silent)
            parts += [x, np.full(7, np.nan, np.float32)]
            pos += n + 7
        self.buf = np.concatenate(parts)
        self.frame_off = np.concatenate([[0], np.cumsum(self.frames)]).astype(np.int64)
        self.total = int(self.frame_off[-1])
        self._ref = None

    @classmethod
    def of_frames(cls, sample_rate, n_mel, frames, seed=0, tone=0.3):
        """utterances of the given frame counts (0: shorter than a window), each with a ragged tail no frame covers"""
        w, s, _ = fbank_geometry(sample_rate)
        return cls(sample_rate, n_mel, [w + (T - 1) * s + 37 if T else 123 for T in frames], seed=seed, tone=tone)

    def starts(self, mutant=None):
        """first sample of every frame of the launch; the run-walk mutants follow fbank512_kernel's frame_ptr"""
        fo, so, s = self.frame_off, self.sample_off, self.shift
        out = np.concatenate([so[u] + s * np.arange(T, dtype=np.int64) for u, T in enumerate(self.frames)] + [np.zeros(0, np.int64)])
        if mutant is None:
            return out
        per = self.per()
        for f0 in range(0, self.total, per):
            u = int(np.searchsorted(fo, f0, side="right")) - 1  # largest u with frame_off[u] <= f0
            u_beg, u_end, s_off = fo[u], fo[u + 1], so[u]
            for f in range(f0, min(self.total, f0 + per)):
                if mutant == "stale_sample_offset":
                    while f >= u_end:
                        u, u_beg = u + 1, u_end
                        u_end = fo[u + 1]
                elif f >= u_end:  # "empty_not_skipped": one step, whatever the next utterance holds
                    u, u_beg = u + 1, u_end
                    u_end, s_off = fo[u + 1], so[u]
                out[f] = s_off + (f - u_beg) * s
        return out

    def per(self):
        grid = min(FB_MAX_GRID, -(-self.total // FB_WAVES))
        return -(-self.total // (grid * FB_WAVES)) if self.total else 1

    def floor(self):
        silent = np.concatenate([np.full(T, q) for T, q in zip(self.frames, self.silent_utt)] + [np.zeros(0, bool)])
        return silent[:, None] | (np.asarray(self.tab["mel_len"]) == 0)[None, :]

    def reference(self):
        if self._ref is None:
            self._ref = fbank_frames(self.buf, self.starts(), self.win_len, self.n_fft, self.tab)
        return self._ref


# (sample_rate, n_mel): n_fft 512 takes fbank512_kernel, everything else fbank_kernel
GEOS_512 = [(16000, 80), (16000, 8), (16000, 64), (16000, 65), (16000, 128), (16000, 160), (11025, 80), (20000, 80), (20480, 80)]
GEOS_GENERIC = [(2000, 23), (4000, 40), (8000, 80), (8000, 160), (22050, 80), (32000, 80), (40960, 160)]
FBANK_GEOS = GEOS_512 + GEOS_GENERIC
REJECTED_RATES = [1000, 44100]
WALKS = {  # frames per utterance at 16 kHz, 80 bins -> per = ceil(total / (grid * 4)), grid capped at 2048
    "total8192_per1": [5000, 0, 3192],
    "total8193_per2": [5000, 0, 3193],
    "total10200_per2": [2500, 0, 1, 3000, 0, 0, 2999, 1700, 0],
    "total20000_per3": [0, 7001, 1, 0, 12998],
}
WALK_PER = {"total8192_per1": 1, "total8193_per2": 2, "total10200_per2": 2, "total20000_per3": 3}
WALK_SEED = {"total8192_per1": 0, "total8193_per2": 0, "total10200_per2": 2, "total20000_per3": 4}
_batches = {}


def geo_batch(sample_rate, n_mel, tab=None):
    """the per-geometry ragged batch: w - 1 (0 frames), w (1), w + s - 1 (1), w + s (2), w + 5 s + 3 (6), silence of 3 frames, 300"""
    key = ("geo", sample_rate, n_mel)
    if key not in _batches or tab is not None:
        w, s, _ = fbank_geometry(sample_rate)
        _batches[key] = FbankBatch(sample_rate, n_mel, [w - 1, w, w + s - 1, w + s, w + 5 * s + 3, w + 2 * s, 300], silent=(5, ),
                                   seed=sample_rate + n_mel, tab=tab)
    return _batches[key]


def walk_batch(name):
    key = ("walk", name)
    if key not in _batches:
        # noise alone, and a seed at which no element's tolerance exceeds 1e-2: among a million elements a one-weight filter meets
        # a spectrum bin of next to no energy somewhere, and the tone's share of the frame norm would make that element looser still
        _batches[key] = FbankBatch.of_frames(16000, 80, WALKS[name], seed=WALK_SEED[name], tone=0.0)
    return _batches[key]


def hand_tables(lens, n_fft=512, win_len=400, seed=5):
    """caller's own tables at n_fft 512: filter m has lens[m] weights in (0.25, 1.25), start + len <= n_fft / 2; a Hamming window,
    which unlike Povey's is not 0 at sample 0 - there the x[-1] := x[0] of the pre-emphasis shows in the result"""
    rng = np.random.default_rng(seed)
    tab = {k: v for k, v in fbank_tables(16000, 80).items() if k in ("tw_re", "tw_im")}
    tab["window"] = (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(win_len) / (win_len - 1))).astype(np.float32)
    starts = [int(rng.integers(0, n_fft // 2 - ln + 1)) for ln in lens]
    starts[-1] = n_fft // 2 - lens[-1]  # the last one ends on the last bin
    tab["mel_start"] = np.asarray(starts, np.int32)
    tab["mel_len"] = np.asarray(lens, np.int32)
    tab["mel_woff"] = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    tab["mel_w"] = (0.25 + rng.random(max(1, int(np.sum(lens))))).astype(np.float32)
    return tab


HAND_TABLES = {"out_of_lds": [201] * 12, "mixed_lengths": [0, 1, 3, 4, 5, 0, 5, 4, 3, 1]}


def hand_batch(name):
    """the per-geometry batch at 16 kHz with the caller's own tables"""
    key = ("hand", name)
    if key not in _batches:
        w, s, _ = fbank_geometry(16000)
        _batches[key] = FbankBatch(16000, len(HAND_TABLES[name]), [w - 1, w, w + s - 1, w + s, w + 5 * s + 3, w + 2 * s, 300], silent=(5, ),
                                   seed=len(name), tab=hand_tables(HAND_TABLES[name]))
    return _batches[key]


# ====================================================================================================== CMVN statistics
CMVN_F = [1, 5, 64, 80, 83, 85]
CMVN_F_REFUSED = [86, 256]
CMVN_LENS = [0, 1, 7, 8, 9, 12, 13, 97, 1000]
CMVN_MAX_FRAMES = [0, 5, 8, 40, 2000]
CMVN_SETTINGS = [(1, 1), (1, 0), (0, 1), (0, 0)]  # (norm_means, norm_vars)
CONST_VALUE = 2.5  # 2.5 and 6.25 are float32 numbers: the constant column's variance is exactly 0 in any precision


def cmvn_features(F, lens, max_frames, seed=0, lead=3, tail=4):
    """-> (feat float32 [lead + sum(lens) + tail, F], frame_off int64 relative to row `lead`, const column).  3 randn + a per-bin
    offset in [-10, 10]; the last column constant; NaN: the rows around the batch and every frame behind max_frames."""
    rng = np.random.default_rng(seed + 7 * F)
    off = rng.uniform(-10.0, 10.0, F)
    rows = int(np.sum(lens))
    x = (3.0 * rng.standard_normal((rows, F)) + off[None, :]).astype(np.float32)
    const = F - 1
    x[:, const] = CONST_VALUE
    fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if max_frames > 0:
        for u, T in enumerate(lens):
            x[fo[u] + min(T, max_frames):fo[u + 1]] = np.nan
    nan = lambda n: np.full((n, F), np.nan, np.float32)  # noqa: E731
    return np.concatenate([nan(lead), x, nan(tail)]), fo, const


def cmvn_ref(feat, frame_off, norm_means, norm_vars, max_frames, mutant=None):
    """feat float32 [rows, F] (row 0 = frame_off 0) -> fp64 dict: mean, istd [U, F], fill [U] as the kernels define them, and m (the
    mean itself), ex2 = E[x^2], var, all over the kept frames."""
    U, F = len(frame_off) - 1, feat.shape[1]
    m, ex2, var = np.zeros((U, F)), np.zeros((U, F)), np.zeros((U, F))
    for u in range(U):
        T = int(frame_off[u + 1] - frame_off[u])
        Tk = min(T, max_frames) if max_frames > 0 else T
        if Tk == 0:
            continue
        x = feat[frame_off[u]:frame_off[u] + (T if mutant == "cmvn_over_all_frames" else Tk)].astype(np.float64)
        s, q = x.sum(0), (x * x).sum(0)
        if mutant == "cmvn_pieces_overlap":  # piece p of 8 runs one frame into piece p + 1
            per = -(-Tk // 8)
            for p in range(8):
                tb = min(Tk, p * per) + per
                if tb < Tk:
                    s, q = s + x[tb], q + x[tb] * x[tb]
        n = x.shape[0] if mutant == "cmvn_over_all_frames" else Tk
        m[u], ex2[u] = s / n, q / n
        var[u] = ((x - m[u])**2).mean(0) if mutant is None else ex2[u] - m[u]**2
    with np.errstate(all="ignore"):
        istd = 1.0 / np.sqrt(var if mutant == "variance_not_clamped" else np.maximum(var, VAR_FLOOR)) if norm_vars else np.ones((U, F))
    with np.errstate(all="ignore"):
        fill = ((0.0 if norm_means else m) * istd).mean(1)
    return dict(mean=m if norm_means else np.zeros((U, F)), istd=istd, fill=fill, m=m, ex2=ex2, var=var)


def cmvn_as_kernel(ref, norm_means, norm_vars):
    """the float32 steps of the kernels' contract on the fp64 sums (m, sq, m * m, the difference each rounded): NEVER the expected
    value - the self-check uses it to show that the bounds leave room for a correct kernel"""
    f = np.float32
    m, sq = ref["m"].astype(f), ref["ex2"].astype(f)
    var = sq - m * m
    istd = (f(1) / np.sqrt(np.maximum(var, f(1e-10)))).astype(f) if norm_vars else np.ones_like(m)
    prod = ((f(0) * m if norm_means else m) * istd).astype(np.float64)
    return dict(mean=m if norm_means else np.zeros_like(m), istd=istd, fill=prod.mean(1).astype(f), m=m)


def judge_cmvn(got, ref, norm_means, norm_vars, const, m32=None):
    """got: mean, istd [U, F], fill [U] float32.  -> (ok, {name: worst err / allowed}, [failures]).
    mean   within 1 ulp32 of the fp64 mean (+ 2^-48 E|x| for the fp64 sums' own error); exactly 0 without norm_means.
    istd   where the fp64 variance exceeds 1e-6: relative error <= 4 2^-24 (E[x^2] + mean^2) / var + 2^-22 (the float32 variance takes
           four roundings: m, sq, m * m, the difference).  Column `const` and every utterance without frames (variance exactly 0):
           1 / sqrt(1e-10f) within 2 ulp32.  Elsewhere (a variance of rounding noise, such as any column of a one-frame utterance)
           the contract promises a positive finite number of at most that.  Exactly 1 without norm_vars.
    fill   exactly 0 with norm_means; otherwise within 2^-22 mean_c |m_c istd_c| of the fp64 mean over the bins of m_c istd_c, with
           m the kernel's own float32 mean (m32: what the same route returns under norm_means; default the rounded fp64 mean) and
           istd the values it has just returned - istd alone may be further from fp64 than 2^-22, by its own bound above, and is
           judged there.  Without norm_vars (istd = 1) the same bound is also asserted against the pure fp64 value."""
    mean, istd, fill = (np.asarray(got[k], dtype=np.float64) for k in ("mean", "istd", "fill"))
    ratios, bad = {}, []

    def rule(name, err, allowed):
        with np.errstate(all="ignore"):
            r = np.where(err <= allowed, np.where(allowed > 0, err / np.where(allowed > 0, allowed, 1.0), 0.0), np.inf)
        ratios[name] = max(ratios.get(name, 0.0), float(np.max(r, initial=0.0)))
        if not np.all(err <= allowed):
            i = np.unravel_index(int(np.argmax(np.nan_to_num(r, posinf=1e300))), r.shape)
            bad.append(f"{name} at {i}: err {np.asarray(err)[i]:.3e} allowed {np.asarray(allowed)[i]:.3e}")

    rule("mean", np.abs(mean - ref["mean"]), ulp32(ref["mean"]) + 2.0**-48 * np.sqrt(ref["ex2"]) if norm_means else np.zeros_like(mean))
    if not norm_vars:
        rule("istd", np.abs(istd - 1.0), np.zeros_like(istd))
    else:
        top = 1.0 / math.sqrt(VAR_FLOOR)
        exact = np.zeros(istd.shape, bool)
        exact[:, const] = True
        exact[(ref["ex2"] == 0).all(1)] = True
        wide = ref["var"] > 1e-6
        with np.errstate(all="ignore"):
            rel = 4.0 * U24 * (ref["ex2"] + ref["m"]**2) / ref["var"] + 2.0**-22
        rule("istd", np.abs(istd - ref["istd"])[wide & ~exact], (rel * ref["istd"])[wide & ~exact])
        rule("istd const", np.abs(istd - top)[exact], np.broadcast_to(2.0 * ulp32(top), istd.shape)[exact])
        rest = istd[~wide & ~exact]
        if not np.all((rest > 0) & (rest <= top + 2.0 * ulp32(top))):
            bad.append("istd: not in (0, 1 / sqrt(1e-10f)] where the variance is rounding noise")
    if norm_means:
        rule("fill", np.abs(fill), np.zeros_like(fill))
    else:
        m = (ref["m"].astype(np.float32) if m32 is None else np.asarray(m32)).astype(np.float64)
        terms = m * istd
        rule("fill", np.abs(fill - terms.mean(1)), 2.0**-22 * np.abs(terms).mean(1))
        if not norm_vars:
            rule("fill", np.abs(fill - ref["fill"]), 2.0**-22 * np.abs(ref["m"]).mean(1))
    return not bad, ratios, bad


# ====================================================================================================== batch writer, transform
FIN_F = [1, 80, 83]
FIN_LENS = [0, 1, 20, 57]
FIN_TMAX = [13, 57, 64]
FIN_CROPS = [None, 57, 60, "above"]  # "above": Tmax + 5
FIN_BIG = dict(U=3, Tmax=8750, F=80, lens=[8750, 8000, 0])  # 2,100,000 elements: 2848 more than one trip of the capped grid
PAD_VALUE = 1.0


def writer_inputs(F, lens, Tmax=None, seed=0, lead=2, tail=3):
    """-> feat float32 [lead + sum(lens) + tail, F] (NaN around the batch and in the rows t >= Tmax of a truncated utterance),
    frame_off, mean, istd [U, F], fill [U] float32"""
    rng = np.random.default_rng(seed + 11 * F + (Tmax or 0))
    U, rows = len(lens), int(np.sum(lens))
    x = (3.0 * rng.standard_normal((rows, F)) + 1.0).astype(np.float32)
    fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if Tmax is not None:
        for u, T in enumerate(lens):
            x[fo[u] + min(T, Tmax):fo[u + 1]] = np.nan
    nan = lambda n: np.full((n, F), np.nan, np.float32)  # noqa: E731
    mean = rng.standard_normal((U, F)).astype(np.float32)
    istd = (0.5 + rng.random((U, F))).astype(np.float32)
    fill = (10.0 * rng.standard_normal(U)).astype(np.float32)
    return np.concatenate([nan(lead), x, nan(tail)]), fo, mean, istd, fill


def finalize_masks(lens, F):
    """int32 [U, 8] = (f0, f, f0, f, t0, t, t0, t): masks on both edges (f0 + f = F, t0 + t = T), of width 0 at a non-zero start,
    overlapping, and a time mask that reaches past T"""
    out = np.zeros((len(lens), 8), np.int32)
    for u, T in enumerate(lens):
        fa = min(3, F)
        if u % 2 == 0:
            out[u] = [F - fa, fa if F > 1 else 0, max(1, F // 2), 0, max(T - 2, 0), min(2, T), 5, 0]
        else:
            fb = min(2, F - 1)
            out[u] = [0, min(4, F) if F > 1 else 0, fb, min(4, F - fb) if F > 1 else 0, max(T - 3, 0), 10, max(T - 5, 0), 4]
    return out


def _apply(x, mean, istd, fill, fmasks, tmasks):
    """(x - mean) istd, fill inside a mask, for one utterance (fp64) -> (values, |x - mean| istd, exact)"""
    T, F = x.shape
    if mean is not None:
        v, scale = (x - mean) * istd, np.abs(x - mean) * istd
    else:
        v, scale = x.copy(), np.zeros_like(x)
    exact = np.full((T, F), mean is None)
    hit = np.zeros((T, F), bool)
    c, t = np.arange(F)[None, :], np.arange(T)[:, None]
    for s0, wd in fmasks:
        hit |= (wd > 0) & (c >= s0) & (c < s0 + wd)
    for s0, wd in tmasks:
        hit |= (wd > 0) & (t >= s0) & (t < s0 + wd)
    v[hit] = fill if hit.any() else 0.0
    exact |= hit
    return v, scale, exact


def finalize_ref(feat, frame_off, mean, istd, fill, masks, Tmax, crop=None, pad_value=PAD_VALUE, mutant=None):
    """-> (ref, scale, exact), each [U, Tmax, F]: the padded batch in fp64, |x - mean| istd, and where it must match bit for bit
    (masked, padded, cropped, and everything when there is no normalisation)"""
    U, F = len(frame_off) - 1, feat.shape[1]
    crop = Tmax if crop is None else crop
    t = np.arange(Tmax)
    pad = np.where(t < crop, pad_value, 0.0) if mutant != "pad_value_behind_crop" else np.full(Tmax, pad_value)
    ref = np.broadcast_to(pad[None, :, None], (U, Tmax, F)).copy()
    scale, exact = np.zeros((U, Tmax, F)), np.ones((U, Tmax, F), bool)
    f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)  # noqa: E731
    mean, istd, fill = f64(mean), f64(istd), f64(fill)
    for u in range(U):
        T = int(min(frame_off[u + 1] - frame_off[u], Tmax))
        x = feat[frame_off[u]:frame_off[u] + T].astype(np.float64)
        mk = None if masks is None else masks[u].reshape(4, 2)
        ref[u, :T], scale[u, :T], exact[u, :T] = _apply(x, None if mean is None else mean[u], None if mean is None else istd[u],
                                                        None if mk is None else fill[u], [] if mk is None else mk[:2],
                                                        [] if mk is None else mk[2:])
        if mutant == "time_mask_in_padding" and mk is not None:
            for s0, wd in mk[2:]:
                ref[u, max(T, s0):max(T, min(Tmax, s0 + wd))] = fill[u]
    if mutant == "grid_stride_stops":
        ref.reshape(-1)[FIN_ONE_TRIP:] = np.nan  # never written: the sentinel stays
    return ref, scale, exact


def transform_ref(feat, frame_off, mean, istd, fill, masks, n_freq, n_time, mutant=None):
    """js2t_feature_transform on the ragged rows [frame_off[0], frame_off[U]) -> (ref, scale, exact), each [rows, F]"""
    U, F = len(frame_off) - 1, feat.shape[1]
    rows = int(frame_off[U])
    ref, scale, exact = np.zeros((rows, F)), np.zeros((rows, F)), np.ones((rows, F), bool)
    f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)  # noqa: E731
    mean, istd, fill = f64(mean), f64(istd), f64(fill)
    for u in range(U):
        a, b = int(frame_off[u]), int(frame_off[u + 1])
        x = feat[a:b].astype(np.float64)
        mk = None if masks is None else masks[u].reshape(n_freq + n_time, 2)
        ref[a:b], scale[a:b], exact[a:b] = _apply(x, None if mean is None else mean[u], None if mean is None else istd[u],
                                                  None if mk is None else fill[u], [] if mk is None else mk[:n_freq],
                                                  [] if mk is None else mk[n_freq:])
        if mutant == "grid_stride_stops":
            ref[a:b].reshape(-1)[TRF_ONE_TRIP:] = x.reshape(-1)[TRF_ONE_TRIP:]  # the input stays
    return ref, scale, exact


def transform_masks(lens, F, n_freq, n_time):
    """int32 [U, n_freq + n_time, 2]: frequency masks first; the last time mask reaches past T"""
    out = np.zeros((len(lens), n_freq + n_time, 2), np.int32)
    for u, T in enumerate(lens):
        for k in range(n_freq):
            out[u, k] = [(7 * u + 13 * k) % F, (u + 2 * k) % 5]
        for k in range(n_time):
            out[u, n_freq + k] = [(3 * u + 5 * k) % max(T, 1), (u + k) % 4]
        if n_time:
            out[u, -1] = [max(T - 2, 0), 9]
    return out


def judge_affine(got32, ref, scale, exact):
    """float32 output of the writer / the transform.  Normalised elements: |got - ref| <= 2 2^-24 |x - mean| istd + 2^-24 |ref| (the
    subtraction and the product each round once, then the store); everything else bit for bit.  -> (ok, worst err / allowed, text)"""
    got32 = np.asarray(got32, dtype=np.float32)
    same = got32.view(np.uint32) == ref.astype(np.float32).view(np.uint32)
    got = got32.astype(np.float64)
    allowed = 2.0 * U24 * scale + U24 * np.abs(ref)
    err = np.abs(got - ref)
    fine = np.where(exact, same, err <= allowed)
    with np.errstate(all="ignore"):
        ratio = np.where(exact | (allowed == 0), 0.0, err / allowed)
    worst = float(np.nan_to_num(ratio, nan=np.inf).max(initial=0.0))
    if fine.all():
        return True, worst, f"worst err / allowed {worst:.2f}"
    i = np.unravel_index(int(np.argmin(fine)), fine.shape)
    return False, float("inf"), f"{int((~fine).sum())} elements off, first at {i}: got {got32[i]!r} ref {ref[i]!r} ({'exact' if exact[i] else 'allowed %.3e' % allowed[i]})"


def judge_bf16(got_bits, out32):
    """the bf16 output must be the round-to-nearest-even cast of the float32 output of the same call, bit for bit"""
    want = bf16_bits(out32)
    n = int((np.asarray(got_bits).view(np.uint16) != want).sum())
    return n == 0, f"{n} bf16 elements are not the rounded float32 output"


# ====================================================================================================== mutants
# (name, where the judge rejects it).  GPU cases that would fail for each: the table in tests/test_hip_frontend_ref.py.
MUTANTS = [
    ("preemph_first_sample_zero", "hand mixed_lengths"),  # invisible under the Povey window, which is 0 at sample 0
    ("no_dc_removal", "fbank 16000/80"),
    ("window_over_n", "fbank 16000/80"),
    ("stale_sample_offset", "walk total10200_per2"),
    ("empty_not_skipped", "walk total10200_per2"),
    ("nyquist_bin_included", "fbank 16000/80"),
    ("bins_ge_64_dropped", "fbank 16000/65"),
    ("bins_ge_128_dropped", "fbank 16000/160"),
    ("filter_tail_dropped", "fbank 16000/80"),
    ("no_log_floor", "fbank 16000/80"),
    ("twiddle_sign", "fbank 8000/80"),
    ("cmvn_over_all_frames", "cmvn F 83 max_frames 8"),
    ("cmvn_pieces_overlap", "cmvn F 83 max_frames 0"),
    ("variance_not_clamped", "cmvn F 83 max_frames 0"),
    ("pad_value_behind_crop", "finalize F 83 Tmax 64 crop 57"),
    ("time_mask_in_padding", "finalize F 83 Tmax 64 crop None"),
    ("bf16_store_truncates", "finalize F 83 Tmax 64 bf16"),
    ("grid_stride_stops", "finalize big / transform 60 x 80"),
]
