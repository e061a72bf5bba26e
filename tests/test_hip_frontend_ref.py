"""The audio front-end kernels (joeys2t_amd/csrc/fbank.hip: fbank512_kernel, fbank_kernel, both CMVN routes, feature_finalize(_crop),
feature_transform) against the plain fp64 references of tests/frontend_reference.py.

Every output lives between sentinels in a buffer of the test's own and untouched() is asserted after every launch; what a kernel
must not read is NaN: the gaps between the utterances of a waveform buffer, the samples behind an utterance's last full window, the
frames behind max_frames, the rows of a truncated utterance at t >= Tmax, the rows around a batch.  The rules (frontend_reference):
    filterbank   |got - ref| <= K 2^-24 cond + 2 ulp32(|ref|), cond = |frame|_2 sum_k w 2 |X_k| / E, K = 8 = 4 x the K <= 2 that the
                 project's float32 oracle needs against the same reference (re-measured by tests/test_frontend_reference_cpu.py);
                 log(eps32) within 4 ulp32 for an empty filter or a silent frame
    CMVN         mean 1 ulp32; istd 4 2^-24 (E[x^2] + mean^2) / var + 2^-22 relative; fill 2^-22; both routes within 1 ulp32
    writer       2 2^-24 |x - mean| istd + 2^-24 |ref|; masked / padded / cropped / copied elements bit for bit; the bf16 output
                 bit-equal to the rounded float32 output of the same call

Measured on MI355X: the largest err / allowed per kernel and case group (the rules allow 1), and for the filterbank the largest
K = max (err - 2 ulp32) / (2^-24 cond) a case needed, next to the 8 it is held to.  K_oracle, the same figure for the float32 oracle on
the CPU, is 0.75 over the per-geometry batches and 1.58 over 2000 frames of a long launch (asserted <= 2).
    kernel / case group                                  err / allowed    K needed   K held to
    fbank512_kernel  nine geometries                     0.23             1.33       8
    fbank512_kernel  run walk (8192 .. 20000 frames)     0.65             5.15       8     (4.84, 4.84, 4.23, 5.15)
    fbank512_kernel  hand-made tables                    0.20             0.49       8
    fbank_kernel     seven geometries                    0.28             1.56       8
    both             total_frames > frame_off[U]         0.28             1.15       8
    cmvn_stats / cmvn_stats_ws (the same figures)        mean 0.50   istd 0.23   constant columns 0.04   fill 0.17
    feature_finalize_crop  small cases, f32              0.63             (bf16: bit-equal to the rounded f32 output)
    feature_finalize_crop  second trip, f32              0.65
    feature_transform                                    0.64
The run walk needs more K than the small batches because it has 10^6 elements to find its worst in, not because of the walk: every
launch is bit-equal to the per = 1 launches of the same utterances.  With __logf in the kernels, as they were, the run walk needed
K = 7.86, 7.86, 8.50: v_log_f32 is good to one ulp of log2 E, which for E in 2^32 .. 2^46 is two ulps of ln E, and on a well-conditioned
element (cond about 1) nothing but the 2 ulp32 term is there to take it.  logf is the same instruction with a better multiply and gave
the same bits; the kernels now take the log of the mantissa and add the exponent in two parts (mel_log in fbank.hip).

Which GPU case fails if a slip of frontend_reference.MUTANTS were put into a kernel (the CPU self-check shows the rule rejects it):
    preemph_first_sample_zero   test_fbank_hand_tables (Hamming window; under the Povey window, 0 at sample 0, the slip is invisible)
    no_dc_removal, window_over_n, nyquist_bin_included, no_log_floor (silent utterance, empty filters)
                                every test_fbank_geometry case
    twiddle_sign                every test_fbank_geometry case; a slip in fbank_kernel's table walk at the seven generic ones
    bins_ge_64_dropped          (16000, 65) (16000, 80) (16000, 128) (16000, 160): the sentinel stays in the payload
    bins_ge_128_dropped         (16000, 160)
    filter_tail_dropped         every 512-point geometry; lengths 1, 3, 5 and 201 in test_fbank_hand_tables
    stale_sample_offset         test_fbank_run_walk total10200_per2 (frame 2501, 5501), total20000_per3 (frame 7001)
    empty_not_skipped           test_fbank_run_walk total10200_per2 (frame 5501 reads the NaN of an utterance without frames)
    cmvn_over_all_frames        test_cmvn max_frames in {5, 8, 40}: the frames behind the cut are NaN
    cmvn_pieces_overlap         test_cmvn, the _ws route, every utterance of 9 frames or more
    variance_not_clamped        test_cmvn: the constant column, the utterances of 0 and 1 frames
    pad_value_behind_crop       test_finalize_crop Tmax 64, crop 57 and 60
    time_mask_in_padding        test_finalize_crop Tmax 64: the masks (T - 3, 10) of the utterances of 1 and 57 frames
    bf16_store_truncates        every bf16 launch of test_finalize_crop
    grid_stride_stops           test_finalize_second_trip (element 2,097,152 on), test_feature_transform (element 4096 of 60 x 80 on)
"""
import numpy as np
import pytest
import torch

import frontend_reference as R
from attn_reference import sentinel_bf16, sentinel_f32, untouched

pytestmark = pytest.mark.gpu
G = 3      # guard rows around a filterbank output
LEAD = 64  # guard elements around every other output
MEASURED = {}


def _note(group, **figures):
    """largest figure per case group, printed as the test goes: the table above is made from these lines"""
    m = MEASURED.setdefault(group, {})
    for k, v in figures.items():
        m[k] = max(m.get(k, 0.0), float(v))
    print(f"[measured] {group}: " + ", ".join(f"{k} {v:.3f}" for k, v in m.items()))


def _abi():
    from joeys2t_amd import ops
    from joeys2t_amd._lib import Js2tError, check, lib
    return lib(), check, ops._p, ops._stream, Js2tError


def _dev_tables(tab, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in tab.items()}


def _extractor_tables(dev, sr, n_mel):
    """the tables the extractor has uploaded, read back; they are what the reference filters with"""
    from joeys2t_amd.helpers_for_audio import get_extractor
    ex = get_extractor(dev, sr, n_mel)
    names = ("window", "tw_re", "tw_im", "mel_start", "mel_len", "mel_woff", "mel_w")
    tab = {k: getattr(ex, k).cpu().numpy() for k in names}
    return ex, tab, {k: getattr(ex, k) for k in names}


def _fbank(dev, wave, soff, foff, dtab, win_len, shift, n_fft, cap=None):
    """js2t_fbank through the ABI -> float32 [total, n_mel]; `cap`: the total_frames the launch is sized for"""
    L, check, p, stream, _ = _abi()
    M, U, total = dtab["mel_start"].numel(), len(soff), int(foff[-1])
    cap = total if cap is None else cap
    out = sentinel_f32((cap + 2 * G) * M, dev)
    d_soff = torch.tensor([int(s) for s in soff], dtype=torch.int64, device=dev)
    d_foff = torch.tensor([int(f) for f in foff], dtype=torch.int64, device=dev)
    check(L.js2t_fbank(p(wave), p(d_soff), p(d_foff), U, cap, p(dtab["window"]), p(dtab["tw_re"]), p(dtab["tw_im"]), p(dtab["mel_start"]),
                       p(dtab["mel_len"]), p(dtab["mel_woff"]), p(dtab["mel_w"]), p(out[G * M:]), win_len, shift, n_fft, M, 2.0**15, 0.97,
                       R.EPS32, stream()), "js2t_fbank")
    torch.cuda.synchronize()
    assert untouched(out, [slice(G * M, (G + total) * M)]), "js2t_fbank wrote outside its rows"
    return out[G * M:(G + total) * M].view(total, M).cpu().numpy()


def _fbank_batch(dev, b, dtab, cap=None):
    wave = torch.from_numpy(b.buf).to(dev)
    return wave, _fbank(dev, wave, b.sample_off, b.frame_off, dtab, b.win_len, b.shift, b.n_fft, cap)


def _judge_fbank(group, got, b, label):
    val, cond = b.reference()
    ok, ratio, need, text = R.judge_fbank(got, val, cond, b.floor())
    print(f"{label}: err / allowed {ratio:.3f}, K needed {need:.2f} (held to {R.K_KERNEL:g})")
    assert ok, f"{label}: {text}"
    _note(group, ratio=ratio, K=need)


# ================================================================================================================ filterbank
@pytest.mark.parametrize("sr,n_mel", R.FBANK_GEOS, ids=[f"{sr}-{m}" for sr, m in R.FBANK_GEOS])
def test_fbank_geometry(device, sr, n_mel):
    """one ragged batch per geometry (0, 1, 1, 2, 6 frames, a silent utterance of 3, 300 samples) in one NaN-gapped buffer"""
    from joeys2t_amd.helpers_for_audio import fbank_tables
    ex, tab, dtab = _extractor_tables(device, sr, n_mel)
    recipe = fbank_tables(sr, n_mel)
    assert all(np.array_equal(tab[k], recipe[k]) for k in tab)  # the cached reference was filtered with these very numbers
    b = R.geo_batch(sr, n_mel)
    assert (ex.win_len, ex.shift, ex.n_fft) == (b.win_len, b.shift, b.n_fft) and b.total % 4
    wave, got = _fbank_batch(device, b, dtab)
    _judge_fbank("fbank512 geometries" if b.n_fft == 512 else "fbank generic geometries", got, b, f"{sr} Hz, {n_mel} bins")
    feat, foff, frames = ex.batch(wave, b.n_samples, b.sample_off)  # the public entry: the same launch, its own bookkeeping
    assert frames == b.frames and foff.cpu().tolist() == b.frame_off.tolist()
    assert np.array_equal(feat.cpu().numpy().view(np.uint32), got.view(np.uint32))


def test_fbank_rejected_rates(device):
    """n_fft below 64 / above 1024: the extractor says so, and the launcher writes nothing"""
    from joeys2t_amd.helpers_for_audio import FbankExtractor, fbank_geometry
    L, check, p, stream, Js2tError = _abi()
    _, _, dtab = _extractor_tables(device, 16000, 80)
    wave = torch.zeros(4096, device=device)
    soff, foff = torch.zeros(1, dtype=torch.int64, device=device), torch.tensor([0, 1], dtype=torch.int64, device=device)
    for sr in R.REJECTED_RATES:
        with pytest.raises(Js2tError, match="64..1024"):
            FbankExtractor(device, sr, 80)
        w, s, n_fft = fbank_geometry(sr)
        out = sentinel_f32(2 * LEAD + 80, device)
        with pytest.raises(Js2tError, match="n_fft"):
            check(L.js2t_fbank(p(wave), p(soff), p(foff), 1, 1, p(dtab["window"]), p(dtab["tw_re"]), p(dtab["tw_im"]), p(dtab["mel_start"]),
                               p(dtab["mel_len"]), p(dtab["mel_woff"]), p(dtab["mel_w"]), p(out[LEAD:]), w, s, n_fft, 80, 2.0**15, 0.97, R.EPS32,
                               stream()), "js2t_fbank")
        torch.cuda.synchronize()
        assert untouched(out, [])


@pytest.mark.parametrize("name", list(R.WALKS))
def test_fbank_run_walk(device, name):
    """fbank512_kernel's per-wave runs of `per` consecutive frames (per > 1 from 8193 frames a launch on): the whole launch against
    fp64, and bit for bit against the same utterances extracted in launches of at most 8192 frames (per = 1)"""
    _, tab, dtab = _extractor_tables(device, 16000, 80)
    b = R.walk_batch(name)
    assert b.per() == R.WALK_PER[name] and all(np.array_equal(tab[k], b.tab[k]) for k in tab)
    wave, got = _fbank_batch(device, b, dtab)
    _judge_fbank("fbank512 run walk", got, b, name)
    for u, T in enumerate(b.frames):
        for c0 in range(0, T, 8192):
            n = min(8192, T - c0)
            one = _fbank(device, wave, [b.sample_off[u] + c0 * b.shift], [0, n], dtab, b.win_len, b.shift, b.n_fft)
            lo = int(b.frame_off[u]) + c0
            assert np.array_equal(one.view(np.uint32), got[lo:lo + n].view(np.uint32)), f"{name}: utterance {u}, frames {c0}.. differ by launch"


@pytest.mark.parametrize("sr", [16000, 8000])
def test_fbank_total_frames_beyond_the_real_total(device, sr):
    """a launch sized for more frames than frame_off[U] holds (a captured launch serving a smaller batch): the rows behind stay"""
    _, _, dtab = _extractor_tables(device, sr, 80)
    b = R.geo_batch(sr, 80)
    for extra in (1, 9):
        _, got = _fbank_batch(device, b, dtab, cap=b.total + extra)  # untouched() inside: rows total .. total + extra keep the sentinel
        _judge_fbank("fbank total_frames > total", got, b, f"{sr} Hz, cap + {extra}")


@pytest.mark.parametrize("name", list(R.HAND_TABLES))
def test_fbank_hand_tables(device, name):
    """a caller's own tables at n_fft 512: 12 x 201 = 2412 weights (more than the 2048 the kernel keeps in LDS: read from memory),
    and filters of 0, 1, 3, 4, 5 weights (empty; every remainder of the four partial sums); a window that is not 0 at sample 0"""
    b = R.hand_batch(name)
    val, cond = b.reference()
    loud = ~np.repeat(np.asarray(b.silent_utt), b.frames)
    share, worst = R.tolerance_profile(val[loud], cond[loud], b.floor()[loud])
    assert share >= 0.9 and worst <= 1e-2, (share, worst)
    _, got = _fbank_batch(device, b, _dev_tables(b.tab, device))
    _judge_fbank("fbank512 hand tables", got, b, name)


# ================================================================================================================ CMVN
def _cmvn(dev, route, feat_dev, lead, fo, F, nm, nv, mf):
    L, check, p, stream, _ = _abi()
    U = len(fo) - 1
    d_fo = torch.from_numpy(fo).to(dev)
    mean, istd, fill = sentinel_f32(U * F + 2 * LEAD, dev), sentinel_f32(U * F + 2 * LEAD, dev), sentinel_f32(U + 2 * LEAD, dev)
    x = feat_dev[lead:]
    if route == "ws":
        n = int(L.js2t_cmvn_stats_workspace(U, F))
        ws = sentinel_f32(2 * n + 4 * LEAD, dev)  # n doubles between 2 x LEAD floats
        check(L.js2t_cmvn_stats_ws(p(x), p(d_fo), U, F, p(mean[LEAD:]), p(istd[LEAD:]), p(fill[LEAD:]), nm, nv, mf, p(ws[2 * LEAD:]), stream()),
              "js2t_cmvn_stats_ws")
    else:
        check(L.js2t_cmvn_stats(p(x), p(d_fo), U, F, p(mean[LEAD:]), p(istd[LEAD:]), p(fill[LEAD:]), nm, nv, mf, stream()), "js2t_cmvn_stats")
    torch.cuda.synchronize()
    assert untouched(mean, [slice(LEAD, LEAD + U * F)]) and untouched(istd, [slice(LEAD, LEAD + U * F)]) and untouched(fill, [slice(LEAD, LEAD + U)])
    if route == "ws":
        assert untouched(ws, [slice(2 * LEAD, 2 * LEAD + 2 * n)]), "the workspace's neighbours were written"
    return dict(mean=mean[LEAD:LEAD + U * F].view(U, F).cpu().numpy(), istd=istd[LEAD:LEAD + U * F].view(U, F).cpu().numpy(),
                fill=fill[LEAD:LEAD + U].cpu().numpy())


def _cmvn_case(dev, F, lens, mf, settings, label):
    feat, fo, const = R.cmvn_features(F, lens, mf)
    feat_dev = torch.from_numpy(feat).to(dev)
    got = {}
    for nm, nv in settings:
        ref = R.cmvn_ref(feat[3:], fo, nm, nv, mf)
        for route in ("one", "ws"):
            g = got[route, nm, nv] = _cmvn(dev, route, feat_dev, 3, fo, F, nm, nv, mf)
            m32 = got[route, 1, nv]["mean"] if (route, 1, nv) in got else None  # the route's own float32 mean (settings: (1, nv) first)
            ok, ratios, bad = R.judge_cmvn(g, ref, nm, nv, const, m32=m32)
            assert ok, f"{label} max_frames {mf} norm {nm}{nv} route {route}: {bad}"
            _note("cmvn " + route, **ratios)
        a, c = got["one", nm, nv], got["ws", nm, nv]
        for k in ("mean", "istd", "fill"):
            d = np.abs(a[k].astype(np.float64) - c[k].astype(np.float64))
            assert (d <= R.ulp32(np.maximum(np.abs(a[k]), np.abs(c[k])))).all(), f"{label} max_frames {mf} norm {nm}{nv}: the routes differ in {k}"


@pytest.mark.parametrize("F", R.CMVN_F)
def test_cmvn(device, F):
    """both routes; nine utterance lengths in one call and one at a time; every max_frames and norm_means / norm_vars setting.
    12 F threads rounded up to 64 leave idle threads behind the last frame group at F in {1, 5, 83, 85}"""
    for mf in R.CMVN_MAX_FRAMES:
        _cmvn_case(device, F, R.CMVN_LENS, mf, R.CMVN_SETTINGS, f"F {F}, nine utterances")
    for T in R.CMVN_LENS:
        for mf in (0, 8):
            _cmvn_case(device, F, [T], mf, [(1, 1), (0, 1)], f"F {F}, one utterance of {T}")


@pytest.mark.parametrize("F", R.CMVN_F_REFUSED)
def test_cmvn_refuses_more_than_85_bins(device, F):
    _, _, _, _, Js2tError = _abi()
    feat, fo, _ = R.cmvn_features(F, [4, 9], 0)
    feat_dev = torch.from_numpy(feat).to(device)
    for route in ("one", "ws"):
        with pytest.raises(Js2tError, match="1..85 feature bins"):
            _cmvn(device, route, feat_dev, 3, fo, F, 1, 1, 0)  # raised by check() in front of the sentinel assertions ...
    L, check, p, stream, _ = _abi()
    out = sentinel_f32(2 * F + 2, device)                         # ... so once more with a buffer this test looks at
    d_fo = torch.from_numpy(fo).to(device)
    assert L.js2t_cmvn_stats(p(feat_dev[3:]), p(d_fo), 2, F, p(out), p(out), p(out), 1, 1, 0, stream()) != 0
    torch.cuda.synchronize()
    assert untouched(out, [])


# ================================================================================================================ batch writer
def _finalize(dev, dtype, feat_dev, lead, d_fo, d_mean, d_istd, d_fill, d_masks, U, Tmax, F, d_crop):
    from joeys2t_amd import ops
    L, check, p, stream, _ = _abi()
    n = U * Tmax * F
    out = sentinel_f32(n + 2 * LEAD, dev) if dtype == torch.float32 else sentinel_bf16(1, n + 2 * LEAD, dev).view(-1)
    check(L.js2t_feature_finalize_crop(p(feat_dev[lead:]), p(d_fo), p(d_mean), p(d_istd), p(d_fill), p(d_masks), p(out[LEAD:]), ops.dt_code(dtype), U,
                                       Tmax, F, R.PAD_VALUE, p(d_crop), stream()), "js2t_feature_finalize_crop")
    torch.cuda.synchronize()
    assert untouched(out, [slice(LEAD, LEAD + n)]), "js2t_feature_finalize_crop wrote outside its batch"
    pay = out[LEAD:LEAD + n]
    if dtype == torch.float32:
        return pay.cpu().numpy().reshape(U, Tmax, F)
    return pay.view(torch.int16).cpu().numpy().view(np.uint16).reshape(U, Tmax, F)


def _finalize_case(dev, F, lens, Tmax, crops, label, variants=((0, 0), (0, 1), (1, 0), (1, 1))):
    feat, fo, mean, istd, fill = R.writer_inputs(F, lens, Tmax)
    masks = R.finalize_masks(lens, F)
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    feat_dev, d_fo, d_mean, d_istd, d_fill, d_masks = up(feat), up(fo), up(mean), up(istd), up(fill), up(masks)
    U = len(lens)
    for crop in crops:
        cv = None if crop is None else Tmax + 5 if crop == "above" else crop
        d_crop = None if cv is None else torch.tensor([cv], dtype=torch.int64, device=dev)
        for norm, mask in variants:
            ref, scale, exact = R.finalize_ref(feat[2:], fo, mean if norm else None, istd if norm else None, fill if mask else None,
                                               masks if mask else None, Tmax, cv)
            args = (feat_dev, 2, d_fo, d_mean if norm else None, d_istd if norm else None, d_fill if mask else None, d_masks if mask else None,
                    U, Tmax, F, d_crop)
            out32 = _finalize(dev, torch.float32, *args)
            ok, ratio, text = R.judge_affine(out32, ref, scale, exact)
            assert ok, f"{label} crop {crop} norm {norm} masks {mask}: {text}"
            ok16, text16 = R.judge_bf16(_finalize(dev, torch.bfloat16, *args), out32)
            assert ok16, f"{label} crop {crop} norm {norm} masks {mask}: {text16}"
            _note("finalize " + label.split(",")[0], ratio=ratio)


@pytest.mark.parametrize("Tmax", R.FIN_TMAX)
@pytest.mark.parametrize("F", R.FIN_F)
def test_finalize_crop(device, F, Tmax):
    """utterances of 0, 1, 20, 57 frames against Tmax 13 (two are truncated: their rows behind are NaN), 57 and 64; crop_t absent, 57,
    60, above Tmax; with and without mean / istd, with and without masks; float32 and bf16"""
    _finalize_case(device, F, R.FIN_LENS, Tmax, R.FIN_CROPS, f"small, F {F} Tmax {Tmax}")


def test_finalize_second_trip(device):
    """3 x 8750 x 80 = 2,100,000 elements: 2848 more than the 8192 x 256 threads of the capped grid cover in one trip"""
    big = R.FIN_BIG
    _finalize_case(device, big["F"], big["lens"], big["Tmax"], [None], "second trip", variants=((1, 1), ))


# ================================================================================================================ transform
def _transform(dev, feat, fo, mean, istd, fill, masks, n_freq, n_time):
    L, check, p, stream, _ = _abi()
    rows, F = int(fo[-1]), feat.shape[1]
    U = len(fo) - 1
    buf = sentinel_f32((rows + 2 * G) * F, dev)
    buf[G * F:(G + rows) * F] = torch.from_numpy(feat[:rows]).to(dev).view(-1)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d = [up(a) for a in (fo, mean, istd, fill, masks)]
    check(L.js2t_feature_transform(p(buf[G * F:]), p(d[0]), U, F, p(d[1]), p(d[2]), p(d[3]), p(d[4]), n_freq, n_time, stream()), "js2t_feature_transform")
    torch.cuda.synchronize()
    assert untouched(buf, [slice(G * F, (G + rows) * F)]), "js2t_feature_transform wrote outside the utterances"
    return buf[G * F:(G + rows) * F].view(rows, F).cpu().numpy()


@pytest.mark.parametrize("U", [1, 300])
def test_feature_transform(device, U):
    """in place on the ragged rows: an utterance of 60 x 80 = 4800 elements (more than the 16 x 256 threads an utterance gets);
    normalisation only; time masks without frequency masks and the reverse; a time mask that reaches past T"""
    F = 80
    lens = [60] + [(7 * u) % 23 for u in range(1, U)]
    feat, fo, mean, istd, fill = R.writer_inputs(F, lens)
    feat = feat[2:]
    for norm, n_freq, n_time in ((1, 0, 0), (0, 0, 2), (1, 3, 0), (1, 3, 2)):
        masks = R.transform_masks(lens, F, n_freq, n_time) if n_freq + n_time else None
        ref, scale, exact = R.transform_ref(feat, fo, mean if norm else None, istd if norm else None, fill, masks, n_freq, n_time)
        got = _transform(device, feat, fo, mean if norm else None, istd if norm else None, fill if masks is not None else None, masks, n_freq, n_time)
        ok, ratio, text = R.judge_affine(got, ref, scale, exact)
        assert ok, f"U {U} norm {norm} masks {n_freq} + {n_time}: {text}"
        _note("transform", ratio=ratio)


def test_feature_transform_refuses_65536_utterances(device):
    L, check, p, stream, Js2tError = _abi()
    buf = sentinel_f32(2 * LEAD + 80, device)
    fo = torch.zeros(65537, dtype=torch.int64, device=device)
    with pytest.raises(Js2tError, match="65535"):
        check(L.js2t_feature_transform(p(buf[LEAD:]), p(fo), 65536, 80, None, None, None, None, 0, 0, stream()), "js2t_feature_transform")
    check(L.js2t_feature_transform(p(buf[LEAD:]), p(fo), 65535, 80, None, None, None, None, 0, 0, stream()), "js2t_feature_transform")
    torch.cuda.synchronize()
    assert untouched(buf, [])  # 65535 utterances without frames: the largest launch there is, and it touches nothing
