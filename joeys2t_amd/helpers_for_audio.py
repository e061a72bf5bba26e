"""Audio feature extraction on the GPU with the reference's function names (joeynmt/helpers_for_audio.py).

`extract_fbank_features` (:41-68), `get_n_frames` (:93-96) and `pad_features` (:130-170) keep their signatures;
the arithmetic (Kaldi fbank = torchaudio.compliance.kaldi.fbank with default arguments, :30-37) runs in
js2t_fbank.  `FbankExtractor.batch()` is the MI355X-native entry: a whole ragged batch of waveforms resident in
HBM -> one launch, one wavefront per frame.

Kaldi defaults reproduced (from the published torchaudio/Kaldi algorithm; torchaudio itself is absent here and the
result is pinned by the reference's known-answer test, tests/test_oracle_golden.py::test_fbank_known_answer):
25 ms window / 10 ms shift, snip_edges, dither 0, remove_dc_offset, preemphasis 0.97, Povey window, FFT size =
next power of two, power spectrum, 80 triangular mel filters from 20 Hz to Nyquist, log(max(x, FLT_EPSILON)).
"""
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from joeys2t_amd import ops
from joeys2t_amd._lib import check, lib

_p, _stream = ops._p, ops._stream


def get_n_frames(wave_length: int, sample_rate: int) -> int:
    """reference :93-96 — int(1 + (int(N/sr*1000) - 25)/10)."""
    duration_ms = int(wave_length / sample_rate * 1000)
    return int(1 + (duration_ms - 25) / 10)


def _mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


MIN_FFT, MAX_FFT = 64, 1024  # transform sizes js2t_fbank takes (fbank.hip: FB_MAX_FFT complex points of LDS per frame)


def fbank_geometry(sample_rate: int, frame_length_ms: float = 25.0, frame_shift_ms: float = 10.0) -> Tuple[int, int, int]:
    """(win_len, shift, n_fft) of the Kaldi framing at a sample rate: n_fft = the window length rounded up to a power of two."""
    win_len = int(sample_rate * frame_length_ms * 0.001)
    shift = int(sample_rate * frame_shift_ms * 0.001)
    return win_len, shift, 1 << (max(win_len, 1) - 1).bit_length()


def fbank_tables(sample_rate: int = 16000, n_mel_bins: int = 80, frame_length_ms: float = 25.0, frame_shift_ms: float = 10.0,
                 low_freq: float = 20.0, high_freq: float = 0.0) -> Dict[str, np.ndarray]:
    """The tables js2t_fbank reads, as host arrays (no device needed): window f32[win_len], tw_re / tw_im f32[n_fft / 2],
    mel_start / mel_len / mel_woff int32[n_mel] and mel_w f32 (the filters' non-zero stretches, back to back in bin order)."""
    n_mel = int(n_mel_bins)
    win_len, _, n_fft = fbank_geometry(sample_rate, frame_length_ms, frame_shift_ms)
    n = np.arange(win_len, dtype=np.float64)
    window = (0.5 - 0.5 * np.cos(2.0 * np.pi * n / (win_len - 1)))**0.85  # Povey
    k = np.arange(n_fft // 2, dtype=np.float64)
    ang = 2.0 * np.pi * k / n_fft
    # triangular filters on the mel scale, evaluated at the FFT bin centres (Nyquist bin weight = 0)
    nyq = 0.5 * sample_rate
    hi = high_freq + nyq if high_freq <= 0.0 else high_freq
    mlo, mhi = _mel(low_freq), _mel(hi)
    delta = (mhi - mlo) / (n_mel + 1)
    b = np.arange(n_mel, dtype=np.float64)[:, None]
    left, center, right = mlo + b * delta, mlo + (b + 1) * delta, mlo + (b + 2) * delta
    melf = _mel((sample_rate / n_fft) * np.arange(n_fft // 2, dtype=np.float64))[None, :]
    banks = np.maximum(0.0, np.minimum((melf - left) / (center - left), (right - melf) / (right - center)))
    starts, lens, woffs, wts = [], [], [], []
    for m in range(n_mel):
        nz = np.nonzero(banks[m] > 0)[0]
        st, ln = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if nz.size else (0, 0)
        starts.append(st), lens.append(ln), woffs.append(len(wts))
        wts.extend(banks[m, st:st + ln].astype(np.float32).tolist())
    return dict(window=window.astype(np.float32), tw_re=np.cos(ang).astype(np.float32), tw_im=(-np.sin(ang)).astype(np.float32),
                mel_start=np.asarray(starts, dtype=np.int32), mel_len=np.asarray(lens, dtype=np.int32),
                mel_woff=np.asarray(woffs, dtype=np.int32), mel_w=np.asarray(wts if wts else [0.0], dtype=np.float32))


class FbankExtractor:
    """Device-resident tables (window, FFT twiddles, sparse mel filters) + launcher for js2t_fbank."""

    def __init__(self, device, sample_rate: int = 16000, n_mel_bins: int = 80, frame_length_ms: float = 25.0,
                 frame_shift_ms: float = 10.0, low_freq: float = 20.0, high_freq: float = 0.0, preemph: float = 0.97):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ops.Js2tError("FbankExtractor needs a cuda (ROCm) device: features are extracted by js2t_fbank")
        self.sample_rate, self.n_mel = int(sample_rate), int(n_mel_bins)
        self.win_len, self.shift, self.n_fft = fbank_geometry(sample_rate, frame_length_ms, frame_shift_ms)
        if not (MIN_FFT <= self.n_fft <= MAX_FFT and self.shift > 0 and self.n_mel > 0):
            raise ops.Js2tError(f"fbank: a {frame_length_ms} ms window at {sample_rate} Hz has {self.win_len} samples, a transform of "
                                f"{self.n_fft} points; js2t_fbank takes {MIN_FFT}..{MAX_FFT} points (windows of {MIN_FFT // 2 + 1}.."
                                f"{MAX_FFT} samples: {1000.0 * (MIN_FFT // 2 + 1) / frame_length_ms:.0f}.."
                                f"{1000.0 * MAX_FFT / frame_length_ms:.0f} Hz at this window length)")
        self.preemph = float(preemph)
        tables = fbank_tables(sample_rate, n_mel_bins, frame_length_ms, frame_shift_ms, low_freq, high_freq)
        for name, arr in tables.items():
            setattr(self, name, torch.from_numpy(arr).to(self.device))
        self._plans = {}

    def n_frames(self, n_samples: int) -> int:
        return 0 if n_samples < self.win_len else 1 + (n_samples - self.win_len) // self.shift

    def batch(self, wave: torch.Tensor, n_samples: Sequence[int], sample_off: Optional[Sequence[int]] = None):
        """wave: f32 device buffer holding all utterances; utterance u = wave[sample_off[u] : +n_samples[u]]
        (default: rows of a [U, Nmax] tensor).  Returns (feat f32 [sum T_u, n_mel], frame_off int64[U+1] on device,
        frames per utterance as a host list)."""
        ops._dev(wave)
        if wave.dtype != torch.float32 or not wave.is_contiguous():
            raise ops.Js2tError("fbank: waveform buffer must be contiguous float32")
        U = len(n_samples)
        if sample_off is None:
            stride = wave.shape[-1] if wave.dim() == 2 else 0
            sample_off = [u * stride for u in range(U)]
        if wave.numel() < max(o + n for o, n in zip(sample_off, n_samples)):
            raise ops.Js2tError("fbank: waveform buffer shorter than sample_off + n_samples")
        # offset tables are cached per batch geometry: repeated shapes cost no host->device traffic (and the call
        # becomes capturable in a hipGraph)
        key = (tuple(int(n) for n in n_samples), tuple(int(o) for o in sample_off))
        plan = self._plans.get(key)
        if plan is None:
            frames = [self.n_frames(int(n)) for n in n_samples]
            foff = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
            plan = (frames, torch.tensor(list(sample_off), dtype=torch.int64, device=self.device),
                    torch.tensor(foff, dtype=torch.int64, device=self.device), int(foff[-1]))
            if len(self._plans) > 64:
                self._plans.clear()
            self._plans[key] = plan
        frames, d_soff, d_foff, total = plan
        return self.batch_tables(wave, d_soff, d_foff, U, total), d_foff, frames

    def batch_tables(self, wave: torch.Tensor, d_soff: torch.Tensor, d_foff: torch.Tensor, U: int, total_cap: int) -> torch.Tensor:
        """The same with the offset tables already on the device (int64 sample_off[U], frame_off[U + 1]): nothing on the host
        depends on the utterances' lengths, so one captured launch serves every batch whose frames fit `total_cap` rows (the
        kernel reads the real total from frame_off[U]; rows beyond it are left unwritten)."""
        ops._dev(wave, d_soff, d_foff)
        total = int(total_cap)
        feat = torch.empty((total, self.n_mel), dtype=torch.float32, device=self.device)
        check(lib().js2t_fbank(_p(wave), _p(d_soff), _p(d_foff), U, total, _p(self.window), _p(self.tw_re), _p(self.tw_im),
                               _p(self.mel_start), _p(self.mel_len), _p(self.mel_woff), _p(self.mel_w), _p(feat), self.win_len, self.shift,
                               self.n_fft, self.n_mel, 2.0**15, self.preemph, float(np.finfo(np.float32).eps), _stream()), "js2t_fbank")
        return feat


_extractors: Dict[Tuple, FbankExtractor] = {}


def get_extractor(device, sample_rate: int = 16000, n_mel_bins: int = 80) -> FbankExtractor:
    key = (str(device), int(sample_rate), int(n_mel_bins))
    if key not in _extractors:
        _extractors[key] = FbankExtractor(device, sample_rate, n_mel_bins)
    return _extractors[key]


def extract_fbank_features(waveform: torch.Tensor, sample_rate: int, output_path: Optional[Path] = None, n_mel_bins: int = 80,
                           overwrite: bool = False, device="cuda") -> Optional[np.ndarray]:
    """Single-utterance API of the reference (:41-68): waveform [C, N] float in [-1,1] -> np.float32 [T, n_mel].
    As in the reference, a multi-channel input is NOT mixed down (:53-54) — the first channel is used."""
    if output_path is not None and Path(output_path).is_file() and not overwrite:
        return np.load(Path(output_path).as_posix())
    wav = waveform[0] if waveform.dim() == 2 else waveform
    ex = get_extractor(device, sample_rate, n_mel_bins)
    wav = wav.to(ex.device, torch.float32).contiguous()
    feat, _, _ = ex.batch(wav, [wav.numel()], [0])
    features = feat.cpu().numpy()
    if output_path is not None:
        np.save(Path(output_path).as_posix(), features)
    return features


def pad_features(feat_list: List[np.ndarray], embed_size: int = 80, pad_index: int = 1):
    """Host-side batch padding with float(pad_index) = 1.0 (reference :130-170) for features that are already
    NumPy arrays (pre-extracted .npy inputs).  Device-resident features are padded by js2t_feature_finalize."""
    max_len = max(int(f.shape[0]) for f in feat_list)
    features = np.full((len(feat_list), max_len, embed_size), float(pad_index), dtype=np.float32)
    lengths = []
    for i, f in enumerate(feat_list):
        length = min(int(f.shape[0]), max_len)
        assert length > 0, "empty feature!"
        features[i, :length, :] = f[:length, :]
        lengths.append(length)
    assert max(lengths) == features.shape[1] and embed_size == features.shape[2]
    return features, lengths, None
