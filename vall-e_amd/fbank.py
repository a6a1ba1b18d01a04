"""Log-mel filterbank features on the GPU: the reference's `valle/data/fbank.py` (`BigVGANFbank`: 24 kHz, n_fft 1024, hop 256,
100 Slaney mels, log with a 1e-5 floor) behind `vx_fbank_*` (include/vallex.h, csrc/fbank_kernels.hpp); there is no CPU
fallback.  The reference's names are kept, so `--audio-extractor Fbank` code swaps the import:

    from valle_amd.fbank import get_fbank_extractor
    feats = get_fbank_extractor().extract(samples, 24000)            # numpy (n_frames, 100) float32, as the reference returns
    mels = extractor.extract_batch([wav_a, wav_b])                   # device tensors, one ragged launch
    mels = extractor.extract_batch([stereo_48k], sr=48000)           # mixed down and resampled on the GPU first
    d = mel_distance(mels[0], mels[1])                               # mean |log-mel difference| over the common frames

Per utterance of L samples: n_frames = (L + 128) // 256, zeros appended up to (n_frames - 1) * 256 + 1024 samples (no centring,
no reflection: the branch the reference runs), periodic Hann window, one-sided DFT, sqrt(re^2 + im^2 + 1e-9), mel basis,
log(max(., 1e-5)).  Fewer than 128 samples give an empty (0, n_mels) result (the reference fails inside torch.stft there).

`slaney_mel_basis` is written from the published definition behind `librosa.filters.mel(htk=False, norm="slaney")`; librosa
and lhotse are not dependencies, so bit parity with librosa's table and with lhotse's `compute_num_frames` at its rounding
edges is not pinned: pass `mel_basis=` to use a table of your own."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import asdict, dataclass
from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import engine as _e
from ._handle import Handle, i32_array, owner_resampler, prepare_waveforms, ptr_array, shared

SAMPLE_RATE = 24000
N_FFT = 1024
HOP = 256
N_BINS = N_FFT // 2 + 1
TILE_FRAMES = 16  # frames one workgroup owns (csrc/fbank_kernels.hpp FBANK_TILE)
EPSILON = 1e-10   # lhotse.utils.EPSILON


@dataclass
class BigVGANFbankConfig:
    # the reference's fields (valle/data/fbank.py:29-41); the served geometry is the default one
    frame_length: float = 1024 / 24000.0
    frame_shift: float = 256 / 24000.0
    remove_dc_offset: bool = True
    round_to_power_of_two: bool = True
    low_freq: float = 0.0
    high_freq: float = 12000.0
    num_mel_bins: int = 100
    use_energy: bool = False

    def to_dict(self) -> Dict[str, Any]:
        return asdict(self)

    @staticmethod
    def from_dict(data: Dict[str, Any]) -> "BigVGANFbankConfig":
        return BigVGANFbankConfig(**data)


def num_frames(n_samples: int) -> int:
    """(L + 128) // 256: L / hop rounded half up, what the reference gets from `compute_num_frames`."""
    return (int(n_samples) + HOP // 2) // HOP if n_samples > 0 else 0


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, math.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (np.maximum(m, min_log_mel) - min_log_mel)), f_sp * m)


def slaney_mel_basis_f64(sr: int, n_fft: int, n_mels: int, fmin: float, fmax: float) -> np.ndarray:
    """`slaney_mel_basis` before its rounding: numpy (n_mels, n_fft // 2 + 1) float64."""
    pts = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    freqs = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    fdiff = np.diff(pts)
    ramps = pts[:, None] - freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (pts[2:] - pts[:-2]))[:, None]


def slaney_mel_basis(sr: int = SAMPLE_RATE, n_fft: int = N_FFT, n_mels: int = 100, fmin: float = 0.0,
                     fmax: Optional[float] = None) -> torch.Tensor:
    """(n_mels, n_fft // 2 + 1) float32: triangular filters between n_mels + 2 points equally spaced on Slaney's mel scale
    (linear below 1 kHz at 200 / 3 Hz per mel, logarithmic above with step log(6.4) / 27), each scaled by 2 / (its width in
    Hz).  Computed in fp64 on the host and rounded once."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    return torch.from_numpy(slaney_mel_basis_f64(sr, n_fft, n_mels, float(fmin), fmax).astype(np.float32))


def mel_distance(a: torch.Tensor, b: torch.Tensor, warp: bool = False) -> torch.Tensor:
    """Mean absolute log-mel difference over the frames both (n_frames, n_mels) tensors have; a 0-dim tensor on their device.
    With `warp` the frames are paired along the DTW path of the raw log-mels (`dtw.DTW` with n_ceps = 0: Euclidean local cost)
    instead of index by index, for two signals whose timing differs; device tensors only then."""
    assert a.dim() == 2 and b.dim() == 2 and a.shape[1] == b.shape[1], "two (n_frames, n_mels) tensors of one n_mels"
    n = min(a.shape[0], b.shape[0])
    if n == 0:
        raise ValueError("mel_distance: no common frame (an input has fewer than 128 samples)")
    if warp:
        from .dtw import shared_dtw

        path = shared_dtw(a.device, a.shape[1], 0).compare(a, b, return_path=True).path.long()
        return (a[path[:, 0]] - b[path[:, 1]]).abs().mean()
    return (a[:n] - b[:n]).abs().mean()


class BigVGANFbank(Handle):
    """The reference's extractor on the GPU.  `extract` is the reference's call (numpy out); `extract_batch` serves up to
    `max_batch` utterances of any lengths per launch and returns device tensors."""
    _PREFIX, _NAME = "vx_fbank", "BigVGANFbank"

    name = "fbank"
    config_type = BigVGANFbankConfig

    def __init__(self, config: Optional[Any] = None, mel_basis: Optional[torch.Tensor] = None, max_batch: int = 64):
        if isinstance(config, dict):
            config = BigVGANFbankConfig.from_dict(config)
        self.config = config or BigVGANFbankConfig()
        self.max_batch = int(max_batch)
        self.clip_val = 1e-5
        n = int(self.config.num_mel_bins)
        if mel_basis is None:
            mel_basis = slaney_mel_basis(SAMPLE_RATE, N_FFT, n, self.config.low_freq, self.config.high_freq)
        mel_basis = torch.as_tensor(mel_basis).detach().to("cpu", torch.float32).contiguous()
        if tuple(mel_basis.shape) != (n, N_BINS):
            raise ValueError(f"mel_basis is {tuple(mel_basis.shape)}, expected ({n}, {N_BINS})")
        self.mel_basis = mel_basis
        self._init_handle()

    def _config_struct(self) -> "_e.VxFbankConfig":
        c, g = _e.VxFbankConfig(), self.config
        c.struct_size = C.sizeof(_e.VxFbankConfig)
        c.sample_rate = SAMPLE_RATE
        c.n_fft = int(round(g.frame_length * SAMPLE_RATE))
        c.hop = int(round(g.frame_shift * SAMPLE_RATE))
        c.n_mels, c.fmin, c.fmax, c.clip, c.max_batch = int(g.num_mel_bins), g.low_freq, g.high_freq, self.clip_val, self.max_batch
        return c

    def _configure(self, lib):
        _e._check(lib.vx_fbank_set_mel_basis(self._h, self.mel_basis.data_ptr()))

    # ---- the reference's surface --------------------------------------------------------------------
    @property
    def frame_shift(self) -> float:
        return self.config.frame_shift

    def feature_dim(self, sampling_rate: int) -> int:
        return self.config.num_mel_bins

    @staticmethod
    def mix(features_a: np.ndarray, features_b: np.ndarray, energy_scaling_factor_b: float) -> np.ndarray:
        return np.log(np.maximum(EPSILON, np.exp(features_a) + energy_scaling_factor_b * np.exp(features_b)))

    @staticmethod
    def compute_energy(features: np.ndarray) -> float:
        return float(np.sum(np.exp(features)))

    def extract(self, samples: Union[np.ndarray, torch.Tensor], sampling_rate: int) -> np.ndarray:
        """samples (L,) or (1, L) at 24 kHz -> numpy (n_frames, num_mel_bins) float32."""
        assert sampling_rate == SAMPLE_RATE
        if not isinstance(samples, torch.Tensor):
            samples = torch.from_numpy(np.ascontiguousarray(samples))
        return self.extract_batch([samples.to(torch.float32)])[0].cpu().numpy()

    # ---- ours ---------------------------------------------------------------------------------------
    def resampler(self, orig_hz: int):
        """The object's `Resampler` from a rate to 24 kHz (kept per rate, `max_batch` utterances per call)."""
        return owner_resampler(self, orig_hz, SAMPLE_RATE)

    @torch.no_grad()
    def extract_batch(self, wavs: Sequence[torch.Tensor], sr: Optional[int] = None) -> List[torch.Tensor]:
        """wavs[i]: (L_i,), (1, L_i) or (1, 1, L_i) float32 mono at 24 kHz -> [(n_frames_i, num_mel_bins) float32 on the device],
        every utterance bitwise what it is alone.  With `sr` given the entries are (L_i,), (C_i, L_i) or (1, C_i, L_i) at that
        rate and go through `Resampler` (channel mean, windowed sinc) first; mono input at 24000 is taken as it is."""
        self._need_device()
        wavs = list(wavs)
        outs: List[torch.Tensor] = []
        for i in range(0, len(wavs), self.max_batch):
            outs += self._extract_chunk(wavs[i:i + self.max_batch], sr)
        return outs

    def _extract_chunk(self, wavs, sr):
        ws = prepare_waveforms(self, wavs, sr, SAMPLE_RATE, strict=False)
        n_mels = int(self.config.num_mel_bins)
        outs = [torch.empty((num_frames(w.numel()), n_mels), dtype=torch.float32, device=self.device) for w in ws]
        live = [i for i, o in enumerate(outs) if o.shape[0] > 0]  # an empty result has no storage to point at, and nothing to write
        if live:
            with torch.cuda.device(self.device):
                self._extract_raw([ws[i].data_ptr() for i in live], [ws[i].numel() for i in live], [outs[i].data_ptr() for i in live])
        return outs

    def _extract_raw(self, wav_ptrs, lengths, out_ptrs):
        """vx_fbank_extract on raw pointers (the argument checks run before any device work)."""
        self._invoke("extract", len(wav_ptrs), ptr_array(wav_ptrs), i32_array(lengths), ptr_array(out_ptrs))


_SHARED: Dict[tuple, BigVGANFbank] = {}


def shared_fbank(device) -> BigVGANFbank:
    """The process-wide default extractor of a device (what the distances on waveforms in dtw, pitch and stft use)."""
    return shared(_SHARED, device, (), BigVGANFbank, "fbank")


def get_fbank_extractor(device: Optional[Union[str, torch.device]] = None) -> BigVGANFbank:
    """The reference's factory.  The extractor is placed on `device`, by default on the current GPU where there is one (the
    reference's call then works as it is); without a GPU it stays on the host and only its host-side surface works."""
    fb = BigVGANFbank(BigVGANFbankConfig())
    if device is None and torch.cuda.is_available():
        device = "cuda"
    return fb.to(device) if device is not None else fb
