"""Multi-resolution STFT distance (M-STFT: spectral convergence plus log-magnitude distance at several window sizes, the loss of
Parallel WaveGAN and the first column of BigVGAN's objective table) between two waveforms on the GPU, and the STFT magnitudes
themselves, behind `vx_stft_*` (include/vallex.h states the definition, csrc/stft_kernels.hpp the kernel); there is no CPU
fallback.

    m = MultiResolutionSTFT().to("cuda")              # (1024, 120, 600), (2048, 240, 1200), (512, 50, 240)
    r = m.compare(pred, target)                       # MSTFTResult(sc (R,), log_mag (R,), total, frames (R,))
    rs = m.compare_batch(preds, targets)              # one ragged call, every pair bitwise what it is alone
    mag = m.magnitude(wav, 0)                         # (1 + L // hop, n_fft / 2 + 1) float32 on the device
    d = mstft_distance(pred, target, sr=16000)        # the total; resampled to 24 kHz first
    d = copy_synthesis_distance(wav, vocoder)         # wav -> log-mel -> vocoder -> waveform, against wav

Both signals are cut to the common length L; L must exceed max n_fft / 2 (1025 samples for the default triple: the reflect
padding's rule), else ValueError: a resolution is never dropped silently.  sc_r = ||Y - X||_F / ||Y||_F is not symmetric in
(pred, target); lm_r = mean |ln Y - ln X| is.  total = mean over r of sc_r + lm_r.

On synthetic weights the number means nothing, and nothing here has been validated on trained audio: what is tested is that the
kernels compute this definition.  Parity with the `auraloss` package is not pinned: the definition is written from its paper."""
from __future__ import annotations

import ctypes as C
from dataclasses import asdict, dataclass
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import engine as _e
from ._handle import Handle, i32_array, prepare_waveforms, ptr_array, shared, to_native_rate

SAMPLE_RATE = 24000
RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))  # (n_fft, hop, win)
MAX_RES = 4
MAX_BATCH = 64                    # pairs per call
MAX_SAMPLES = 1 << 22
TILE_FRAMES = 16                  # frames a workgroup owns in compare (csrc/stft_kernels.hpp STFT_ROWS_CMP)
TILE_FRAMES_MAGNITUDE = 32        # ... and in magnitude


@dataclass
class STFTConfig:
    resolutions: Tuple[Tuple[int, int, int], ...] = RESOLUTIONS
    eps: float = 1e-8             # clamp on the power: a floor of 1e-4 on the magnitude
    sample_rate: int = SAMPLE_RATE
    max_samples: int = MAX_SAMPLES

    def __post_init__(self):
        self.resolutions = tuple(tuple(int(v) for v in r) for r in self.resolutions)

    def to_dict(self) -> Dict[str, Any]:
        d = asdict(self)
        d["resolutions"] = [list(r) for r in self.resolutions]
        return d

    @staticmethod
    def from_dict(data: Dict[str, Any]) -> "STFTConfig":
        return STFTConfig(**data)

    @property
    def min_samples(self) -> int:
        """The shortest common length served: max n_fft / 2 + 1."""
        return max(r[0] for r in self.resolutions) // 2 + 1


class MSTFTResult(NamedTuple):
    sc: torch.Tensor        # (R,) float64: spectral convergence per resolution
    log_mag: torch.Tensor   # (R,) float64: mean |ln Y - ln X| per resolution
    total: float            # mean over the resolutions of sc + log_mag
    frames: torch.Tensor    # (R,) int64: 1 + L // hop


def result_from_sums(s: torch.Tensor, n_bins: Sequence[int]) -> MSTFTResult:
    """(R, 4) float64 rows of vx_stft_compare -> the figures."""
    s = s.to(torch.float64)
    sc = torch.sqrt(s[:, 0] / s[:, 1])
    lm = s[:, 2] / s[:, 3]
    frames = torch.tensor([int(round(float(s[r, 3]))) // int(n_bins[r]) for r in range(s.shape[0])], dtype=torch.int64)
    return MSTFTResult(sc, lm, float((sc + lm).mean()), frames)


class MultiResolutionSTFT(Handle):
    """`compare_batch` serves any number of pairs, `max_batch` per call."""
    _PREFIX, _NAME = "vx_stft", "MultiResolutionSTFT"

    def __init__(self, config: Optional[STFTConfig] = None, max_batch: int = MAX_BATCH):
        self.config = config if config is not None else STFTConfig()
        self.max_batch = int(max_batch)
        self._init_handle()  # a geometry the kernel does not serve is refused here

    @property
    def n_res(self) -> int:
        return len(self.config.resolutions)

    @property
    def n_bins(self) -> List[int]:
        return [r[0] // 2 + 1 for r in self.config.resolutions]

    def _config_struct(self) -> "_e.VxStftConfig":
        c = _e.VxStftConfig()
        c.struct_size = C.sizeof(_e.VxStftConfig)
        c.sample_rate = int(self.config.sample_rate)
        res = self.config.resolutions
        c.n_res = len(res)
        for i, r in enumerate(res[:MAX_RES]):
            c.n_fft[i], c.hop[i], c.win[i] = r
        c.eps = float(self.config.eps)
        c.max_samples, c.max_batch = int(self.config.max_samples), self.max_batch
        return c

    def frames(self, n_samples: int, res: int) -> int:
        return 1 + int(n_samples) // self.config.resolutions[res][1]

    def _mono(self, wavs: Sequence[torch.Tensor], what: str) -> List[torch.Tensor]:
        return prepare_waveforms(self, wavs, None, SAMPLE_RATE, strict=True, what=what)

    # ---- the distance ---------------------------------------------------------------------------------
    @torch.no_grad()
    def compare_sums(self, preds: Sequence[torch.Tensor], targets: Sequence[torch.Tensor]) -> torch.Tensor:
        """-> (n, R, 4) float64 on the host: the sums of vx_stft_compare (include/vallex.h lists them)."""
        if len(preds) != len(targets) or not len(preds):
            raise ValueError("MultiResolutionSTFT: two lists of one length >= 1")
        need = self.config.min_samples
        for i, (x, y) in enumerate(zip(preds, targets)):  # before the device is asked for, and before the library is called
            if min(x.shape[-1], y.shape[-1]) < need:
                raise ValueError(f"MultiResolutionSTFT: pair {i}: common length {min(x.shape[-1], y.shape[-1])} < {need} samples "
                                 f"(reflect padding of n_fft {2 * (need - 1)})")
        self._need_device("compare_sums")
        xs, ys = self._mono(preds, "pred"), self._mono(targets, "target")
        rows = []
        for i in range(0, len(xs), self.max_batch):
            cx, cy = xs[i:i + self.max_batch], ys[i:i + self.max_batch]
            sums = torch.empty((len(cx), self.n_res, _e.STFT_NSUMS), dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                self._compare_raw([x.data_ptr() for x in cx], [x.numel() for x in cx], [y.data_ptr() for y in cy], [y.numel() for y in cy],
                                  sums.data_ptr())
            rows.append(sums.cpu())  # waits for the call on the current stream
        return torch.cat(rows)

    def _compare_raw(self, x_ptrs, nx, y_ptrs, ny, sums_ptr):
        """vx_stft_compare on raw pointers (the argument checks run before any device work)."""
        self._invoke("compare", len(nx), ptr_array(x_ptrs), i32_array(nx), ptr_array(y_ptrs), i32_array(ny), sums_ptr)

    def compare_batch(self, preds: Sequence[torch.Tensor], targets: Sequence[torch.Tensor]) -> List[MSTFTResult]:
        """preds[i], targets[i]: (L,), (1, L) or (1, 1, L) float32 mono at 24 kHz on the object's device, of any two lengths."""
        sums = self.compare_sums(preds, targets)
        return [result_from_sums(sums[i], self.n_bins) for i in range(sums.shape[0])]

    def compare(self, pred: torch.Tensor, target: torch.Tensor) -> MSTFTResult:
        return self.compare_batch([pred], [target])[0]

    # ---- the magnitudes -------------------------------------------------------------------------------
    @torch.no_grad()
    def magnitude_batch(self, wavs: Sequence[torch.Tensor], res: int = 0) -> List[torch.Tensor]:
        """[(L_i,)] -> [(1 + L_i // hop, n_fft / 2 + 1) float32] of resolution `res`."""
        if not 0 <= int(res) < self.n_res:
            raise ValueError(f"MultiResolutionSTFT.magnitude: resolution {res} of {self.n_res}")
        n_fft = self.config.resolutions[res][0]
        for i, w in enumerate(wavs):
            if w.shape[-1] <= n_fft // 2:
                raise ValueError(f"MultiResolutionSTFT.magnitude: signal {i}: {w.shape[-1]} samples <= n_fft / 2 = {n_fft // 2}")
        self._need_device("magnitude")
        ws = self._mono(wavs, "signal")
        outs = [torch.empty((self.frames(w.numel(), res), n_fft // 2 + 1), dtype=torch.float32, device=self.device) for w in ws]
        for i in range(0, len(ws), self.max_batch):
            cw, co = ws[i:i + self.max_batch], outs[i:i + self.max_batch]
            with torch.cuda.device(self.device):
                self._magnitude_raw(res, [w.data_ptr() for w in cw], [w.numel() for w in cw], [o.data_ptr() for o in co])
        return outs

    def magnitude(self, wav: torch.Tensor, res: int = 0) -> torch.Tensor:
        return self.magnitude_batch([wav], res)[0]

    def _magnitude_raw(self, res, w_ptrs, lengths, o_ptrs):
        """vx_stft_magnitude on raw pointers (the argument checks run before any device work)."""
        self._invoke("magnitude", int(res), len(lengths), ptr_array(w_ptrs), i32_array(lengths), ptr_array(o_ptrs))


_SHARED: Dict[tuple, MultiResolutionSTFT] = {}


def shared_mstft(device) -> MultiResolutionSTFT:
    """The module's own object of the default configuration for a device (kept: its handle is reused by later calls)."""
    return shared(_SHARED, device, (), MultiResolutionSTFT, "stft")


@torch.no_grad()
def mstft_distance(pred: torch.Tensor, target: torch.Tensor, sr: Optional[int] = None) -> float:
    """The M-STFT total of two waveforms on one device at the default resolutions.  With `sr` given both are mixed down and
    resampled to 24 kHz first (`Resampler`).  A common length below 1025 samples at 24 kHz: ValueError."""
    device = pred.device
    if sr is None and min(pred.shape[-1], target.shape[-1]) < 1025:
        raise ValueError(f"mstft_distance: common length {min(pred.shape[-1], target.shape[-1])} < 1025 samples")
    if device.type != "cuda" or target.device != device:
        raise RuntimeError("valle_amd.mstft_distance runs only on an MI355X: pass device tensors of one device (no CPU fallback)")
    m = shared_mstft(device)
    x, y = to_native_rate(m, [pred, target], sr, SAMPLE_RATE)
    return m.compare(x, y).total


@torch.no_grad()
def copy_synthesis_distance(wav: torch.Tensor, vocoder, fbank=None) -> MSTFTResult:
    """Copy-synthesis: the log-mel of `wav` (mono float32 at 24 kHz on the device; `fbank`, default a `BigVGANFbank` of the
    module's own) through `vocoder` (a `GriffinLim` or a `GanVocoder`: anything that maps (T, n_mels) to a waveform), then M-STFT of
    the result (pred) against `wav` (target).  The vocoder returns 256 T samples: the comparison is over the common length."""
    device = wav.device
    if device.type != "cuda":
        raise RuntimeError("valle_amd.copy_synthesis_distance runs only on an MI355X: pass a device tensor (no CPU fallback)")
    if fbank is None:
        from .fbank import shared_fbank

        fbank = shared_fbank(device)
    mel = fbank.extract_batch([wav])[0]
    rec = vocoder(mel)
    return shared_mstft(device).compare(rec.reshape(-1), wav.reshape(-1))
