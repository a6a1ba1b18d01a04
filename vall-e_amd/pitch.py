"""Fundamental-frequency tracking (YIN, de Cheveigné & Kawahara 2002) on the GPU in the filterbank's framing, and the F0 figures
of two utterances under the DTW path of their cepstra, behind `vx_pitch_*` (include/vallex.h, csrc/pitch_kernels.hpp); there is
no CPU fallback.

    tracker = PitchTracker(fmin=60, fmax=600, threshold=0.1).to("cuda")
    tr = tracker.track(wav)                        # PitchTrack(f0, aperiodicity, lag, voiced): device tensors of (L + 128) // 256 frames
    trs = tracker.track_batch([w0, w1], sr=48000)  # one ragged launch, every utterance bitwise what it is alone
    r = f0_distance(wav_a, wav_b)                  # F0Result(rmse_cents, rmse_hz, log_f0_corr, vuv_error, n_voiced, length, mcd_db)

Per frame t (samples 256 t .. 256 t + 1023 of the 24 kHz waveform, zeros past its end: row t of the log-mel): the difference
function over a 512-sample window on differences in fp32, its cumulative mean normalised form d', the first lag in
[floor(24000 / fmax), ceil(24000 / fmin)] under the threshold walked to its local minimum (else the frame is unvoiced and the
lag is d's first global minimum), parabolic refinement.  `f0` is 0 on unvoiced frames, `aperiodicity` is d' at the lag.

`f0_distance` runs the filterbank, `DTW.compare_batch(..., return_path=True)` on 13 cepstra, `track_batch` and
`vx_pitch_compare`; features, tracks and paths stay on the device.  rmse_cents and rmse_hz are over the path cells voiced in
both utterances, log_f0_corr is Pearson's r of log f0 over those cells (NaN with fewer than 2 of them or without variance),
vuv_error the share of cells voiced in exactly one.

On synthetic codec weights the numbers mean nothing, and nothing has been validated on trained audio: what is tested is that the
kernels compute this definition.  Parity with `librosa.yin` / `pyin` is not pinned either: they differ in window and framing."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import engine as _e
from ._handle import Handle, i32_array, prepare_waveforms, ptr_array, shared

SAMPLE_RATE = 24000
HOP = 256
TAU_LO, TAU_HI = 12, 512   # served lags (csrc/pitch_kernels.hpp)
MAX_BATCH = 64             # utterances per call
MAX_FRAMES = 1 << 20
TILE_FRAMES = 16           # frames one workgroup owns (PITCH_TILE)


class PitchTrack(NamedTuple):
    f0: torch.Tensor            # (T,) float32 Hz, 0 on unvoiced frames
    aperiodicity: torch.Tensor  # (T,) float32: d' at the lag
    lag: torch.Tensor           # (T,) int32: tau*
    voiced: torch.Tensor        # (T,) bool


@dataclass
class F0Result:
    rmse_cents: float     # over the path cells voiced in both; NaN without one
    rmse_hz: float
    log_f0_corr: float    # Pearson's r of ln f0 over those cells; NaN with fewer than 2 or without variance
    vuv_error: float      # cells voiced in exactly one utterance / length
    n_voiced: int         # cells voiced in both
    length: int           # cells on the path
    mcd_db: float         # the mel-cepstral distortion the same path gives (DTWResult.mcd_db)


def num_frames(n_samples: int) -> int:
    return (int(n_samples) + HOP // 2) // HOP


def result_from_sums(s: Sequence[float], mcd_db: float = float("nan")) -> F0Result:
    """One row of vx_pitch_compare's sums -> the figures."""
    n_path, n_vv, n_mis, sc, sc2, shz2, sla, slb, sla2, slb2, slab = (float(v) for v in s)
    nan = float("nan")
    rc = math.sqrt(sc2 / n_vv) if n_vv > 0 else nan
    rh = math.sqrt(shz2 / n_vv) if n_vv > 0 else nan
    corr = nan
    if n_vv >= 2:
        va, vb, cov = n_vv * sla2 - sla * sla, n_vv * slb2 - slb * slb, n_vv * slab - sla * slb
        # the variances are differences of two sums: below their rounding they are zero
        if va > 1e-12 * n_vv * sla2 and vb > 1e-12 * n_vv * slb2:
            corr = max(-1.0, min(1.0, cov / math.sqrt(va * vb)))
    return F0Result(rc, rh, corr, n_mis / n_path, int(n_vv), int(n_path), mcd_db)


class PitchTracker(Handle):
    """`track_batch` serves any number of utterances, `max_batch` per call."""
    _PREFIX, _NAME = "vx_pitch", "PitchTracker"

    def __init__(self, fmin: float = 60.0, fmax: float = 600.0, threshold: float = 0.1, max_frames: int = MAX_FRAMES,
                 max_batch: int = MAX_BATCH):
        self.fmin, self.fmax, self.threshold = float(fmin), float(fmax), float(threshold)
        self.max_frames, self.max_batch = int(max_frames), int(max_batch)
        self._init_handle()  # a band the kernel does not serve is refused here
        lo, hi = C.c_int32(), C.c_int32()
        _e._check(self._fn("lag_range")(self._h, C.byref(lo), C.byref(hi)))
        self.tau_min, self.tau_max = lo.value, hi.value

    def _config_struct(self) -> "_e.VxPitchConfig":
        c = _e.VxPitchConfig()
        c.struct_size = C.sizeof(_e.VxPitchConfig)
        c.sample_rate = SAMPLE_RATE
        c.fmin_hz, c.fmax_hz, c.threshold = self.fmin, self.fmax, self.threshold
        c.max_frames, c.max_batch = self.max_frames, self.max_batch
        return c

    def _mono_24k(self, wavs: List[torch.Tensor], sr: Optional[int]) -> List[torch.Tensor]:
        """As `BigVGANFbank.extract_batch` takes its input: with `sr`, (L,), (C, L) or (1, C, L) at that rate through `Resampler`."""
        return prepare_waveforms(self, wavs, sr, SAMPLE_RATE, strict=True, what="utterance")

    @torch.no_grad()
    def track_batch(self, wavs: Sequence[torch.Tensor], sr: Optional[int] = None) -> List[PitchTrack]:
        """wavs[i]: (L_i,), (1, L_i) or (1, 1, L_i) float32 mono at 24 kHz on the object's device -> one PitchTrack each, bitwise
        what the utterance gives alone.  With `sr` given the entries go through `Resampler` first, as in `extract_batch`."""
        self._need_device("track_batch")
        ws = self._mono_24k(list(wavs), sr)
        out: List[PitchTrack] = []
        for i in range(0, len(ws), self.max_batch):
            out += self._track_chunk(ws[i:i + self.max_batch])
        return out

    def track(self, wav: torch.Tensor, sr: Optional[int] = None) -> PitchTrack:
        return self.track_batch([wav], sr)[0]

    def _track_chunk(self, ws):
        T = [num_frames(w.numel()) for w in ws]
        f0 = [torch.zeros(t, dtype=torch.float32, device=self.device) for t in T]
        ap = [torch.zeros(t, dtype=torch.float32, device=self.device) for t in T]
        lag = [torch.zeros(t, dtype=torch.int32, device=self.device) for t in T]
        vo = [torch.zeros(t, dtype=torch.uint8, device=self.device) for t in T]
        live = [i for i, t in enumerate(T) if t > 0]  # an empty track has no storage to point at, and nothing to write
        if live:
            with torch.cuda.device(self.device):
                self._track_raw([ws[i].data_ptr() for i in live], [ws[i].numel() for i in live], [f0[i].data_ptr() for i in live],
                                [ap[i].data_ptr() for i in live], [lag[i].data_ptr() for i in live], [vo[i].data_ptr() for i in live])
        return [PitchTrack(f0[i], ap[i], lag[i], vo[i].bool()) for i in range(len(ws))]

    def _track_raw(self, wav_ptrs, lengths, f0_ptrs=None, ap_ptrs=None, lag_ptrs=None, voiced_ptrs=None):
        """vx_pitch_track on raw pointers (the argument checks run before any device work)."""
        self._invoke("track", len(lengths), ptr_array(wav_ptrs), i32_array(lengths), ptr_array(f0_ptrs), ptr_array(ap_ptrs),
                     ptr_array(lag_ptrs), ptr_array(voiced_ptrs))

    @torch.no_grad()
    def compare_sums(self, pairs: Sequence[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]) -> torch.Tensor:
        """pairs[i] = (f0_a (Ta,), f0_b (Tb,) float32, path (length, 2) int32) on the object's device -> (n, 11) float64 on the
        host: the sums of vx_pitch_compare (include/vallex.h lists them).  A path cell outside the tracks is clamped into them."""
        self._need_device("compare_sums")
        keep = []
        for i, (fa, fb, path) in enumerate(pairs):
            assert fa.dtype == torch.float32 and fb.dtype == torch.float32 and fa.dim() == 1 and fb.dim() == 1, f"pair {i}: two (frames,) float32 tracks"
            assert path.dtype == torch.int32 and path.dim() == 2 and path.shape[1] == 2, f"pair {i}: a (length, 2) int32 path"
            if any(t.device != self.device for t in (fa, fb, path)):
                raise RuntimeError(f"valle_amd.PitchTracker: pair {i} is not on {self.device} (no CPU fallback)")
            keep.append((fa.detach().contiguous(), fb.detach().contiguous(), path.detach().contiguous()))
        rows = []
        for i in range(0, len(keep), self.max_batch):
            ch = keep[i:i + self.max_batch]
            sums = torch.empty((len(ch), _e.PITCH_NSUMS), dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                self._compare_raw([a.data_ptr() for a, _, _ in ch], [a.numel() for a, _, _ in ch], [b.data_ptr() for _, b, _ in ch],
                                  [b.numel() for _, b, _ in ch], [p.data_ptr() for _, _, p in ch], [p.shape[0] for _, _, p in ch],
                                  sums.data_ptr())
            rows.append(sums.cpu())  # waits for the call on the current stream
        return torch.cat(rows) if rows else torch.empty((0, _e.PITCH_NSUMS), dtype=torch.float64)

    def _compare_raw(self, a_ptrs, Ta, b_ptrs, Tb, path_ptrs, path_len, sums_ptr):
        """vx_pitch_compare on raw pointers (the argument checks run before any device work)."""
        self._invoke("compare", len(Ta), ptr_array(a_ptrs), i32_array(Ta), ptr_array(b_ptrs), i32_array(Tb), ptr_array(path_ptrs),
                     i32_array(path_len), sums_ptr)


_SHARED: Dict[Tuple[torch.device, float, float, float], PitchTracker] = {}

Wave = Union[torch.Tensor, Sequence[torch.Tensor]]


def shared_tracker(device, fmin: float = 60.0, fmax: float = 600.0, threshold: float = 0.1) -> PitchTracker:
    """The module's own tracker for a device and band (kept: its handle is reused by later calls)."""
    return shared(_SHARED, device, (float(fmin), float(fmax), float(threshold)), lambda: PitchTracker(fmin, fmax, threshold), "pitch")


@torch.no_grad()
def f0_distance(wav_a: Wave, wav_b: Wave, sr: Optional[int] = None, n_ceps: int = 13, fmin: float = 60.0, fmax: float = 600.0,
                threshold: float = 0.1) -> Union[F0Result, List[F0Result]]:
    """F0 RMSE, voicing error and MCD of two utterances under one warp: log-mels (`BigVGANFbank.extract_batch`) -> the DTW path of
    their `n_ceps` cepstra -> the two pitch tracks gathered along it.  One pair of tensors gives one F0Result, two lists of equal
    length a list.  With `sr` given the waveforms are mixed down and resampled to 24 kHz first, once for both the filterbank and
    the tracker.  A waveform too short for a frame (fewer than 128 samples at 24 kHz): ValueError.  See the module's docstring
    for what the figures do not tell."""
    from . import dtw as _dtw
    from .fbank import shared_fbank

    single = isinstance(wav_a, torch.Tensor)
    wa, wb = ([wav_a], [wav_b]) if single else (list(wav_a), list(wav_b))
    if len(wa) != len(wb) or not wa:
        raise ValueError("f0_distance: two lists of one length >= 1, or two tensors")
    device = wa[0].device
    if device.type != "cuda" or any(w.device != device for w in wa + wb):
        raise RuntimeError("valle_amd.f0_distance runs only on an MI355X: pass device tensors of one device (no CPU fallback)")
    tracker = shared_tracker(device, fmin, fmax, threshold)
    ws = tracker._mono_24k([w for p in zip(wa, wb) for w in p], sr)
    if any(num_frames(w.numel()) == 0 for w in ws):
        raise ValueError("f0_distance: a waveform has no frame (fewer than 128 samples at 24 kHz)")
    mels = shared_fbank(device).extract_batch(ws)
    warps = _dtw.shared_dtw(device, mels[0].shape[1], n_ceps).compare_batch(list(zip(mels[0::2], mels[1::2])), return_path=True)
    tracks = tracker.track_batch(ws)
    sums = tracker.compare_sums([(tracks[2 * i].f0, tracks[2 * i + 1].f0, w.path) for i, w in enumerate(warps)])
    res = [result_from_sums(sums[i].tolist(), w.mcd_db if w.mcd_db is not None else float("nan")) for i, w in enumerate(warps)]
    return res[0] if single else res
