"""Dynamic time warping between two feature sequences on the GPU, and mel-cepstral distortion under it (MCD-DTW), behind
`vx_dtw_*` (include/vallex.h, csrc/dtw_kernels.hpp); there is no CPU fallback.

    dtw = DTW(dim=100, n_ceps=13).to("cuda")
    r = dtw.compare(mel_a, mel_b)                      # DTWResult(total, length, mean, mcd_db, path=None)
    rs = dtw.compare_batch([(a0, b0), (a1, b1)], return_path=True)   # one ragged call, every pair bitwise what it is alone
    r = mel_cepstral_distortion(wav_a, wav_b)          # 24 kHz mono waveforms -> log-mels -> 13 cepstra -> DTW
    d = mel_distance(mel_a, mel_b, warp=True)          # fbank.mel_distance along the DTW path of the raw log-mels

Per pair (A (Ta, dim), B (Tb, dim) float32 on the device): with n_ceps > 0 every row becomes its cepstra 1 .. n_ceps (orthonormal
DCT-II without the 0th coefficient); the local cost is the Euclidean distance of two rows, on differences; the warp minimises the
summed cost over the paths from (0, 0) to (Ta - 1, Tb - 1) with steps (1, 1), (1, 0), (0, 1), accumulated in fp64, the diagonal
step preferred on ties, then (1, 0).  `total` is that sum, `length` the number of cells on the path, `mean` their quotient and
`mcd_db` = (10 sqrt(2) / ln 10) mean, the usual scale of mel-cepstral distortion (only with n_ceps > 0).

On synthetic codec weights the number means nothing, and it has not been validated on trained audio: what is tested is that the
kernels compute this definition."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import engine as _e
from ._handle import Handle, i32_array, ptr_array, shared

MAX_DIM = 128
MAX_FRAMES = 4096   # frames per sequence (csrc/dtw_kernels.hpp DTW_MAX_FRAMES: three fp64 diagonals of a pair stay in LDS)
MAX_BATCH = 64      # pairs per call
DIAG_CHUNK = 256    # cells of a diagonal the warp kernel takes per step (DTW_WG)
MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)


@dataclass
class DTWResult:
    total: float                   # G(Ta - 1, Tb - 1): the summed local cost along the best path
    length: int                    # cells on that path, max(Ta, Tb) .. Ta + Tb - 1
    mean: float                    # total / length
    mcd_db: Optional[float]        # MCD_DB * mean; None when the rows were compared as given (n_ceps = 0)
    path: Optional[torch.Tensor]   # (length, 2) int32 on the device, (i, j) ascending; None unless asked for


class DTW(Handle):
    """`compare_batch` serves any number of pairs, `max_batch` per call; the handle's workspace follows the largest call."""
    _PREFIX, _NAME = "vx_dtw", "DTW"

    def __init__(self, dim: int = 100, n_ceps: int = 13, max_frames: int = MAX_FRAMES, max_batch: int = MAX_BATCH):
        self.dim, self.n_ceps, self.max_frames, self.max_batch = int(dim), int(n_ceps), int(max_frames), int(max_batch)
        self._init_handle()  # a geometry the kernels do not serve is refused here

    def _config_struct(self) -> "_e.VxDtwConfig":
        c = _e.VxDtwConfig()
        c.struct_size = C.sizeof(_e.VxDtwConfig)
        c.dim, c.n_ceps, c.max_frames, c.max_batch = self.dim, self.n_ceps, self.max_frames, self.max_batch
        return c

    @torch.no_grad()
    def compare_batch(self, pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]], return_path: bool = False) -> List[DTWResult]:
        """pairs[i] = (A_i (Ta_i, dim), B_i (Tb_i, dim)) float32 on the object's device -> one DTWResult per pair."""
        self._need_device()
        pairs = [(a, b) for a, b in pairs]
        for i, (a, b) in enumerate(pairs):
            for t in (a, b):
                assert isinstance(t, torch.Tensor) and t.dim() == 2 and t.dtype == torch.float32 and t.shape[1] == self.dim, \
                    f"pair {i}: two (frames, {self.dim}) float32 tensors"
                if t.device != self.device:
                    raise RuntimeError(f"valle_amd.DTW: pair {i} is on {t.device}, the object on {self.device} (no CPU fallback)")
                if t.shape[0] == 0:
                    raise ValueError(f"DTW: pair {i} has a sequence without frames")
        out: List[DTWResult] = []
        for i in range(0, len(pairs), self.max_batch):
            out += self._compare_chunk(pairs[i:i + self.max_batch], return_path)
        return out

    def compare(self, a: torch.Tensor, b: torch.Tensor, return_path: bool = False) -> DTWResult:
        return self.compare_batch([(a, b)], return_path)[0]

    def _compare_chunk(self, pairs, return_path):
        n = len(pairs)
        keep = [(a.detach().contiguous(), b.detach().contiguous()) for a, b in pairs]
        total = torch.empty(n, dtype=torch.float64, device=self.device)
        length = torch.empty(n, dtype=torch.int32, device=self.device)
        paths = [torch.empty((a.shape[0] + b.shape[0] - 1, 2), dtype=torch.int32, device=self.device) for a, b in keep] \
            if return_path else None
        with torch.cuda.device(self.device):
            self._compare_raw([a.data_ptr() for a, _ in keep], [a.shape[0] for a, _ in keep], [b.data_ptr() for _, b in keep],
                              [b.shape[0] for _, b in keep], total.data_ptr(), length.data_ptr(),
                              [p.data_ptr() for p in paths] if paths else None)
        tot, lens = total.tolist(), length.tolist()  # waits for the call on the current stream
        res = []
        for i in range(n):
            mean = tot[i] / lens[i]
            res.append(DTWResult(tot[i], lens[i], mean, MCD_DB * mean if self.n_ceps > 0 else None,
                                 paths[i][:lens[i]] if paths else None))
        return res

    def _compare_raw(self, a_ptrs, Ta, b_ptrs, Tb, total_ptr, len_ptr, path_ptrs=None):
        """vx_dtw_compare on raw pointers (the argument checks run before any device work)."""
        self._invoke("compare", len(a_ptrs), ptr_array(a_ptrs), i32_array(Ta), ptr_array(b_ptrs), i32_array(Tb), total_ptr, len_ptr,
                     ptr_array(path_ptrs))


_SHARED: Dict[Tuple[torch.device, int, int], DTW] = {}


def shared_dtw(device, dim: int, n_ceps: int) -> DTW:
    """The module's own DTW object for a device and geometry (kept: its workspace is reused by later calls)."""
    return shared(_SHARED, device, (int(dim), int(n_ceps)), lambda: DTW(dim, n_ceps), "dtw")


Wave = Union[torch.Tensor, Sequence[torch.Tensor]]


@torch.no_grad()
def mel_cepstral_distortion(wav_a: Wave, wav_b: Wave, sr: Optional[int] = None, n_ceps: int = 13) -> Union[DTWResult, List[DTWResult]]:
    """MCD-DTW between waveforms on the device: `BigVGANFbank.extract_batch` (with `sr` given: mix-down and resampling to 24 kHz
    first, as there), then `DTW(100, n_ceps).compare_batch`; the features never leave the device.  One pair of tensors gives one
    DTWResult, two lists of equal length a list.  A waveform too short for a frame (fewer than 128 samples at 24 kHz): ValueError."""
    from .fbank import shared_fbank

    single = isinstance(wav_a, torch.Tensor)
    wa, wb = ([wav_a], [wav_b]) if single else (list(wav_a), list(wav_b))
    if len(wa) != len(wb) or not wa:
        raise ValueError("mel_cepstral_distortion: two lists of one length >= 1, or two tensors")
    device = wa[0].device
    if device.type != "cuda" or any(w.device != device for w in wa + wb):
        raise RuntimeError("valle_amd.mel_cepstral_distortion runs only on an MI355X: pass device tensors of one device (no CPU fallback)")
    mels = shared_fbank(device).extract_batch([w for p in zip(wa, wb) for w in p], sr)
    if any(m.shape[0] == 0 for m in mels):
        raise ValueError("mel_cepstral_distortion: a waveform has no frame (fewer than 128 samples at 24 kHz)")
    res = shared_dtw(device, mels[0].shape[1], n_ceps).compare_batch(list(zip(mels[0::2], mels[1::2])))
    return res[0] if single else res
