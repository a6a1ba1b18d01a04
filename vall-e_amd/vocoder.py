"""Griffin-Lim vocoder on the GPU: log-mel frames, as `BigVGANFbank` extracts them and `models.Transformer.inference` predicts
them, back to a 24 kHz waveform behind `vx_vocoder_*` (include/vallex.h, csrc/vocoder_kernels.hpp); there is no CPU fallback.

    from valle_amd import GriffinLim, mel_to_waveform
    wav = mel_to_waveform(mel)                                   # (T, 100) device tensor -> (256 T,) float32 on that device
    gl = GriffinLim().to("cuda")
    wavs = gl.synthesize_batch([mel_a, mel_b], n_iter=32)        # one ragged call
    wav, ang = gl(mel, n_iter=8, return_phase=True)              # ang (T, 513, 2): the final unit phases
    wav2 = gl(mel, n_iter=24, init_phase=ang)                    # warm start
    gl.save("out.wav", wav)

The definition (mel -> magnitude by the least-squares inverse of the mel basis, then Griffin-Lim with momentum as in
`torchaudio.functional.griffinlim`, both transforms in the filterbank's own framing) is stated in include/vallex.h.  The kernel has no
random number generator: `rand_init=True, seed=` draws the starting phases on the host with a seeded `torch.Generator`.
Griffin-Lim recovers a phase that is consistent with the magnitudes, not the original one: its audio carries the method's known
phasiness, and a mel spectrogram does not determine the magnitudes it was reduced from."""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

import torch

from . import engine as _e
from ._handle import Handle, i32_array, ptr_array, shared
from .fbank import HOP, N_BINS, SAMPLE_RATE, BigVGANFbankConfig

TILE_FRAMES = 16        # frames one workgroup owns in a large call (csrc/vocoder_kernels.hpp VOC_TILE)
TILE_FRAMES_SMALL = 4   # ... and in a call of few frames (VOC_TILE_SMALL); the bits do not depend on which
ENV_FLOOR = 0.1         # floor under the window envelope: part of the definition


def num_samples(n_frames: int) -> int:
    """256 T: the samples `n_frames` = T frames give; `fbank.num_frames` of it is T again."""
    return HOP * int(n_frames) if n_frames > 0 else 0


class GriffinLim(Handle):
    """`GriffinLim(config=None, mel_basis=None, max_batch=64, max_total_frames=131072)`: `config` is the filterbank's
    (`BigVGANFbankConfig`, or a dict of it); `mel_basis` (n_mels, 513) replaces the built-in Slaney table, `inverse` (513, n_mels)
    replaces the least-squares inverse itself.  A call serves up to `max_batch` utterances of `max_total_frames` frames in all."""
    _PREFIX, _NAME = "vx_vocoder", "GriffinLim"

    def __init__(self, config=None, mel_basis: Optional[torch.Tensor] = None, max_batch: int = 64, max_total_frames: int = 131072,
                 env_floor: float = ENV_FLOOR, inverse: Optional[torch.Tensor] = None):
        if isinstance(config, dict):
            config = BigVGANFbankConfig.from_dict(config)
        self.config = config or BigVGANFbankConfig()
        self.max_batch, self.max_total_frames, self.env_floor = int(max_batch), int(max_total_frames), float(env_floor)
        n = int(self.config.num_mel_bins)
        if mel_basis is not None:
            mel_basis = torch.as_tensor(mel_basis).detach().to("cpu", torch.float32).contiguous()
            if tuple(mel_basis.shape) != (n, N_BINS):
                raise ValueError(f"mel_basis is {tuple(mel_basis.shape)}, expected ({n}, {N_BINS})")
        if inverse is not None:
            inverse = torch.as_tensor(inverse).detach().to("cpu", torch.float32).contiguous()
            if tuple(inverse.shape) != (N_BINS, n):
                raise ValueError(f"inverse is {tuple(inverse.shape)}, expected ({N_BINS}, {n})")
        self.mel_basis, self._inverse = mel_basis, inverse
        self._init_handle()  # a geometry the kernels do not serve, or a basis without an inverse, is refused here

    def _config_struct(self) -> "_e.VxVocoderConfig":
        c, g = _e.VxVocoderConfig(), self.config
        c.struct_size = C.sizeof(_e.VxVocoderConfig)
        c.sample_rate = SAMPLE_RATE
        c.n_fft = int(round(g.frame_length * SAMPLE_RATE))
        c.hop = int(round(g.frame_shift * SAMPLE_RATE))
        c.n_mels, c.fmin, c.fmax, c.env_floor = int(g.num_mel_bins), g.low_freq, g.high_freq, self.env_floor
        c.max_batch, c.max_total_frames = self.max_batch, self.max_total_frames
        return c

    def _configure(self, lib):
        if self.mel_basis is not None:
            _e._check(lib.vx_vocoder_set_mel_basis(self._h, self.mel_basis.data_ptr()))
        if self._inverse is not None:
            _e._check(lib.vx_vocoder_set_inverse(self._h, self._inverse.data_ptr()))

    @property
    def inverse(self) -> torch.Tensor:
        """(513, n_mels) float32: the table that takes mel energies to magnitudes (`vx_vocoder_get_inverse`)."""
        out = torch.empty((N_BINS, int(self.config.num_mel_bins)), dtype=torch.float32)
        _e._check(_e.load_library().vx_vocoder_get_inverse(self._handle(), out.data_ptr()))
        return out

    # ---- synthesis ----------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, logmel: torch.Tensor, n_iter: int = 32, momentum: float = 0.99, rand_init: bool = False, seed: int = 0,
                 init_phase: Optional[torch.Tensor] = None, return_phase: bool = False):
        """logmel (T, n_mels) or (1, T, n_mels) float32 -> wav (256 T,) float32 on the device; with `return_phase` also the
        final phases (T, 513, 2).  `init_phase`: (T, 513) radians, or (T, 513, 2) as `return_phase` gives them (a warm start)."""
        res = self.synthesize_batch([logmel], n_iter=n_iter, momentum=momentum, rand_init=rand_init, seed=seed,
                                    init_phase=None if init_phase is None else [init_phase], return_phase=return_phase)
        return (res[0][0], res[1][0]) if return_phase else res[0]

    @torch.no_grad()
    def synthesize_batch(self, logmels: Sequence[torch.Tensor], n_iter: int = 32, momentum: float = 0.99, rand_init: bool = False,
                         seed: int = 0, init_phase: Optional[Sequence[torch.Tensor]] = None, return_phase: bool = False):
        """[(T_i, n_mels)] -> [(256 T_i,)] (and [(T_i, 513, 2)] with `return_phase`), every utterance bitwise what it is alone;
        more than `max_batch` utterances, or more frames than `max_total_frames`, are served in several calls.  With `rand_init`
        utterance i starts from phases drawn uniformly in [0, 2 pi) by a CPU generator seeded with `seed + i`."""
        self._need_device()
        if init_phase is not None and rand_init:
            raise ValueError("init_phase and rand_init exclude each other")
        n_mels = int(self.config.num_mel_bins)
        mels = []
        for m in logmels:
            if m.dim() == 3 and m.shape[0] == 1:
                m = m[0]
            assert m.dim() == 2 and m.shape[1] == n_mels and m.dtype == torch.float32, f"one (T, {n_mels}) float32 log-mel per entry"
            mels.append(m.detach().to(self.device).contiguous())
        inits, warm = None, False
        if rand_init:
            inits = []
            for i, m in enumerate(mels):
                g = torch.Generator().manual_seed(int(seed) + i)
                inits.append((torch.rand((m.shape[0], N_BINS), generator=g) * (2.0 * math.pi)).to(self.device))
        elif init_phase is not None:
            inits = [p.detach().to(self.device, torch.float32).contiguous() for p in init_phase]
            assert len(inits) == len(mels), "one init_phase per utterance"
            warm = any(p.dim() == 3 for p in inits)
            for p, m in zip(inits, mels):
                want = (m.shape[0], N_BINS, 2) if warm else (m.shape[0], N_BINS)
                assert tuple(p.shape) == want, f"init_phase is {tuple(p.shape)}, expected {want}"
        wavs = [torch.empty(num_samples(m.shape[0]), dtype=torch.float32, device=self.device) for m in mels]
        phases = [torch.empty((m.shape[0], N_BINS, 2), dtype=torch.float32, device=self.device) for m in mels] if return_phase else None
        # chunks of at most max_batch utterances and max_total_frames frames (a single longer utterance is refused by the C side)
        chunk: List[int] = []
        frames = 0
        for i, m in enumerate(mels + [None]):
            T = 0 if m is None else m.shape[0]
            if chunk and (m is None or len(chunk) == self.max_batch or frames + T > self.max_total_frames):
                with torch.cuda.device(self.device):
                    self._synthesize_raw([mels[j].data_ptr() for j in chunk], [mels[j].shape[0] for j in chunk],
                                         None if inits is None else [inits[j].data_ptr() for j in chunk], n_iter, momentum,
                                         [wavs[j].data_ptr() for j in chunk],
                                         None if phases is None else [phases[j].data_ptr() for j in chunk], warm=warm)
                chunk, frames = [], 0
            if m is not None and T > 0:  # an empty utterance has no storage to point at, and nothing to write
                chunk.append(i)
                frames += T
        return (wavs, phases) if return_phase else wavs

    def _synthesize_raw(self, mel_ptrs, n_frames, init_ptrs, n_iter, momentum, wav_ptrs, phase_ptrs, warm: bool = False):
        """vx_vocoder_synthesize (or _warm) on raw pointers (the argument checks run before any device work)."""
        self._invoke("synthesize_warm" if warm else "synthesize", len(mel_ptrs), ptr_array(mel_ptrs), i32_array(n_frames),
                     ptr_array(init_ptrs), int(n_iter), float(momentum), ptr_array(wav_ptrs), ptr_array(phase_ptrs))

    @staticmethod
    def save(path: str, wav: torch.Tensor) -> None:
        """16-bit PCM WAV at 24 kHz (`codec.save_wav`)."""
        from .codec import save_wav

        save_wav(path, wav, SAMPLE_RATE)


_SHARED = {}


def shared_griffinlim(device) -> GriffinLim:
    """The process-wide default vocoder of a device (what `mel_to_waveform` and `Transformer.inference_waveform` use)."""
    return shared(_SHARED, device, (), GriffinLim)  # any device: a host object answers the host-side surface (`inverse`)


def mel_to_waveform(logmel: torch.Tensor, **kw):
    """`GriffinLim()(logmel, **kw)` on logmel's device with the default configuration."""
    return shared_griffinlim(logmel.device)(logmel, **kw)
