"""Host-side mirror of the reference's mel-spectrogram Transformer TTS model (``--model-name Transformer``,
valle/models/transformer.py): constructor, ``inference`` and state_dict surface of the reference class, arithmetic in
libvallex.so (the vx_mel_* entries).  The model has no vocabulary: ``inference`` returns (1, T, 100) log-mel frames, which is what
``BigVGANFbank`` extracts from a recording, so ``mel_distance`` and ``mel_cepstral_distortion`` score it directly."""
from __future__ import annotations

from collections import OrderedDict, namedtuple
from typing import Optional

import torch

from .config import NUM_TEXT_TOKENS, MelConfig
from .weights import NUM_MEL_BINS, mel_expected_keys, mel_synthetic_state_dict

_IncompatibleKeys = namedtuple("IncompatibleKeys", ["missing_keys", "unexpected_keys"])


class Transformer:
    """``Transformer(d_model, nhead, num_layers, norm_first=True, add_prenet=False, scaling_xformers=False)`` as in the reference
    (transformer.py:47-55).  Engine keyword arguments: ``precision`` ("bf16" | "fp32"), ``max_text``, ``max_frames`` (capacities;
    a text of S ids yields at most 10 S frames), ``no_graph``, ``device`` (same as ``.to(device)``), ``print_eos``.
    ``scaling_xformers=True`` (ScaledLinear, BasicNorm, DoubleSwish; transformer.py:114-172) is not built and is refused."""

    MODEL_NAME = "Transformer"

    def __init__(self, d_model: int, nhead: int, num_layers: int, norm_first: bool = True, add_prenet: bool = False,
                 scaling_xformers: bool = False, **kwargs):
        if scaling_xformers:
            raise NotImplementedError("Transformer(scaling_xformers=True) (ScaledLinear / BasicNorm / DoubleSwish, "
                                      "valle/models/transformer.py:114-172) is not built: only the stock torch.nn layers are")
        self.engine_opts = dict(precision=kwargs.pop("precision", "bf16"), max_text=kwargs.pop("max_text", 256),
                                max_frames=kwargs.pop("max_frames", 2560), no_graph=kwargs.pop("no_graph", False))
        self.print_eos = kwargs.pop("print_eos", True)
        device = kwargs.pop("device", "cpu")
        if kwargs:
            raise TypeError(f"unexpected arguments {sorted(kwargs)}")
        if self.engine_opts["precision"] not in ("bf16", "fp32", "f32"):
            raise NotImplementedError("the mel-Transformer runs in precision 'bf16' or 'fp32'")
        hd = d_model // nhead if nhead > 0 and d_model % nhead == 0 else 0
        if hd not in (4, 8, 16, 32, 64):  # the engine refuses these too (vx_mel_create)
            raise NotImplementedError(f"head_dim must be 4, 8, 16, 32 or 64 (got {hd})")
        if d_model % 8 or d_model > 1024 or (hd == 64 and d_model % 64):
            raise NotImplementedError("d_model must be a multiple of 8 (of 64 at head_dim 64) and <= 1024")
        self.cfg = MelConfig(d_model=d_model, nhead=nhead, num_layers=num_layers, norm_first=bool(norm_first), add_prenet=bool(add_prenet))
        self.training = True
        self._engine = None
        self.device = torch.device("cpu")
        self._sd = mel_synthetic_state_dict(self.cfg, seed=int(torch.randint(0, 2**31 - 1, (1,))))
        self.to(device)

    # ---- nn.Module-like surface ---------------------------------------------------------------------
    def state_dict(self):
        return OrderedDict(self._sd)

    def load_state_dict(self, state_dict, strict: bool = True):
        want = mel_expected_keys(self.cfg)
        missing = [k for k in want if k not in state_dict]
        unexpected = [k for k in state_dict if k not in want]
        bad = [k for k in want if k in state_dict and tuple(state_dict[k].shape) != tuple(want[k])]
        if bad or (strict and (missing or unexpected)):
            raise RuntimeError(f"Error(s) in loading state_dict for Transformer: missing {missing}, unexpected {unexpected}, "
                               f"size mismatch {bad}")
        for k in want:
            if k in state_dict:
                keep = k.endswith("num_batches_tracked")
                self._sd[k] = state_dict[k].detach().to("cpu", state_dict[k].dtype if keep else torch.float32).contiguous()
        self._drop_engine()
        return _IncompatibleKeys(missing, unexpected)

    def _drop_engine(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    def to(self, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._drop_engine()
        return self

    def cuda(self, index: int = 0):
        return self.to(torch.device("cuda", index))

    def eval(self):
        self.training = False
        return self

    def engine(self):
        """Creates the HIP engine on first use; there is no CPU path."""
        if self._engine is None:
            if self.device.type != "cuda":
                raise RuntimeError("valle_amd.Transformer runs only on an MI355X: call .to('cuda') first (no CPU fallback)")
            from .engine import MelEngine

            self._engine = MelEngine(self.cfg, device=self.device.index or 0, **self.engine_opts)
            self._engine.load_state_dict(self._sd)
        return self._engine

    # ---- checks the reference makes (transformer.py:337-340), and the capacities, before any GPU work ------------------------
    def _check_text(self, x: torch.Tensor, x_lens: torch.Tensor) -> int:
        assert x.ndim == 2, x.shape
        assert x_lens.ndim == 1, x_lens.shape
        assert torch.all(x_lens > 0)
        assert x.shape[0] == 1 and x_lens.shape[0] == 1, "batch 1 only: the reference's loop does not mask finished rows"
        S = int(x_lens[0])
        assert S == x.shape[1], (S, tuple(x.shape))
        if S > self.engine_opts["max_text"]:
            raise ValueError(f"text of {S} ids exceeds max_text={self.engine_opts['max_text']}")
        if bool(((x < 0) | (x >= NUM_TEXT_TOKENS)).any()):
            raise IndexError("index out of range in self")  # nn.Embedding
        return S

    @torch.no_grad()
    def inference(self, x: torch.Tensor, x_lens: torch.Tensor, y=None, max_frames: Optional[int] = None,
                  return_stop_logits: bool = False, **kwargs):
        """transformer.py:320-385: x (1, S) int64, x_lens (1,) -> (1, T, 100) float32 on the model's device, T <= 10 S; ``y`` is
        unused, as in the reference.  ``max_frames`` (an extra): also end once that many frames are out.  With
        ``return_stop_logits`` the result is ``(frames, stop_logits (n_pass,), stop reason)``."""
        S = self._check_text(x, x_lens)
        if max_frames is not None and not 0 <= int(max_frames) <= self.engine_opts["max_frames"]:
            raise ValueError(f"max_frames must be in [0, {self.engine_opts['max_frames']}], got {max_frames}")
        eng = self.engine()
        eng.encode(x[0])
        eng.decode(-1 if max_frames is None else int(max_frames))
        frames, reason, stops = eng.result(out_device=self.device)
        if self.print_eos:
            print(f"TransformerTTS EOS [Text {S} -> Audio {frames.shape[0] + 1}]")  # transformer.py:378-380
        out = frames.unsqueeze(0)
        return (out, stops, reason) if return_stop_logits else out

    @torch.no_grad()
    def inference_waveform(self, x: torch.Tensor, x_lens: torch.Tensor, vocoder=None, **griffinlim_kw):
        """``inference``, then the Griffin-Lim vocoder (``vocoder.GriffinLim``; the device's shared default one when none is given) on
        the same device and stream: ``(mel (1, T, 100), wav (256 T,))``.  ``griffinlim_kw``: n_iter, momentum, rand_init, seed.  A stop
        on pass 0 gives no frame and an empty waveform.  How much of a waveform the vocoder itself keeps is a separate question:
        ``stft.copy_synthesis_distance(wav, vocoder)`` scores wav -> log-mel -> vocoder against wav (multi-resolution STFT)."""
        mel = self.inference(x, x_lens)
        if vocoder is None:
            from .vocoder import shared_griffinlim

            vocoder = shared_griffinlim(self.device)
        return mel, vocoder(mel[0], **griffinlim_kw)

    @torch.no_grad()
    def teacher_forced(self, x: torch.Tensor, x_lens: torch.Tensor, mel: torch.Tensor):
        """The quantities inside the reference's ``forward`` (transformer.py:279-300) for one utterance: mel (1, T, 100) or (T, 100)
        -> ``(predict (T, 100), stop_logits (T,))`` from one causal pass over [0; mel[:-1]].  ``F.mse_loss(predict, mel)`` is the
        reference's reconstruction loss of this checkpoint against that recording's fbank."""
        self._check_text(x, x_lens)
        if mel.ndim == 3:
            assert mel.shape[0] == 1, mel.shape
            mel = mel[0]
        assert mel.ndim == 2, mel.shape
        if mel.shape[1] != NUM_MEL_BINS:
            raise ValueError(f"mel must have {NUM_MEL_BINS} bins per frame, got {tuple(mel.shape)}")
        if not 1 <= mel.shape[0] <= self.engine_opts["max_frames"]:
            raise ValueError(f"mel must have 1..max_frames={self.engine_opts['max_frames']} frames, got {mel.shape[0]}")
        return self.engine().teacher_forced(x[0], mel, out_device=self.device)
