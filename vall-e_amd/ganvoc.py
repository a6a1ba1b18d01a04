"""Neural vocoder on the GPU: a HiFi-GAN / BigVGAN generator that turns log-mel frames, as `BigVGANFbank` extracts them and
`models.Transformer.inference` predicts them, into a waveform behind `vx_gan_*` (include/vallex.h, csrc/ganvoc_kernels.hpp); there
is no CPU fallback.

    from valle_amd import BigVGAN, GanVocoder
    voc = BigVGAN("bigvgan_24khz_100band", state_dict=torch.load("g_05000000", map_location="cpu")).to("cuda")
    wav = voc(mel)                                        # (T, 100) -> (256 T,) float32 on the device
    wavs = voc.synthesize_batch([mel_a, mel_b])           # one ragged call, every utterance bitwise what it is alone
    mel, wav = model.inference_waveform(x, x_lens, vocoder=voc)

    hifi = GanVocoder(model.config).load_state_dict(model.state_dict()).to("cuda")   # model: a transformers.SpeechT5HifiGan

Two activation modes: `lrelu` (HiFi-GAN) and `snake` / `snakebeta` (BigVGAN's anti-aliased periodic activation).  The definition is
stated in include/vallex.h and restated in fp64 in tests/ganvoc_ref.py.  The presets `bigvgan_24khz_100band` and
`bigvgan_base_24khz_100band` are written down as the published configurations are remembered, not read from the package: a
checkpoint's own `config.json` (pass it as a dict) overrides them.  Neither parity with the NVIDIA package and its key layout nor
anything heard on trained weights is pinned by a test."""
from __future__ import annotations

import ctypes as C
import dataclasses
import re
from typing import Dict, List, Optional, Sequence

import torch

from . import engine as _e
from ._handle import WeightedHandle, i32_array, ptr_array

ACTIVATIONS = {"lrelu": _e.VX_GAN_LRELU, "snake": _e.VX_GAN_SNAKE, "snakebeta": _e.VX_GAN_SNAKEBETA}
N_TAPS = 12


@dataclasses.dataclass
class GanConfig:
    n_mels: int = 100
    rates: Sequence[int] = (8, 8, 2, 2)
    kernels: Sequence[int] = (16, 16, 4, 4)
    initial_channels: int = 512
    resblock_kernels: Sequence[int] = (3, 7, 11)
    dilations: Sequence[Sequence[int]] = ((1, 3, 5), (1, 3, 5), (1, 3, 5))  # one row per resblock kernel
    activation: str = "lrelu"
    alpha_logscale: bool = False
    lrelu_slope: float = 0.1
    normalize_before: bool = True  # SpeechT5HifiGanConfig's: False leaves a state dict's mean / scale buffers unapplied, as the model does

    @property
    def hop(self) -> int:
        h = 1
        for u in self.rates:
            h *= int(u)
        return h

    @classmethod
    def from_dict(cls, d: dict) -> "GanConfig":
        """Our field names, or those of a HiFi-GAN / BigVGAN `config.json` (num_mels, upsample_rates, upsample_kernel_sizes,
        upsample_initial_channel, resblock_kernel_sizes, resblock_dilation_sizes, activation, snake_logscale) and of
        `SpeechT5HifiGanConfig` (model_in_dim, leaky_relu_slope)."""
        alias = {"num_mels": "n_mels", "model_in_dim": "n_mels", "upsample_rates": "rates", "upsample_kernel_sizes": "kernels",
                 "upsample_initial_channel": "initial_channels", "resblock_kernel_sizes": "resblock_kernels",
                 "resblock_dilation_sizes": "dilations", "snake_logscale": "alpha_logscale", "leaky_relu_slope": "lrelu_slope"}
        names = {f.name for f in dataclasses.fields(cls)}
        kw = {}
        for k, v in d.items():
            k = alias.get(k, k)
            if k in names:
                kw[k] = v
        return cls(**kw)


_D135 = ((1, 3, 5), (1, 3, 5), (1, 3, 5))
PRESETS: Dict[str, GanConfig] = {
    "bigvgan_24khz_100band": GanConfig(100, (4, 4, 2, 2, 2, 2), (8, 8, 4, 4, 4, 4), 1536, (3, 7, 11), _D135, "snakebeta", True),
    "bigvgan_base_24khz_100band": GanConfig(100, (8, 8, 2, 2), (16, 16, 4, 4), 512, (3, 7, 11), _D135, "snakebeta", True),
    "hifigan_v1_256": GanConfig(100, (8, 8, 2, 2), (16, 16, 4, 4), 512, (3, 7, 11), _D135, "lrelu", False, 0.1),
}


def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """w = g v / |v| with the norm over every dimension but the first (torch's weight_norm, dim = 0), in fp64, rounded once."""
    v64, g64 = v.detach().double(), g.detach().double()
    norm = v64.reshape(v64.shape[0], -1).norm(dim=1).reshape([-1] + [1] * (v64.dim() - 1))
    return (g64.reshape(norm.shape) * v64 / norm).float()


def canonical_state_dict(sd: dict, config: GanConfig):
    """A HiFi-GAN / BigVGAN generator's state dict -> ({canonical key: fp32 CPU tensor}, filter taps or None).  Accepts weight norm as
    `weight_g` / `weight_v`, as `parametrizations.weight.original0 / original1` or folded (`weight`); the layouts `ups.{i}.0`
    (BigVGAN), `ups.{i}` (HiFi-GAN) and `upsampler.{i}` (SpeechT5HifiGan); a checkpoint wrapped in {"generator": ...}.  The
    `*.upsample.filter` / `*.downsample.lowpass.filter` buffers of the anti-aliased activations must all be equal (they then
    replace the built-in taps); unequal ones raise."""
    if "generator" in sd and isinstance(sd["generator"], dict):
        sd = sd["generator"]
    out: Dict[str, torch.Tensor] = {}
    filters = []
    pending: Dict[str, Dict[str, torch.Tensor]] = {}
    for key, t in sd.items():
        t = torch.as_tensor(t).detach().cpu()
        if key.endswith(".upsample.filter") or key.endswith(".downsample.lowpass.filter"):
            filters.append((key, t.double().reshape(-1)))
            continue
        k = re.sub(r"^upsampler\.(\d+)\.", r"ups.\1.", key)
        k = re.sub(r"^ups\.(\d+)\.0\.", r"ups.\1.", k)
        k = re.sub(r"\.act\.(alpha|beta)$", r".\1", k)
        m = re.match(r"^(.*)\.(weight_g|weight_v|parametrizations\.weight\.original0|parametrizations\.weight\.original1)$", k)
        if m:
            pending.setdefault(m.group(1), {})["g" if m.group(2) in ("weight_g", "parametrizations.weight.original0") else "v"] = t
            continue
        out[k] = t.float()
    for base, gv in pending.items():
        if set(gv) != {"g", "v"}:
            raise KeyError(f"{base}: weight norm needs both weight_g / weight_v (original0 / original1)")
        out[base + ".weight"] = fold_weight_norm(gv["g"], gv["v"])
    taps = None
    if filters:
        first = filters[0][1]
        for key, f in filters[1:]:
            if f.shape != first.shape or not torch.equal(f, first):
                raise ValueError(f"the anti-aliasing filters of the checkpoint differ from one another ({filters[0][0]} against {key}): "
                                 "one filter serves every activation")
        if first.numel() != N_TAPS:
            raise ValueError(f"the checkpoint's anti-aliasing filter has {first.numel()} taps, {N_TAPS} are served")
        taps = first.float().contiguous()
    return out, taps


def expected_keys(config: GanConfig) -> Dict[str, tuple]:
    """canonical key -> shape, as vx_gan_create lays them out (the optional conv_post.bias, mean and scale are not listed)."""
    c = config
    keys = {"conv_pre.weight": (c.initial_channels, c.n_mels, 7), "conv_pre.bias": (c.initial_channels,)}
    ch, R, snake, hasb = c.initial_channels, len(c.resblock_kernels), c.activation != "lrelu", c.activation == "snakebeta"
    for i, k in enumerate(c.kernels):
        keys[f"ups.{i}.weight"], keys[f"ups.{i}.bias"] = (ch, ch // 2, int(k)), (ch // 2,)
        ch //= 2
        for r, rk in enumerate(c.resblock_kernels):
            n = i * R + r
            for m in range(len(c.dilations[r])):
                for cv in ("convs1", "convs2"):
                    keys[f"resblocks.{n}.{cv}.{m}.weight"], keys[f"resblocks.{n}.{cv}.{m}.bias"] = (ch, ch, int(rk)), (ch,)
            if snake:
                for a in range(2 * len(c.dilations[r])):
                    keys[f"resblocks.{n}.activations.{a}.alpha"] = (ch,)
                    if hasb:
                        keys[f"resblocks.{n}.activations.{a}.beta"] = (ch,)
    if snake:
        keys["activation_post.alpha"] = (ch,)
        if hasb:
            keys["activation_post.beta"] = (ch,)
    keys["conv_post.weight"] = (1, ch, 7)
    return keys


OPTIONAL_KEYS = ("conv_post.bias", "mean", "scale")


class GanVocoder(WeightedHandle):
    """`GanVocoder(config, state_dict=None, max_batch=32, max_total_frames=65536)`: `config` is a preset name (`PRESETS`), a
    `GanConfig`, or a dict with its fields or those of the generator's own `config.json`, which therefore overrides a preset:
    `GanVocoder(json.load(open("config.json")))`.  The two BigVGAN presets are written from memory of the published
    configurations.  A call serves up to `max_batch` (<= 64) utterances of `max_total_frames` frames in all."""
    _PREFIX, _NAME = "vx_gan", "GanVocoder"

    def __init__(self, config="bigvgan_24khz_100band", state_dict: Optional[dict] = None, max_batch: int = 32,
                 max_total_frames: int = 65536):
        if isinstance(config, str):
            if config not in PRESETS:
                raise ValueError(f"unknown preset {config!r}: one of {sorted(PRESETS)}")
            config = PRESETS[config]
        elif isinstance(config, dict):
            config = GanConfig.from_dict(config)
        elif not isinstance(config, GanConfig):  # any object with the fields (a dataclass, a namespace, SpeechT5HifiGanConfig)
            fields = ("n_mels", "num_mels", "model_in_dim", "rates", "upsample_rates", "kernels", "upsample_kernel_sizes",
                      "initial_channels", "upsample_initial_channel", "resblock_kernels", "resblock_kernel_sizes", "dilations",
                      "resblock_dilation_sizes", "activation", "alpha_logscale", "snake_logscale", "lrelu_slope", "leaky_relu_slope",
                      "normalize_before")
            config = GanConfig.from_dict({k: getattr(config, k) for k in fields if hasattr(config, k)})
        if config.activation not in ACTIVATIONS:
            raise ValueError(f"activation {config.activation!r}: one of {sorted(ACTIVATIONS)}")
        if len(config.rates) != len(config.kernels):
            raise ValueError("rates and kernels have one entry per stage")
        if len(config.dilations) != len(config.resblock_kernels) or len({len(d) for d in config.dilations}) != 1:
            raise ValueError("dilations has one row per resblock kernel, all of one length")
        self.config = config
        self.max_batch, self.max_total_frames = int(max_batch), int(max_total_frames)
        self._taps: Optional[torch.Tensor] = None
        self._init_handle()  # a geometry the kernels do not serve is refused here
        if state_dict is not None:
            self.load_state_dict(state_dict)

    @property
    def hop(self) -> int:
        return self.config.hop

    def num_samples(self, n_frames: int) -> int:
        return self.hop * int(n_frames) if n_frames > 0 else 0

    # ---- handle -------------------------------------------------------------------------------------
    def _config_struct(self) -> "_e.VxGanConfig":
        c, g = _e.VxGanConfig(), self.config
        c.struct_size = C.sizeof(_e.VxGanConfig)
        c.n_mels, c.n_stages, c.initial_channels = int(g.n_mels), len(g.rates), int(g.initial_channels)
        if not 1 <= len(g.rates) <= 8 or not 1 <= len(g.resblock_kernels) <= 4 or not 1 <= len(g.dilations[0]) <= 4:
            raise ValueError("1..8 stages, 1..4 resblock kernels and 1..4 dilations are served")
        for i, (u, k) in enumerate(zip(g.rates, g.kernels)):
            c.rates[i], c.kernels[i] = int(u), int(k)
        c.n_resblocks, c.n_dilations = len(g.resblock_kernels), len(g.dilations[0])
        for r, rk in enumerate(g.resblock_kernels):
            c.resblock_kernels[r] = int(rk)
            for m, d in enumerate(g.dilations[r]):
                c.dilations[r][m] = int(d)
        c.activation, c.alpha_logscale, c.lrelu_slope = ACTIVATIONS[g.activation], int(bool(g.alpha_logscale)), float(g.lrelu_slope)
        c.max_batch, c.max_total_frames = self.max_batch, self.max_total_frames
        return c

    def _configure(self, lib):
        if self._taps is not None:
            _e._check(lib.vx_gan_set_filter(self._h, self._taps.data_ptr(), N_TAPS))

    @property
    def filter(self) -> torch.Tensor:
        """(12,) float32: the anti-aliasing taps in use (`vx_gan_get_filter`)."""
        out = torch.empty(N_TAPS, dtype=torch.float32)
        _e._check(_e.load_library().vx_gan_get_filter(self._handle(), out.data_ptr()))
        return out

    def load_state_dict(self, sd: dict, filter_taps: Optional[torch.Tensor] = None):
        """Folds weight norm in fp64 and hands the tensors over; missing and unexpected keys raise by name.  Returns self.
        `mean` / `scale` (SpeechT5HifiGan's buffers, which its state dict always holds) are applied to the input unless the
        configuration says `normalize_before=False`: build from the model's own config (`GanVocoder(model.config)`), which carries
        the flag, or drop the two keys yourself."""
        w, taps = canonical_state_dict(sd, self.config)
        if not self.config.normalize_before:  # the model does not apply them either
            w.pop("mean", None), w.pop("scale", None)
        if filter_taps is not None:
            taps = torch.as_tensor(filter_taps).detach().to("cpu", torch.float32).contiguous()
            if taps.numel() != N_TAPS:
                raise ValueError(f"filter_taps has {taps.numel()} entries, {N_TAPS} are served")
        weights = self._checked(expected_keys(self.config), w, optional=OPTIONAL_KEYS, together=("mean", "scale"))
        self._taps = taps
        return self._set_weights(weights)

    # ---- synthesis ----------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, logmel: torch.Tensor) -> torch.Tensor:
        """logmel (T, n_mels) or (1, T, n_mels) float32 -> wav (T * hop,) float32 on the device."""
        return self.synthesize_batch([logmel])[0]

    @torch.no_grad()
    def synthesize_batch(self, logmels: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        """[(T_i, n_mels)] -> [(T_i * hop,)], every utterance bitwise what it is alone; more than `max_batch` utterances, or more
        frames than `max_total_frames`, are served in several calls."""
        self._need_device()
        self._need_weights()
        n_mels = int(self.config.n_mels)
        mels = []
        for m in logmels:
            if m.dim() == 3 and m.shape[0] == 1:
                m = m[0]
            assert m.dim() == 2 and m.shape[1] == n_mels and m.dtype == torch.float32, f"one (T, {n_mels}) float32 log-mel per entry"
            mels.append(m.detach().to(self.device).contiguous())
        wavs = [torch.empty(self.num_samples(m.shape[0]), dtype=torch.float32, device=self.device) for m in mels]
        chunk: List[int] = []
        frames = 0
        for i, m in enumerate(mels + [None]):
            T = 0 if m is None else m.shape[0]
            if chunk and (m is None or len(chunk) == self.max_batch or frames + T > self.max_total_frames):
                with torch.cuda.device(self.device):
                    self._synthesize_raw([mels[j].data_ptr() for j in chunk], [mels[j].shape[0] for j in chunk],
                                         [wavs[j].data_ptr() for j in chunk])
                chunk, frames = [], 0
            if m is not None and T > 0:  # an empty utterance has no storage to point at, and nothing to write
                chunk.append(i)
                frames += T
        return wavs

    def _synthesize_raw(self, mel_ptrs, n_frames, wav_ptrs):
        """vx_gan_synthesize on raw pointers (the argument checks run before any device work)."""
        self._invoke("synthesize", len(mel_ptrs), ptr_array(mel_ptrs), i32_array(n_frames), ptr_array(wav_ptrs))

    def save(self, path: str, wav: torch.Tensor, sample_rate: int = 24000) -> None:
        """16-bit PCM WAV (`codec.save_wav`)."""
        from .codec import save_wav

        save_wav(path, wav, sample_rate)


def BigVGAN(config="bigvgan_24khz_100band", state_dict: Optional[dict] = None, **kw) -> GanVocoder:
    """A `GanVocoder` in BigVGAN's mode: `config` as for `GanVocoder` (a preset name or the checkpoint's `config.json` as a dict; a
    dict without an `activation` gets BigVGAN's default, snakebeta with log-scale parameters)."""
    if isinstance(config, dict) and "activation" not in config:
        config = dict(config, activation="snakebeta", snake_logscale=config.get("snake_logscale", config.get("alpha_logscale", True)))
    v = GanVocoder(config, state_dict=state_dict, **kw)
    if v.config.activation == "lrelu":
        raise ValueError("BigVGAN(...) is the snake / snakebeta generator: a leaky-ReLU configuration is GanVocoder's HiFi-GAN mode")
    return v
