"""What `SpeakerEncoder`, `SpeechRecognizer` and `WhisperRecognizer` share on top of `_handle.WeightedHandle`: the preparation of
the waveforms at 16 kHz, the head of a call on them, and for the two Wav2Vec2 networks the backbone's key table, config fields and
synthetic weights.  Private: the public names stay in spk.py, asr.py and whisper.py."""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import math
from typing import Dict, List

import torch

from . import engine as _e
from ._handle import WeightedHandle, i32_array, prepare_waveforms, ptr_array

SAMPLE_RATE = 16000


def config_from_any(cls, cfg):
    """The body of the config dataclasses' `from_any`: `cfg` is an instance, a dict (a checkpoint's `config.json`), a path to one,
    or any object with the attributes.  A field that is absent or None (a `null` in the json) takes the dataclass's default."""
    if isinstance(cfg, cls):
        return cfg
    if isinstance(cfg, str):
        with open(cfg) as f:
            cfg = json.load(f)
    names = [f.name for f in dataclasses.fields(cls)]
    if isinstance(cfg, dict):
        return cls(**{k: cfg[k] for k in names if k in cfg and cfg[k] is not None})
    return cls(**{k: getattr(cfg, k) for k in names if getattr(cfg, k, None) is not None})


class SpeechHandle(WeightedHandle):
    """The three speech networks at 16 kHz.  A subclass gives `_PREFIX`, `_NAME` and `_config_struct()` and may give
    `_configure(lib)`, which runs between create and the hand-over of the weights, and `_tensors()`."""

    def workspace_bytes(self) -> int:
        out = (C.c_double * 4)()
        _e._check(self._fn("get_timings")(self._handle(), out, 4))
        return int(out[1])

    def read_tap(self, name: str, utt: int, rows: int, width: int) -> torch.Tensor:
        """(rows, width) float32 on the host: a tap of the last call (`vx_*_read`; the parity tests)."""
        out = torch.empty((rows, width), dtype=torch.float32)
        _e._check(self._fn("read")(self._handle(), name.encode(), int(utt), out.data_ptr(), out.numel()))
        return out

    def _prepare(self, wavs, sr: int) -> List[torch.Tensor]:
        """One waveform or a list -> flat float32 tensors on the device at 16 kHz (through the GPU `Resampler` from another rate)."""
        if isinstance(wavs, torch.Tensor):
            wavs = [wavs]
        ws = []
        for w in wavs:
            assert isinstance(w, torch.Tensor) and w.dtype == torch.float32, "waveforms are float32 tensors"
            assert w.numel() == w.shape[-1], "one mono utterance per entry: (L,), (1, L) or (1, 1, L)"
            ws.append(w.detach().reshape(-1))
        self._need_device()
        self._need_weights()
        return prepare_waveforms(self, ws, sr, SAMPLE_RATE, strict=False)

    def _call(self, name: str, wav_ptrs, lengths, *rest):
        """`<_PREFIX>_<name>(handle, n, wav pointers, lengths, *rest, stream)`: the head every call on waveforms has."""
        self._invoke(name, len(wav_ptrs), ptr_array(wav_ptrs), i32_array(lengths), *rest)


class W2vHandle(SpeechHandle):
    """The two networks on the Wav2Vec2 backbone: a feature encoder whose strides fix the frames, `max_batch` x `max_samples`."""

    def _fill_backbone(self, s):
        """The fields `vx_spk_config` and `vx_asr_config` share."""
        c = self.config
        s.hidden, s.layers, s.heads, s.ffn = int(c.hidden_size), int(c.num_hidden_layers), int(c.num_attention_heads), int(c.intermediate_size)
        s.n_conv = len(c.conv_dim)
        for i, (dm, k, st) in enumerate(zip(c.conv_dim, c.conv_kernel, c.conv_stride)):
            s.conv_dim[i], s.conv_kernel[i], s.conv_stride[i] = int(dm), int(k), int(st)
        s.conv_bias = int(bool(c.conv_bias))
        s.pos_kernel, s.pos_groups = int(c.num_conv_pos_embeddings), int(c.num_conv_pos_embedding_groups)
        s.layer_norm_eps = float(c.layer_norm_eps)
        s.max_batch, s.max_samples = self.max_batch, self.max_samples

    def num_frames(self, n_samples: int) -> int:
        """Frames the feature encoder leaves of `n_samples` samples at 16 kHz (host only)."""
        return int(self._fn("frames")(self._handle(), int(n_samples)))

    @property
    def max_frames(self) -> int:
        return self.num_frames(self.max_samples)

    @property
    def min_samples(self) -> int:
        """The shortest utterance served (host only)."""
        return int(self._fn("min_samples")(self._handle()))


def w2v_backbone_keys(c, layer_norms: bool, norm0_last: bool = False, per_layer=None) -> Dict[str, tuple]:
    """canonical key -> shape of `feature_extractor.*`, `feature_projection.*` and `encoder.*`, in the order the synthetic weights
    are drawn in.  `layer_norms`: every conv layer has a LayerNorm (else layer 0 has the GroupNorm; `norm0_last` lists it after
    the convolutions, the speaker encoder's order).  `per_layer(keys, lin, prefix)` adds a layer's own keys after its attention."""
    d = int(c.hidden_size)
    keys: Dict[str, tuple] = {}

    def lin(name, n, k):
        keys[name + ".weight"], keys[name + ".bias"] = (n, k), (n,)

    def norm(name, n):
        keys[name + ".weight"], keys[name + ".bias"] = (n,), (n,)

    cin = 1
    for i, (co, k) in enumerate(zip(c.conv_dim, c.conv_kernel)):
        keys[f"feature_extractor.conv_layers.{i}.conv.weight"] = (int(co), cin, int(k))
        if c.conv_bias:
            keys[f"feature_extractor.conv_layers.{i}.conv.bias"] = (int(co),)
        if layer_norms or (i == 0 and not norm0_last):
            norm(f"feature_extractor.conv_layers.{i}.layer_norm", int(co))
        cin = int(co)
    if norm0_last and not layer_norms:
        norm("feature_extractor.conv_layers.0.layer_norm", int(c.conv_dim[0]))
    if getattr(c, "feat_proj_layer_norm", True):
        norm("feature_projection.layer_norm", cin)
    lin("feature_projection.projection", d, cin)
    keys["encoder.pos_conv_embed.conv.weight"] = (d, d // int(c.num_conv_pos_embedding_groups), int(c.num_conv_pos_embeddings))
    keys["encoder.pos_conv_embed.conv.bias"] = (d,)
    norm("encoder.layer_norm", d)
    for l in range(int(c.num_hidden_layers)):
        pre = f"encoder.layers.{l}."
        for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(pre + "attention." + nm, d, d)
        if per_layer is not None:
            per_layer(keys, lin, pre)
        norm(pre + "layer_norm", d)
        lin(pre + "feed_forward.intermediate_dense", int(c.intermediate_size), d)
        lin(pre + "feed_forward.output_dense", d, int(c.intermediate_size))
        norm(pre + "final_layer_norm", d)
    return keys


def w2v_synthetic_state_dict(keys: Dict[str, tuple], seed: int, prefix: str, is_head, own: Dict[str, tuple], hidden: int) -> Dict[str, torch.Tensor]:
    """Seeded weights for `keys`, drawn in their order, in the `transformers` layout: `prefix` before every key but the head's
    (`is_head(key)`), the positional convolution's weight norm unfolded, `masked_spec_embed` last.  `own`: key suffix ->
    (offset, scale) of the tensors a network scales its own way; the others get norm gains and biases away from 1 and 0, a layer-0
    convolution of order one and unit gain over the fan-in elsewhere."""
    g = torch.Generator().manual_seed(int(seed))
    sd: Dict[str, torch.Tensor] = {}

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    for k, shape in keys.items():
        name = k if is_head(k) else prefix + k
        mine = [v for suffix, v in own.items() if k.endswith(suffix)]
        if k == "encoder.pos_conv_embed.conv.weight":
            sd[prefix + "encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = 0.5 + torch.rand(1, 1, shape[2], generator=g)
            sd[prefix + "encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = rnd(*shape)
        elif mine:
            offset, scale = mine[0]
            sd[name] = offset + rnd(*shape, scale=scale) if offset else rnd(*shape, scale=scale)
        elif k.endswith("layer_norm.weight"):
            sd[name] = 1.0 + rnd(*shape, scale=0.2)
        elif k.endswith("layer_norm.bias"):
            sd[name] = rnd(*shape, scale=0.5)
        elif k.endswith(".bias"):
            sd[name] = rnd(*shape, scale=0.1)
        elif k == "feature_extractor.conv_layers.0.conv.weight":
            sd[name] = rnd(*shape, scale=1.0)
        else:  # Linear and convolution weights: unit gain over the fan-in
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            sd[name] = rnd(*shape, scale=1.5 / math.sqrt(fan_in))
    sd[prefix + "masked_spec_embed"] = rnd(int(hidden))
    return sd
