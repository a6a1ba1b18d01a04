"""Speaker encoder on the GPU: the WavLM / Wav2Vec2 x-vector network (`transformers.WavLMForXVector`, the network of
`microsoft/wavlm-base-plus-sv`) behind `vx_spk_*` (include/vallex.h, csrc/spk_kernels.hpp), and the speaker similarity ("SIM") of
two utterances, the cosine of their embeddings; there is no CPU fallback.

    from valle_amd import SpeakerEncoder, speaker_similarity
    enc = SpeakerEncoder(json.load(open("config.json"))).load_state_dict(torch.load("pytorch_model.bin")).to("cuda")
    emb = enc.embed([prompt_wav, synth_wav], sr=24000)         # (2, 512) float32 on the device, one ragged call
    sim = speaker_similarity(prompt_wav, synth_wav, encoder=enc, sr=24000)

Two attention modes: `wavlm` (gated, bucketed relative position bias) and `plain` (`Wav2Vec2ForXVector`: the same network without
the bias).  The definition is stated in include/vallex.h and restated in fp64 in tests/spk_ref.py, which tests/test_spk_cpu.py pins
against the two `transformers` classes.  Nothing has been heard or scored on trained weights: no checkpoint is available where
this is built, and on synthetic weights the similarity means nothing."""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import re
from typing import Dict, Optional, Sequence, Union

import torch

from . import engine as _e
from ._speech_handle import SAMPLE_RATE, W2vHandle, config_from_any, w2v_backbone_keys, w2v_synthetic_state_dict

ATTENTION = {"wavlm": _e.VX_SPK_WAVLM, "plain": _e.VX_SPK_PLAIN}
HEAD_DIMS = (16, 32, 64)


@dataclasses.dataclass
class SpeakerConfig:
    """The fields of `WavLMConfig` / `Wav2Vec2Config` the network reads, under their names and with `WavLMConfig()`'s defaults."""
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    conv_dim: Sequence[int] = (512, 512, 512, 512, 512, 512, 512)
    conv_kernel: Sequence[int] = (10, 3, 3, 3, 3, 2, 2)
    conv_stride: Sequence[int] = (5, 2, 2, 2, 2, 2, 2)
    conv_bias: bool = False
    num_conv_pos_embeddings: int = 128
    num_conv_pos_embedding_groups: int = 16
    num_buckets: int = 320
    max_bucket_distance: int = 800
    tdnn_dim: Sequence[int] = (512, 512, 512, 512, 1500)
    tdnn_kernel: Sequence[int] = (5, 3, 3, 1, 1)
    tdnn_dilation: Sequence[int] = (1, 2, 3, 1, 1)
    xvector_output_dim: int = 512
    layer_norm_eps: float = 1e-5
    use_weighted_layer_sum: bool = False
    feat_extract_norm: str = "group"
    feat_extract_activation: str = "gelu"
    hidden_act: str = "gelu"
    do_stable_layer_norm: bool = False
    add_adapter: bool = False

    @classmethod
    def from_any(cls, cfg) -> "SpeakerConfig":
        """A dict (a checkpoint's `config.json`), a path to one, or any object with the attributes; a field that is absent or
        None (a `null` in the json) takes the default."""
        return config_from_any(cls, cfg)


PRESETS: Dict[str, SpeakerConfig] = {
    # WavLMConfig()'s defaults with the layer sum the speaker-verification checkpoint uses; its own config.json overrides this
    "wavlm_base_plus_sv": SpeakerConfig(use_weighted_layer_sum=True),
}


def relative_position_buckets(rel: torch.Tensor, num_buckets: int, max_distance: int) -> torch.Tensor:
    """WavLM's `_relative_positions_bucket` for relative positions j - i: positive ones offset by num_buckets / 2, exact below
    num_buckets / 4, logarithmic above with the logarithm taken in fp32 as torch takes it, saturated at max_distance."""
    nb = num_buckets // 2
    out = (rel > 0).to(torch.long) * nb
    a = rel.abs()
    max_exact = nb // 2
    large = torch.log(a.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)
    large = (max_exact + large).to(torch.long)
    large = torch.minimum(large, torch.full_like(large, nb - 1))
    return out + torch.where(a < max_exact, a, large)


def fold_pos_conv_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """w = g v / |v| for weight_norm(dim=2): g is (1, 1, k) and the norm runs over (out, in) per tap; fp64, rounded once."""
    v64, g64 = v.detach().double(), g.detach().double().reshape(1, 1, -1)
    norm = v64.permute(2, 0, 1).flatten(1).norm(dim=1).reshape(1, 1, -1)
    return (g64 * v64 / norm).float()


def expected_keys(c: SpeakerConfig, attention: str = "wavlm") -> Dict[str, tuple]:
    """canonical key -> shape, as vx_spk_create lays them out."""
    d, H, L = int(c.hidden_size), int(c.num_attention_heads), int(c.num_hidden_layers)

    def gate(keys, lin, pre):
        lin(pre + "attention.gru_rel_pos_linear", 8, d // H)
        keys[pre + "attention.gru_rel_pos_const"] = (1, H, 1, 1)

    keys = w2v_backbone_keys(c, False, norm0_last=True, per_layer=gate if attention == "wavlm" else None)

    def lin(name, n, k):
        keys[name + ".weight"], keys[name + ".bias"] = (n, k), (n,)

    if attention == "wavlm":
        keys["encoder.layers.0.attention.rel_attn_embed.weight"] = (int(c.num_buckets), H)
    if c.use_weighted_layer_sum:
        keys["layer_weights"] = (L + 1,)
    lin("projector", int(c.tdnn_dim[0]), d)
    cin = int(c.tdnn_dim[0])
    for i, (co, k) in enumerate(zip(c.tdnn_dim, c.tdnn_kernel)):
        lin(f"tdnn.{i}.kernel", int(co), cin * int(k))
        cin = int(co)
    lin("feature_extractor", int(c.xvector_output_dim), 2 * cin)
    lin("classifier", int(c.xvector_output_dim), int(c.xvector_output_dim))
    return keys


IGNORED_KEYS = ("masked_spec_embed", "objective.weight")


def canonical_state_dict(sd: dict) -> Dict[str, torch.Tensor]:
    """A `WavLMForXVector` / `Wav2Vec2ForXVector` state dict -> {canonical key: fp32 CPU tensor}: the `wavlm.` / `wav2vec2.` prefix
    dropped, the positional convolution's weight norm folded (`parametrizations.weight.original0 / original1` or the legacy
    `weight_g / weight_v`), `masked_spec_embed` and `objective.weight` ignored."""
    out: Dict[str, torch.Tensor] = {}
    gv: Dict[str, torch.Tensor] = {}
    for key, t in sd.items():
        t = torch.as_tensor(t).detach().cpu()
        k = re.sub(r"^(wavlm|wav2vec2)\.", "", key)
        if k in IGNORED_KEYS:
            continue
        m = re.match(r"^encoder\.pos_conv_embed\.conv\.(weight_g|weight_v|parametrizations\.weight\.original0|parametrizations\.weight\.original1)$", k)
        if m:
            gv["g" if m.group(1) in ("weight_g", "parametrizations.weight.original0") else "v"] = t
            continue
        out[k] = t.float()
    if gv:
        if set(gv) != {"g", "v"}:
            raise KeyError("encoder.pos_conv_embed.conv: weight norm needs both weight_g / weight_v (original0 / original1)")
        out["encoder.pos_conv_embed.conv.weight"] = fold_pos_conv_weight_norm(gv["g"], gv["v"])
    return out


def synthetic_state_dict(config, seed: int = 0, attention: str = "wavlm") -> Dict[str, torch.Tensor]:
    """Seeded weights in the `transformers` layout (prefix `wavlm.` / `wav2vec2.`, weight norm unfolded) for the tests.  The scales
    keep every stage alive and make every part of the definition matter: a relative position embedding and gate weights of order
    one (so the bias, its gate and its direction move the output), a GroupNorm bias and convolution gains that put the GELUs in
    their curved range, unequal layer weights."""
    c = SpeakerConfig.from_any(config)
    keys = expected_keys(c, attention)

    def is_head(k):
        return k.split(".")[0] in ("projector", "tdnn", "classifier", "layer_weights") or k.startswith("feature_extractor.weight") \
            or k.startswith("feature_extractor.bias")

    own = {"rel_attn_embed.weight": (0.0, 2.0), "gru_rel_pos_linear.weight": (0.0, 0.5), "gru_rel_pos_const": (1.0, 0.5),
           "layer_weights": (0.0, 1.0)}
    return w2v_synthetic_state_dict(keys, seed, "wavlm." if attention == "wavlm" else "wav2vec2.", is_head, own, int(c.hidden_size))


class SpeakerEncoder(W2vHandle):
    """`SpeakerEncoder(config=None, attention="wavlm", max_batch=32, max_seconds=20.0)`: `config` is a preset name (`PRESETS`,
    default `wavlm_base_plus_sv`), a `SpeakerConfig`, a dict or path of the checkpoint's `config.json`, or any object with the
    `WavLMConfig` / `Wav2Vec2Config` attributes.  A call serves up to `max_batch` (<= 64) utterances of up to `max_seconds` at
    16 kHz each; the workspace is sized from the two.  Head dimensions 16, 32 and 64 are served; `feat_extract_norm="layer"`,
    `do_stable_layer_norm`, adapters and activations other than GELU raise NotImplementedError."""
    _PREFIX, _NAME = "vx_spk", "SpeakerEncoder"

    def __init__(self, config=None, attention: str = "wavlm", max_batch: int = 32, max_seconds: float = 20.0,
                 state_dict: Optional[dict] = None, keep_taps: bool = False):
        if config is None:
            config = "wavlm_base_plus_sv"
        if isinstance(config, str) and config in PRESETS:
            config = PRESETS[config]
        config = SpeakerConfig.from_any(config)
        if attention not in ATTENTION:
            raise ValueError(f"attention {attention!r}: one of {sorted(ATTENTION)}")
        c = config
        if c.feat_extract_norm != "group":
            raise NotImplementedError(f"feat_extract_norm = {c.feat_extract_norm!r}: the group-norm feature encoder is served")
        if c.do_stable_layer_norm:
            raise NotImplementedError("do_stable_layer_norm: the post-norm encoder is served")
        if c.add_adapter:
            raise NotImplementedError("add_adapter: adapters are not served")
        if c.feat_extract_activation != "gelu" or c.hidden_act != "gelu":
            raise NotImplementedError(f"activations {c.feat_extract_activation!r} / {c.hidden_act!r}: gelu is served")
        if int(c.hidden_size) % int(c.num_attention_heads) or int(c.hidden_size) // int(c.num_attention_heads) not in HEAD_DIMS:
            raise NotImplementedError(f"head_dim = {c.hidden_size} / {c.num_attention_heads}: {HEAD_DIMS} are served")
        if not (len(c.conv_dim) == len(c.conv_kernel) == len(c.conv_stride)) or not 1 <= len(c.conv_dim) <= 8:
            raise ValueError("conv_dim, conv_kernel and conv_stride have one entry per layer, 1..8 layers")
        if not (len(c.tdnn_dim) == len(c.tdnn_kernel) == len(c.tdnn_dilation)) or not 1 <= len(c.tdnn_dim) <= 8:
            raise ValueError("tdnn_dim, tdnn_kernel and tdnn_dilation have one entry per layer, 1..8 layers")
        self.config, self.attention = config, attention
        self.max_batch, self.max_samples = int(max_batch), int(round(float(max_seconds) * SAMPLE_RATE))
        self.keep_taps = bool(keep_taps)
        self._init_handle()
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # ---- handle -------------------------------------------------------------------------------------
    def _config_struct(self) -> "_e.VxSpkConfig":
        s, c = _e.VxSpkConfig(), self.config
        s.struct_size = C.sizeof(_e.VxSpkConfig)
        s.attention = ATTENTION[self.attention]
        self._fill_backbone(s)
        s.num_buckets = int(c.num_buckets)
        s.n_tdnn = len(c.tdnn_dim)
        for i, (dm, k, dl) in enumerate(zip(c.tdnn_dim, c.tdnn_kernel, c.tdnn_dilation)):
            s.tdnn_dim[i], s.tdnn_kernel[i], s.tdnn_dilation[i] = int(dm), int(k), int(dl)
        s.xvector = int(c.xvector_output_dim)
        s.use_weighted_layer_sum = int(bool(c.use_weighted_layer_sum))
        s.flags = _e.VX_SPK_KEEP_TAPS if self.keep_taps else 0
        return s

    def _configure(self, lib):
        if self._weights is not None and self.attention == "wavlm":
            T = self.max_frames
            idx = relative_position_buckets(torch.arange(-(T - 1), T), int(self.config.num_buckets),
                                            int(self.config.max_bucket_distance)).to(torch.int32).contiguous()
            _e._check(lib.vx_spk_set_buckets(self._h, idx.data_ptr(), idx.numel()))

    @property
    def min_samples(self) -> int:
        """The shortest utterance served (two pooled frames): 5200 samples at the default strides and TDNN kernels."""
        return super().min_samples

    @property
    def embedding_dim(self) -> int:
        return int(self.config.xvector_output_dim)

    def load_state_dict(self, sd: dict):
        """Takes the `transformers` key layout (see `canonical_state_dict`); missing and unexpected keys and wrong shapes raise by
        name.  Returns self."""
        return self._check_state_dict(expected_keys(self.config, self.attention), canonical_state_dict(sd))

    # ---- embedding ----------------------------------------------------------------------------------
    @torch.no_grad()
    def embed(self, wavs: Union[torch.Tensor, Sequence[torch.Tensor]], sr: int = 24000, normalize: bool = False,
              return_logits: bool = False):
        """One waveform or a list of ragged ones, float32 (L,), (1, L) or (1, 1, L) at `sr` -> (n, xvector) float32 on the device
        (with `return_logits`: the pair (embeddings, logits)).  Audio at another rate than 16 kHz goes through the GPU `Resampler`
        first.  `normalize=True` applies the Wav2Vec2 feature extractor's zero-mean unit-variance rule per utterance: the
        checkpoint's `preprocessor_config.json` (`do_normalize`) says which it wants.  More than `max_batch` utterances are served
        in several calls; every utterance is bitwise what it is alone."""
        ws = self._prepare(wavs, sr)
        n = len(ws)
        emb = torch.empty((n, self.embedding_dim), dtype=torch.float32, device=self.device)
        logits = torch.empty_like(emb) if return_logits else None
        for i in range(0, n, self.max_batch):
            chunk = ws[i:i + self.max_batch]
            with torch.cuda.device(self.device):
                self._embed_raw([w.data_ptr() for w in chunk], [w.numel() for w in chunk], normalize, emb[i:].data_ptr(),
                                None if logits is None else logits[i:].data_ptr())
        return (emb, logits) if return_logits else emb

    def _embed_raw(self, wav_ptrs, lengths, normalize, emb_ptr, logits_ptr):
        """vx_spk_embed on raw pointers (the argument checks run before any device work)."""
        self._call("embed", wav_ptrs, lengths, _e.VX_SPK_NORMALIZE if normalize else 0, emb_ptr, logits_ptr)

    @torch.no_grad()
    def cosine(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """(n, xvector) x (n, xvector) embeddings on the device -> (n,) cosines (`vx_spk_similarity`)."""
        self._need_device()
        a = a.detach().to(self.device, torch.float32).reshape(-1, self.embedding_dim).contiguous()
        b = b.detach().to(self.device, torch.float32).reshape(-1, self.embedding_dim).contiguous()
        assert a.shape == b.shape, "one embedding of b per embedding of a"
        out = torch.empty(a.shape[0], dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._invoke("similarity", a.shape[0], a.data_ptr(), b.data_ptr(), out.data_ptr())
        return out

    @torch.no_grad()
    def similarity(self, a, b, sr: int = 24000, normalize: bool = False) -> torch.Tensor:
        """Speaker similarity of waveform(s) `a` against waveform(s) `b` (one tensor or equally long lists): (n,) cosines of their
        embeddings on the device, all utterances embedded in one ragged call when they fit `max_batch`."""
        la = [a] if isinstance(a, torch.Tensor) else list(a)
        lb = [b] if isinstance(b, torch.Tensor) else list(b)
        assert len(la) == len(lb), "one waveform of b per waveform of a"
        emb = self.embed(la + lb, sr=sr, normalize=normalize)
        return self.cosine(emb[:len(la)], emb[len(la):])


def speaker_similarity(prompt_wav: torch.Tensor, synth_wav: torch.Tensor, encoder: SpeakerEncoder, sr: int = 24000,
                       normalize: bool = False) -> torch.Tensor:
    """"SIM": the cosine of the speaker embeddings of the prompt and of the synthesised utterance, a 0-dim tensor on the device.
    On synthetic weights the number means nothing."""
    return encoder.similarity(prompt_wav, synth_wav, sr=sr, normalize=normalize)[0]
