"""The speaker encoder's test cases, shared by test_spk_cpu.py and test_gpu_spk.py: geometries, seeded weights and waveforms, the
restatement's results (computed once per case and left unchanged) and the bound.

Bound: the project's standing rule, engine max-abs error <= TOL_FACTOR x floor, the floor being the restatement (spk_ref.forward)
in torch fp32 on the host against itself in fp64, per tap and per utterance."""
import torch

import spk_ref as R

TOL_FACTOR = 4.0
WEIGHT_SEED = 0
TAPS = ("features", "hidden", "gate", "layer_sum", "tdnn", "pooled", "embedding", "logits")

_TINY = dict(hidden_size=64, num_attention_heads=4, num_hidden_layers=2, intermediate_size=128, conv_dim=(32,) * 7,
             num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, tdnn_dim=(32, 32, 32, 32, 96), xvector_output_dim=24,
             num_buckets=32, max_bucket_distance=40, use_weighted_layer_sum=True)
GEOMETRIES = {
    # name: (attention, config fields over WavLMConfig()'s defaults)
    "tiny_wavlm": ("wavlm", _TINY),
    "tiny_plain": ("plain", _TINY),
    "tiny_last": ("wavlm", dict(_TINY, use_weighted_layer_sum=False)),
    "hd64": ("wavlm", dict(_TINY, hidden_size=128, num_attention_heads=2)),
    # the base widths, two layers: the float4 gathers, K = 6144 in the positional convolution, buckets 320 / 800
    "base2": ("wavlm", dict(num_hidden_layers=2, use_weighted_layer_sum=True)),
}
FRAMES = (16, 17, 31, 33, 63, 64, 65, 130)  # 16 is the minimum; the others straddle the row tiles (32 / 64 / 128) and the key tile (32)
BASE_FRAMES = (16, 49)


def config(name):
    from valle_amd.spk import SpeakerConfig

    return SpeakerConfig(**GEOMETRIES[name][1])


def attention(name):
    return GEOMETRIES[name][0]


_SD = {}


def state_dict(name, seed=WEIGHT_SEED):
    """The `transformers`-layout synthetic state dict of a geometry."""
    from valle_amd.spk import synthetic_state_dict

    if (name, seed) not in _SD:
        _SD[(name, seed)] = synthetic_state_dict(config(name), seed, attention(name))
    return _SD[(name, seed)]


def ref_state_dict(sd):
    """The restatement's layout: no prefix, the positional convolution's weight norm unfolded as weight_g / weight_v."""
    out = {}
    for k, v in sd.items():
        k = k.split(".", 1)[1] if k.startswith(("wavlm.", "wav2vec2.")) else k
        k = k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")
        if k not in ("masked_spec_embed", "objective.weight"):
            out[k] = v
    return out


def wave(name, frames, seed=None):
    """A seeded 16 kHz waveform that leaves `frames` encoder frames; a few samples more than the fewest that do, so that the strided
    convolutions drop a remainder."""
    cfg = config(name)
    L = R.samples_for_frames(cfg, frames) + frames % 4
    assert R.conv_frames(cfg, L) == frames
    g = torch.Generator().manual_seed(1000 + frames if seed is None else seed)
    t = torch.arange(L) / 16000.0
    return 0.3 * torch.randn(L, generator=g) + 0.2 * torch.sin(2 * torch.pi * (110.0 + 3.0 * frames) * t) + 0.05


_REF = {}


def reference(name, frames, dtype, normalize=False):
    key = (name, frames, dtype, normalize)
    if key not in _REF:
        _REF[key] = R.forward(ref_state_dict(state_dict(name)), config(name), wave(name, frames), dtype, attention(name), normalize=normalize)
    return _REF[key]


def named_taps(out):
    """name -> tensor over every tap of spk_ref.forward's result: hidden0 .. hidden<L>, gate0 .. gate<L-1> and the single ones."""
    flat = {}
    for tap in TAPS:
        v = out[tap]
        if isinstance(v, (list, tuple)):
            for i, t in enumerate(v):
                flat[f"{tap}{i}"] = t
        else:
            flat[tap] = v
    return flat


def floors(name, frames, normalize=False):
    """tap name -> max-abs error of the fp32 restatement against the fp64 one."""
    r64, r32 = named_taps(reference(name, frames, torch.float64, normalize)), named_taps(reference(name, frames, torch.float32, normalize))
    return {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64}
