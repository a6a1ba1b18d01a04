"""The CTC recogniser's test cases, shared by test_asr_cpu.py and test_gpu_asr.py: geometries, seeded weights and waveforms, the
restatement's results (computed once per case and left unchanged) and the bounds.

Bound: the project's standing rule, engine max-abs error <= TOL_FACTOR x floor, the floor being the restatement (asr_ref.forward)
in torch fp32 on the host against itself in fp64, per tap and per utterance.  A frame's argmax is compared with fp64's when the
fp64 top-two logit margin exceeds 2 x TOL_FACTOR x the case's logits floor (both logits may move by the bound, in opposite
directions); a frame below that is excused, and at most EXCUSED_SHARE of a case's frames may be."""
import torch

import asr_ref as R

TOL_FACTOR = 4.0
EXCUSED_SHARE = 0.02
WEIGHT_SEED = 0
VOCAB32 = ["<pad>", "<s>", "</s>", "<unk>", "|"] + list("ETAONIHSRDLUMWCFGYPBVK'XJQZ")  # wav2vec2-base-960h's 32 tokens

_TINY = dict(hidden_size=64, num_attention_heads=4, num_hidden_layers=2, intermediate_size=128, conv_dim=(32,) * 7,
             num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, vocab_size=32)
_LAYER = dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)
GEOMETRIES = {
    # name: config fields over Wav2Vec2Config()'s defaults
    "tiny_group": _TINY,
    "tiny_layer": dict(_TINY, **_LAYER),
    "tiny_group_v40": dict(_TINY, vocab_size=40),              # the head through the 64-column GEMM tile
    "tiny_layer_v40": dict(_TINY, vocab_size=40, **_LAYER),
    "tiny_layer_nofpn": dict(_TINY, feat_proj_layer_norm=False, **_LAYER),  # HuBERT's option
    "hd64_group": dict(_TINY, hidden_size=128, num_attention_heads=2),
    "hd64_layer": dict(_TINY, hidden_size=128, num_attention_heads=2, **_LAYER),
    # the released widths, two layers: the float4 gathers, K = 6144 / 8192 in the positional convolution
    "base2": dict(num_hidden_layers=2),
    "large2": dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=2, **_LAYER),
}
FRAMES = (1, 2, 17, 33, 64, 65, 130)  # 1 is the minimum; the others straddle the row tiles (32 / 64 / 128) and the key tile (32)
WIDE_FRAMES = (16, 49)
WIDE = ("base2", "large2")


def config(name):
    from valle_amd.asr import RecognizerConfig

    return RecognizerConfig(**GEOMETRIES[name])


def vocab(name):
    n = int(GEOMETRIES[name].get("vocab_size", 32))
    toks = VOCAB32 + [f"<x{i}>" for i in range(n - len(VOCAB32))]
    return {t: i for i, t in enumerate(toks)}


_SD = {}


def state_dict(name, seed=WEIGHT_SEED):
    """The `transformers`-layout synthetic state dict of a geometry."""
    from valle_amd.asr import synthetic_state_dict

    if (name, seed) not in _SD:
        _SD[(name, seed)] = synthetic_state_dict(config(name), seed)
    return _SD[(name, seed)]


def ref_state_dict(sd):
    """The restatement's layout: no prefix, the positional convolution's weight norm unfolded as weight_g / weight_v."""
    out = {}
    for k, v in sd.items():
        k = k.split(".", 1)[1] if k.startswith(("wav2vec2.", "hubert.")) else k
        k = k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")
        if k != "masked_spec_embed":
            out[k] = v
    return out


def wave(name, frames, seed=None):
    """A seeded 16 kHz waveform that leaves `frames` encoder frames; a few samples more than the fewest that do, so that the strided
    convolutions drop a remainder."""
    cfg = config(name)
    L = R.samples_for_frames(cfg, frames) + frames % 4
    assert R.conv_frames(cfg, L) == frames
    g = torch.Generator().manual_seed(2000 + frames if seed is None else seed)
    t = torch.arange(L) / 16000.0
    return 0.3 * torch.randn(L, generator=g) + 0.2 * torch.sin(2 * torch.pi * (110.0 + 3.0 * frames) * t) + 0.05


_REF = {}


def reference(name, frames, dtype, normalize=False):
    key = (name, frames, dtype, normalize)
    if key not in _REF:
        _REF[key] = R.forward(ref_state_dict(state_dict(name)), config(name), wave(name, frames), dtype, normalize=normalize)
    return _REF[key]


def named_taps(out):
    """name -> tensor over every tap of asr_ref.forward's result: conv0, features, hidden0 .. hidden<L>, logits."""
    flat = {"conv0": out["conv0"], "features": out["features"], "logits": out["logits"]}
    for i, t in enumerate(out["hidden"]):
        flat[f"hidden{i}"] = t
    return flat


def floors(name, frames, normalize=False):
    """tap name -> max-abs error of the fp32 restatement against the fp64 one."""
    r64, r32 = named_taps(reference(name, frames, torch.float64, normalize)), named_taps(reference(name, frames, torch.float32, normalize))
    return {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64}


def decided_frames(name, frames, normalize=False):
    """(fp64 argmax per frame, mask of the frames whose fp64 top-two margin exceeds 2 x TOL_FACTOR x the logits floor)."""
    lg = reference(name, frames, torch.float64, normalize)["logits"]
    top = lg.topk(2, dim=1).values
    return lg.argmax(1), (top[:, 0] - top[:, 1]) > 2 * TOL_FACTOR * floors(name, frames, normalize)["logits"]


def all_cases():
    tiny = [n for n in GEOMETRIES if n not in WIDE]
    return [(n, f) for n in tiny for f in FRAMES] + [(n, f) for n in WIDE for f in WIDE_FRAMES]
