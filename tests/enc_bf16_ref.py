"""Restatement of the recognisers' bf16 encoder mode (include/vallex.h: VX_WSP_ENC_BF16 / VX_ASR_ENC_BF16).  whisper_ref and asr_ref are
imported unchanged: everything up to the first encoder layer and everything after the last one is theirs; this file adds the
pre-norm encoder stack with the definition's roundings, the dtype of the arithmetic (fp32 or fp64) a parameter.

Rounded to bf16 (round-to-nearest-even, torch's `.to(torch.bfloat16)`): the four matrices of every layer; LN1(h), q, k, v, the
softmax probabilities, the attention output, LN2(h) and gelu(W1 x + b1).  Not rounded: every sum, the softmax, biases and LayerNorm
parameters, the residual stream and the last LayerNorm.  The probabilities are rounded after the normalisation here; the engine's
online softmax rounds them before it (a rounding of the same size, inside the bound, not in the definition)."""
import torch
import torch.nn.functional as F

import asr_ref as AR
import whisper_ref as WR


def rb(x):
    """x rounded to bf16, in x's dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def layer(x, p, heads, eps):
    """One pre-norm layer on rows x (T, d).  p: ln1 / ln2 (weight, bias), q / k / v / o / w1 / w2 (weight, bias or None), in x's dtype."""
    T, d = x.shape
    hd = d // heads

    def lin(t, name):
        w, b = p[name]
        return F.linear(t, rb(w), b)

    h = rb(F.layer_norm(x, (d,), p["ln1"][0], p["ln1"][1], eps))
    q, k, v = (rb(lin(h, n)).view(T, heads, hd).transpose(0, 1) for n in ("q", "k", "v"))
    pr = rb(torch.softmax((q * hd ** -0.5) @ k.transpose(1, 2), -1))  # 64^-1/2 is a power of two: scaling q is exact
    o = rb((pr @ v).transpose(0, 1).reshape(T, d))
    x = x + lin(o, "o")
    h = rb(F.layer_norm(x, (d,), p["ln2"][0], p["ln2"][1], eps))
    f = rb(F.gelu(lin(h, "w1")))
    return x + lin(f, "w2")


def _pick(sd, pre, names):
    out = {}
    for short, (name, has_bias) in names.items():
        out[short] = (sd[pre + name + ".weight"], sd.get(pre + name + ".bias") if has_bias else None)
    return out


_WSP = {"ln1": ("self_attn_layer_norm", True), "q": ("self_attn.q_proj", True), "k": ("self_attn.k_proj", False), "v": ("self_attn.v_proj", True),
        "o": ("self_attn.out_proj", True), "ln2": ("final_layer_norm", True), "w1": ("fc1", True), "w2": ("fc2", True)}
_W2V = {"ln1": ("layer_norm", True), "q": ("attention.q_proj", True), "k": ("attention.k_proj", True), "v": ("attention.v_proj", True),
        "o": ("attention.out_proj", True), "ln2": ("final_layer_norm", True), "w1": ("feed_forward.intermediate_dense", True),
        "w2": ("feed_forward.output_dense", True)}


@torch.no_grad()
def whisper_encode(sd, cfg, base, dtype):
    """whisper_ref.encode's dict with the encoder layers in the bf16 mode.  `base`: whisper_ref.encode(...) at `dtype` of the same
    utterance, whose logmel, conv1, features and enc0 are taken as they are."""
    P = WR.cast(sd, dtype)
    out = {k: base[k] for k in ("logmel", "conv1", "features", "enc0")}
    x = base["enc0"].to(dtype)
    for l in range(int(cfg.encoder_layers)):
        x = layer(x, _pick(P, f"model.encoder.layers.{l}.", _WSP), int(cfg.encoder_attention_heads), 1e-5)
        out[f"enc{l + 1}"] = x
    out["pre_norm"] = x
    out["encoder"] = WR._ln(x, P, "model.encoder.layer_norm")
    return out


@torch.no_grad()
def asr_forward(sd, cfg, base, dtype):
    """asr_ref.forward's dict (stable flavour) with the encoder layers in the bf16 mode.  `sd`: the restatement's layout; `base`:
    asr_ref.forward(...) at `dtype` of the same utterance, whose conv0, features and hidden[0] are taken as they are."""
    assert bool(cfg.do_stable_layer_norm), "the mode serves the stable flavour"
    P = {k: v.to(dtype) for k, v in sd.items()}
    eps = float(cfg.layer_norm_eps)
    x = base["hidden"][0].to(dtype)
    hidden = [x]
    for l in range(int(cfg.num_hidden_layers)):
        x = layer(x, _pick(P, f"encoder.layers.{l}.", _W2V), int(cfg.num_attention_heads), eps)
        hidden.append(x)
    hidden[-1] = AR._ln(x, P["encoder.layer_norm.weight"], P["encoder.layer_norm.bias"], eps)
    return {"conv0": base["conv0"], "features": base["features"], "hidden": hidden,
            "logits": hidden[-1] @ P["lm_head.weight"].t() + P["lm_head.bias"]}
