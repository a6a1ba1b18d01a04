"""Functional restatement of the speaker encoder (include/vallex.h, vx_spk_*): the WavLM / Wav2Vec2 x-vector network written from
its definition with plain tensor operations, the dtype a parameter.  No `transformers`, no `valle_amd`: the configuration is any
object with the `WavLMConfig` attribute names, the weights a state dict in the `transformers` key layout without the
`wavlm.` / `wav2vec2.` prefix and with the positional convolution's weight norm still unfolded
(`encoder.pos_conv_embed.conv.weight_g` (1, 1, k) and `.weight_v`).

`forward(..., mutation=NAME)` computes a deliberately wrong variant (MUTATIONS): tests/test_spk_cpu.py checks that every one of
them moves the embedding far beyond the GPU test's bound, so that bound can tell them from the definition."""
import math

import torch
import torch.nn.functional as F

MUTATIONS = (
    "gate_dropped",          # gate = 1
    "gate_from_q",           # gate from the projected query's head slice instead of the layer input's
    "bias_transposed",       # bias[h, i - j] in place of bias[h, j - i]
    "bias_not_shared",       # no position bias past layer 0
    "pool_biased_std",       # biased standard deviation in the statistics pooling
    "keep_last_frame",       # even-k positional convolution: the last frame kept (and the first dropped) instead of dropped
    "weight_norm_dim",       # weight norm over (in, tap) per output channel (dim = 0) instead of over (out, in) per tap (dim = 2)
    "layer_weights_raw",     # layer weights not soft-maxed
    "layer_sum_skip_input",  # the input to layer 0 left out of the weighted layer sum
    "gn_unbiased",           # GroupNorm with the unbiased variance
    "gelu_tanh",             # the tanh approximation of GELU everywhere
    "tdnn_order_swapped",    # the TDNN Linear read in (channel, tap) order
)


def relative_position_buckets(rel: torch.Tensor, num_buckets: int, max_distance: int) -> torch.Tensor:
    """int64 bucket of every relative position j - i in `rel`: positive positions offset by num_buckets / 2, exact below
    max_exact = num_buckets / 4, logarithmic above (the logarithm in fp32, as torch takes it), saturated at max_distance."""
    nb = num_buckets // 2
    out = (rel > 0).to(torch.long) * nb
    a = rel.abs()
    max_exact = nb // 2
    large = torch.log(a.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)
    large = (max_exact + large).to(torch.long)
    large = torch.minimum(large, torch.full_like(large, nb - 1))
    return out + torch.where(a < max_exact, a, large)


def conv_frames(cfg, n_samples: int) -> int:
    L = int(n_samples)
    for k, s in zip(cfg.conv_kernel, cfg.conv_stride):
        L = (L - int(k)) // int(s) + 1 if L >= int(k) else 0
    return L


def min_samples(cfg) -> int:
    """The shortest input that leaves two pooled frames."""
    need = 2 + sum(int(d) * (int(k) - 1) for k, d in zip(cfg.tdnn_kernel, cfg.tdnn_dilation))
    for k, s in zip(reversed(list(cfg.conv_kernel)), reversed(list(cfg.conv_stride))):
        need = (need - 1) * int(s) + int(k)
    return need


def samples_for_frames(cfg, frames: int) -> int:
    need = int(frames)
    for k, s in zip(reversed(list(cfg.conv_kernel)), reversed(list(cfg.conv_stride))):
        need = (need - 1) * int(s) + int(k)
    return need


def _gelu(x, tanh=False):
    if tanh:
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _ln(x, w, b, eps):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * w + b


def fold_pos_conv(g, v, wrong_dim=False):
    """w = g v / |v|: the norm over (out, in) per tap (weight_norm dim = 2)."""
    if wrong_dim:
        return g.reshape(1, 1, -1) * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)
    return g.reshape(1, 1, -1) * v / v.permute(2, 0, 1).flatten(1).norm(dim=1).reshape(1, 1, -1)


@torch.no_grad()
def forward(sd, cfg, wav, dtype=torch.float64, attention="wavlm", normalize=False, mutation=None, device=None):
    """One utterance (L,) -> dict: embedding (xvector,), logits (xvector,), features (T, C), hidden [L + 1 x (T, d)],
    gate [L x (T, H)] (wavlm), layer_sum (T, d), tdnn (T', tdnn[-1]), pooled (2 tdnn[-1],)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    dev = torch.device(device) if device is not None else wav.device
    P = {k: v.to(dev, dtype) for k, v in sd.items()}
    tanh = mutation == "gelu_tanh"
    eps = float(cfg.layer_norm_eps)
    x = wav.reshape(-1).to(dev, dtype)
    if normalize:
        x = (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-7)
    h = x[None, None]
    for i, s in enumerate(cfg.conv_stride):
        pre = f"feature_extractor.conv_layers.{i}."
        h = F.conv1d(h, P[pre + "conv.weight"], P.get(pre + "conv.bias"), stride=int(s))
        if i == 0:  # GroupNorm, one group per channel: the utterance's own frames
            m = h.mean(-1, keepdim=True)
            v = h.var(-1, keepdim=True, unbiased=mutation == "gn_unbiased")
            h = (h - m) / torch.sqrt(v + 1e-5) * P[pre + "layer_norm.weight"][None, :, None] + P[pre + "layer_norm.bias"][None, :, None]
        h = _gelu(h, tanh)
    feats = h[0].t()
    out = {"features": feats}
    h = _ln(feats, P["feature_projection.layer_norm.weight"], P["feature_projection.layer_norm.bias"], eps)
    h = h @ P["feature_projection.projection.weight"].t() + P["feature_projection.projection.bias"]
    T, d = h.shape
    k = int(cfg.num_conv_pos_embeddings)
    w = fold_pos_conv(P["encoder.pos_conv_embed.conv.weight_g"], P["encoder.pos_conv_embed.conv.weight_v"], mutation == "weight_norm_dim")
    pc = F.conv1d(h.t()[None], w, P["encoder.pos_conv_embed.conv.bias"], padding=k // 2, groups=int(cfg.num_conv_pos_embedding_groups))[0]
    if k % 2 == 0:
        pc = pc[:, 1:] if mutation == "keep_last_frame" else pc[:, :-1]
    h = _ln(h + _gelu(pc, tanh).t(), P["encoder.layer_norm.weight"], P["encoder.layer_norm.bias"], eps)
    H = int(cfg.num_attention_heads)
    hd = d // H
    hidden, gates = [h], []
    bias = None
    if attention == "wavlm":
        pos = torch.arange(T)
        rel = pos[None, :] - pos[:, None]  # j - i
        if mutation == "bias_transposed":
            rel = -rel
        bucket = relative_position_buckets(rel, int(cfg.num_buckets), int(cfg.max_bucket_distance)).to(dev)
        bias = P["encoder.layers.0.attention.rel_attn_embed.weight"][bucket].permute(2, 0, 1)  # (H, T, T)
    for l in range(int(cfg.num_hidden_layers)):
        pre = f"encoder.layers.{l}."
        a = pre + "attention."
        q = h @ P[a + "q_proj.weight"].t() + P[a + "q_proj.bias"]
        kk = h @ P[a + "k_proj.weight"].t() + P[a + "k_proj.bias"]
        v = h @ P[a + "v_proj.weight"].t() + P[a + "v_proj.bias"]
        qh, kh, vh = (t.reshape(T, H, hd).permute(1, 0, 2) for t in (q, kk, v))
        scores = (qh * hd ** -0.5) @ kh.transpose(1, 2)
        if bias is not None:
            src = q if mutation == "gate_from_q" else h
            p = src.reshape(T, H, hd) @ P[a + "gru_rel_pos_linear.weight"].t() + P[a + "gru_rel_pos_linear.bias"]  # (T, H, 8)
            ga = torch.sigmoid(p[..., :4].sum(-1))
            gb = torch.sigmoid(p[..., 4:].sum(-1))
            gate = ga * (gb * P[a + "gru_rel_pos_const"].reshape(1, H) - 1.0) + 2.0  # (T, H)
            gates.append(gate)
            if mutation == "gate_dropped":
                gate = torch.ones_like(gate)
            if not (mutation == "bias_not_shared" and l > 0):
                scores = scores + gate.t()[:, :, None] * bias
        o = (torch.softmax(scores, -1) @ vh).permute(1, 0, 2).reshape(T, d)
        o = o @ P[a + "out_proj.weight"].t() + P[a + "out_proj.bias"]
        h = _ln(h + o, P[pre + "layer_norm.weight"], P[pre + "layer_norm.bias"], eps)
        f = _gelu(h @ P[pre + "feed_forward.intermediate_dense.weight"].t() + P[pre + "feed_forward.intermediate_dense.bias"], tanh)
        f = f @ P[pre + "feed_forward.output_dense.weight"].t() + P[pre + "feed_forward.output_dense.bias"]
        h = _ln(h + f, P[pre + "final_layer_norm.weight"], P[pre + "final_layer_norm.bias"], eps)
        hidden.append(h)
    out["hidden"], out["gate"] = hidden, gates
    if bool(cfg.use_weighted_layer_sum):
        lw = P["layer_weights"] if mutation == "layer_weights_raw" else torch.softmax(P["layer_weights"], -1)
        s = torch.zeros_like(h)
        for l, hl in enumerate(hidden):  # in layer order
            if l == 0 and mutation == "layer_sum_skip_input":
                continue
            s = s + lw[l] * hl
        h = s
    out["layer_sum"] = h
    h = h @ P["projector.weight"].t() + P["projector.bias"]
    cin = int(cfg.tdnn_dim[0])
    for i, (co, kt, dl) in enumerate(zip(cfg.tdnn_dim, cfg.tdnn_kernel, cfg.tdnn_dilation)):
        W = P[f"tdnn.{i}.kernel.weight"]
        if mutation == "tdnn_order_swapped":
            W = W.reshape(int(co), cin, int(kt))
        else:
            W = W.reshape(int(co), int(kt), cin).transpose(1, 2)
        h = torch.relu(F.conv1d(h.t()[None], W, P[f"tdnn.{i}.kernel.bias"], dilation=int(dl))[0].t())
        cin = int(co)
    out["tdnn"] = h
    pooled = torch.cat([h.mean(0), h.std(0, unbiased=mutation != "pool_biased_std")])
    out["pooled"] = pooled
    emb = P["feature_extractor.weight"] @ pooled + P["feature_extractor.bias"]
    out["embedding"] = emb
    out["logits"] = P["classifier.weight"] @ emb + P["classifier.bias"]
    return out


def cosine(a, b):
    a, b = a.double(), b.double()
    return float((a * b).sum() / max(float(a.norm() * b.norm()), 1e-8))
