"""Functional restatement of the CTC recogniser (include/vallex.h, vx_asr_*, vx_ctc_greedy, vx_edit_distance): the Wav2Vec2 / HuBERT
CTC network written from its definition with plain tensor operations, the dtype a parameter, and the greedy decode and the edit
distance in numpy.  No `transformers`, no `valle_amd`: the configuration is any object with the `Wav2Vec2Config` attribute names,
the weights a state dict in the `transformers` key layout without the `wav2vec2.` / `hubert.` prefix and with the positional
convolution's weight norm still unfolded (`encoder.pos_conv_embed.conv.weight_g` (1, 1, k) and `.weight_v`).

`forward(..., mutation=NAME)` computes a deliberately wrong variant (MUTATIONS): tests/test_asr_cpu.py checks that every one of
them moves the logits far beyond the GPU test's bound, so that bound can tell them from the definition."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from spk_ref import _gelu, _ln, conv_frames, fold_pos_conv, samples_for_frames  # noqa: F401  the same rules

MUTATIONS = (
    "stable_as_post_norm",     # the stable encoder's weights run through the post-norm order
    "final_norm_dropped",      # stable: no encoder.layer_norm after the last layer
    "conv_norm_after_gelu",    # layer flavour: conv -> GELU -> LayerNorm
    "conv_norm_no_affine",     # layer flavour: the conv LayerNorm without gain and bias
    "conv_bias_dropped",       # layer flavour: the convolutions without their bias
    "proj_norm_skipped",       # the feature projection's LayerNorm left out
    "gelu_tanh",               # the tanh approximation of GELU everywhere
    "residual_from_normed",    # stable: the residual taken from the normed input, h = LN(h) + Attn(LN(h))
)


@torch.no_grad()
def forward(sd, cfg, wav, dtype=torch.float64, normalize=False, mutation=None):
    """One utterance (L,) -> dict: conv0 (T0, C0), features (T, C), hidden [L + 1 x (T, d)], logits (T, vocab)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    P = {k: v.to(dtype) for k, v in sd.items()}
    tanh = mutation == "gelu_tanh"
    eps = float(cfg.layer_norm_eps)
    layer = cfg.feat_extract_norm == "layer"
    stable = bool(cfg.do_stable_layer_norm)
    x = wav.reshape(-1).to(dtype)
    if normalize:
        x = (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-7)
    h = x[None, None]
    out = {}
    for i, s in enumerate(cfg.conv_stride):
        pre = f"feature_extractor.conv_layers.{i}."
        bias = None if mutation == "conv_bias_dropped" else P.get(pre + "conv.bias")
        h = F.conv1d(h, P[pre + "conv.weight"], bias, stride=int(s))
        if layer:  # LayerNorm over the channels of each frame
            w, b = P[pre + "layer_norm.weight"], P[pre + "layer_norm.bias"]
            if mutation == "conv_norm_no_affine":
                w, b = torch.ones_like(w), torch.zeros_like(b)
            if mutation == "conv_norm_after_gelu":
                h = _ln(_gelu(h, tanh).transpose(1, 2), w, b, 1e-5).transpose(1, 2)
            else:
                h = _gelu(_ln(h.transpose(1, 2), w, b, 1e-5).transpose(1, 2), tanh)
        else:
            if i == 0:  # GroupNorm, one group per channel: the utterance's own frames
                m = h.mean(-1, keepdim=True)
                v = h.var(-1, keepdim=True, unbiased=False)
                h = (h - m) / torch.sqrt(v + 1e-5) * P[pre + "layer_norm.weight"][None, :, None] + P[pre + "layer_norm.bias"][None, :, None]
            h = _gelu(h, tanh)
        if i == 0:
            out["conv0"] = h[0].t()
    feats = h[0].t()
    out["features"] = feats
    h = feats
    if bool(cfg.feat_proj_layer_norm) and mutation != "proj_norm_skipped":
        h = _ln(h, P["feature_projection.layer_norm.weight"], P["feature_projection.layer_norm.bias"], eps)
    h = h @ P["feature_projection.projection.weight"].t() + P["feature_projection.projection.bias"]
    T, d = h.shape
    k = int(cfg.num_conv_pos_embeddings)
    w = fold_pos_conv(P["encoder.pos_conv_embed.conv.weight_g"], P["encoder.pos_conv_embed.conv.weight_v"])
    pc = F.conv1d(h.t()[None], w, P["encoder.pos_conv_embed.conv.bias"], padding=k // 2, groups=int(cfg.num_conv_pos_embedding_groups))[0]
    if k % 2 == 0:
        pc = pc[:, :-1]
    h = h + _gelu(pc, tanh).t()
    H = int(cfg.num_attention_heads)
    hd = d // H
    post = not stable or mutation == "stable_as_post_norm"

    def ln(name, t):
        return _ln(t, P[name + ".weight"], P[name + ".bias"], eps)

    def attn(pre, t):
        a = pre + "attention."
        q, kk, v = (t @ P[a + n + ".weight"].t() + P[a + n + ".bias"] for n in ("q_proj", "k_proj", "v_proj"))
        qh, kh, vh = (u.reshape(T, H, hd).permute(1, 0, 2) for u in (q, kk, v))
        o = (torch.softmax((qh * hd ** -0.5) @ kh.transpose(1, 2), -1) @ vh).permute(1, 0, 2).reshape(T, d)
        return o @ P[a + "out_proj.weight"].t() + P[a + "out_proj.bias"]

    def ffn(pre, t):
        f = _gelu(t @ P[pre + "feed_forward.intermediate_dense.weight"].t() + P[pre + "feed_forward.intermediate_dense.bias"], tanh)
        return f @ P[pre + "feed_forward.output_dense.weight"].t() + P[pre + "feed_forward.output_dense.bias"]

    if post:
        h = ln("encoder.layer_norm", h)
    hidden = [h]
    for l in range(int(cfg.num_hidden_layers)):
        pre = f"encoder.layers.{l}."
        if post:
            h = ln(pre + "layer_norm", h + attn(pre, h))
            h = ln(pre + "final_layer_norm", h + ffn(pre, h))
        else:
            n1 = ln(pre + "layer_norm", h)
            h = (n1 if mutation == "residual_from_normed" else h) + attn(pre, n1)
            h = h + ffn(pre, ln(pre + "final_layer_norm", h))
        hidden.append(h)
    if not post and mutation != "final_norm_dropped":
        hidden[-1] = ln("encoder.layer_norm", h)
    out["hidden"] = hidden
    out["logits"] = hidden[-1] @ P["lm_head.weight"].t() + P["lm_head.bias"]
    return out


# ---- greedy CTC ------------------------------------------------------------------------------------------------------------------
def ctc_greedy(logits, blank=0):
    """logits (T, V) -> (ids kept, their frame indices, mean log-probability over all frames, per-frame log-probabilities), fp64.
    The argmax is the lowest index among equal maxima; frame t is kept when id[t] != blank and (t == 0 or id[t] != id[t - 1])."""
    x = np.asarray(logits, dtype=np.float64)
    T = x.shape[0]
    if T == 0:
        return [], [], 0.0, np.zeros(0)
    ids = x.argmax(1)  # numpy: the first occurrence
    mx = x.max(1)
    lp = -np.log(np.exp(x - mx[:, None]).sum(1))
    keep = [t for t in range(T) if ids[t] != blank and (t == 0 or ids[t] != ids[t - 1])]
    return [int(ids[t]) for t in keep], keep, float(lp.mean()), lp


# ---- edit distance ---------------------------------------------------------------------------------------------------------------
def edit_distance(ref, hyp):
    """(distance, substitutions, deletions, insertions) turning ref into hyp, unit costs, the counts carried with the cost: the
    predecessor is the diagonal one (match or substitution) unless the deletion is strictly cheaper, then that unless the insertion is
    strictly cheaper still."""
    R, H = len(ref), len(hyp)
    prev = [(j, 0, 0, j) for j in range(H + 1)]
    for i in range(1, R + 1):
        cur = [(i, 0, i, 0)]
        for j in range(1, H + 1):
            c, s, d, n = prev[j - 1]
            sub = int(ref[i - 1] != hyp[j - 1])
            best = (c + sub, s + sub, d, n)
            c, s, d, n = prev[j]
            if c + 1 < best[0]:
                best = (c + 1, s, d + 1, n)
            c, s, d, n = cur[j - 1]
            if c + 1 < best[0]:
                best = (c + 1, s, d, n + 1)
            cur.append(best)
        prev = cur
    return prev[H]


def edit_distance_fast(ref, hyp):
    """edit_distance for long sequences: the same recurrence over anti-diagonals in numpy, a cell packed as cost << 48 | S << 32 |
    D << 16 | I (lengths up to 2^15).  test_asr_cpu.py checks it against edit_distance."""
    r, h = np.asarray(ref, dtype=np.int64).reshape(-1), np.asarray(hyp, dtype=np.int64).reshape(-1)
    Rn, Hn = len(r), len(h)
    SUB, DEL, INS = (1 << 48) | (1 << 32), (1 << 48) | (1 << 16), (1 << 48) | 1
    p1 = p2 = np.zeros(Rn + 1, dtype=np.int64)
    for d in range(Rn + Hn + 1):
        i = np.arange(max(0, d - Hn), min(Rn, d) + 1)
        j = d - i
        cur = np.zeros(Rn + 1, dtype=np.int64)
        inner = (i > 0) & (j > 0)
        ii, jj = i[inner], j[inner]
        best = p2[ii - 1] + np.where(r[ii - 1] != h[jj - 1], SUB, 0)
        dele, ins = p1[ii - 1] + DEL, p1[ii] + INS
        best = np.where((dele >> 48) < (best >> 48), dele, best)
        best = np.where((ins >> 48) < (best >> 48), ins, best)
        cur[ii] = best
        top = i[(i > 0) & (j == 0)]
        cur[top] = p1[top - 1] + DEL
        if d > 0 and d <= Hn:
            cur[0] = p1[0] + INS
        p2, p1 = p1, cur
    v = int(p1[Rn])
    return v >> 48, (v >> 32) & 0xffff, (v >> 16) & 0xffff, v & 0xffff


# ---- text ------------------------------------------------------------------------------------------------------------------------
def normalize_text(text):
    """Upper-case; letters, digits and apostrophes kept; everything else a space; spaces collapsed."""
    return " ".join("".join(ch if (ch.isalnum() or ch == "'") else " " for ch in str(text).upper()).split())


def error_rate(ref_units, hyp_units):
    """Lists of unit lists -> (corpus rate, [(distance, S, D, I, N)])."""
    rows = [edit_distance(r, h) + (len(r),) for r, h in zip(ref_units, hyp_units)]
    total = sum(r[4] for r in rows)
    return (sum(r[0] for r in rows) / total if total else math.nan), rows
