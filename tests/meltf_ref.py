"""The reference's mel-spectrogram Transformer (valle/models/transformer.py) restated functionally in torch, so that it runs in
fp32 AND fp64: the reference class hard-codes a float32 first frame (transformer.py:353-355) and cannot run in fp64 itself.
Test infrastructure: tools/gen_meltf_golden.py asserts that this restatement in fp32 equals the unmodified class frame for frame
before it records the fp64 results the GPU tests compare against.  No cache: every pass recomputes every row, as the reference."""
import math

import torch
import torch.nn.functional as F

NUM_MEL_BINS = 100


def _ln(x, sd, p):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], 1e-5)


def _mha(sd, p, q_in, kv_in, H, causal):
    """torch.nn.MultiheadAttention (packed in_proj), batch 1: q_in (T, d), kv_in (N, d)."""
    d = q_in.shape[-1]
    w, b = sd[p + ".in_proj_weight"], sd[p + ".in_proj_bias"]
    q = F.linear(q_in, w[:d], b[:d]).view(-1, H, d // H).transpose(0, 1)
    k = F.linear(kv_in, w[d:2 * d], b[d:2 * d]).view(-1, H, d // H).transpose(0, 1)
    v = F.linear(kv_in, w[2 * d:], b[2 * d:]).view(-1, H, d // H).transpose(0, 1)
    s = (q @ k.transpose(1, 2)) / math.sqrt(d // H)
    if causal:
        T = q_in.shape[0]
        s = s.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool, device=s.device), diagonal=1), float("-inf"))
    o = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(-1, d)
    return F.linear(o, sd[p + ".out_proj.weight"], sd[p + ".out_proj.bias"])


def _ff(sd, p, x):
    return F.linear(F.relu(F.linear(x, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"])), sd[p + ".linear2.weight"], sd[p + ".linear2.bias"])


def _encoder_layer(sd, p, x, H, norm_first):  # torch.nn.TransformerEncoderLayer.forward
    if norm_first:
        x = x + _mha(sd, p + ".self_attn", _ln(x, sd, p + ".norm1"), _ln(x, sd, p + ".norm1"), H, False)
        return x + _ff(sd, p, _ln(x, sd, p + ".norm2"))
    x = _ln(x + _mha(sd, p + ".self_attn", x, x, H, False), sd, p + ".norm1")
    return _ln(x + _ff(sd, p, x), sd, p + ".norm2")


def _decoder_layer(sd, p, x, mem, H, norm_first):  # torch.nn.TransformerDecoderLayer.forward
    if norm_first:
        h = _ln(x, sd, p + ".norm1")
        x = x + _mha(sd, p + ".self_attn", h, h, H, True)
        x = x + _mha(sd, p + ".multihead_attn", _ln(x, sd, p + ".norm2"), mem, H, False)
        return x + _ff(sd, p, _ln(x, sd, p + ".norm3"))
    x = _ln(x + _mha(sd, p + ".self_attn", x, x, H, True), sd, p + ".norm1")
    x = _ln(x + _mha(sd, p + ".multihead_attn", x, mem, H, False), sd, p + ".norm2")
    return _ln(x + _ff(sd, p, x), sd, p + ".norm3")


class MelRef:
    """sd: the reference's state_dict (any float dtype; cast to ``dtype``); pe: the fp32 sine table (weights.sine_table), model
    data like the weights, cast as they are."""

    def __init__(self, sd, d_model, nhead, num_layers, norm_first=True, add_prenet=False, dtype=torch.float64, pe=None, device="cpu"):
        from valle_amd.weights import sine_table

        self.device = torch.device(device)
        self.sd = {k: (v.to(self.device, dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        self.d, self.H, self.L, self.norm_first, self.add_prenet, self.dtype = d_model, nhead, num_layers, norm_first, add_prenet, dtype
        self.pe = (pe if pe is not None else sine_table(4000, d_model)).to(self.device, dtype)

    def encode(self, ids):
        sd = self.sd
        x = sd["text_embedding.word_embeddings.weight"][ids.to(self.device)]
        if self.add_prenet:  # transformer.py:69-85, eval mode: BatchNorm on its running statistics, no dropout
            h = x.t().unsqueeze(0)
            for conv in (1, 5, 9):
                h = F.conv1d(h, sd[f"encoder_prenet.{conv}.weight"], sd[f"encoder_prenet.{conv}.bias"], padding=2)
                bn = f"encoder_prenet.{conv + 1}"
                h = F.batch_norm(h, sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".bias"], False, 0.0, 1e-5)
                h = F.relu(h)
            x = F.linear(h[0].t(), sd["encoder_prenet.14.weight"], sd["encoder_prenet.14.bias"])
        x = x + sd["encoder_position.alpha"] * self.pe[: x.shape[0]]
        for i in range(self.L):
            x = _encoder_layer(sd, f"encoder.layers.{i}", x, self.H, self.norm_first)
        return _ln(x, sd, "encoder.norm") if self.norm_first else x

    def rows(self, mem, y_in):
        """y_in (T, 100): the decoder's input frames -> (predict (T, 100), stop logits (T,)) under the causal mask."""
        sd = self.sd
        if self.add_prenet:
            h = F.relu(F.linear(y_in, sd["decoder_prenet.0.weight"], sd["decoder_prenet.0.bias"]))
            h = F.relu(F.linear(h, sd["decoder_prenet.3.weight"], sd["decoder_prenet.3.bias"]))
            y = F.linear(h, sd["decoder_prenet.6.weight"], sd["decoder_prenet.6.bias"])
        else:
            y = F.linear(y_in, sd["decoder_prenet.weight"], sd["decoder_prenet.bias"])
        y = y + sd["decoder_position.alpha"] * self.pe[: y.shape[0]]
        for i in range(self.L):
            y = _decoder_layer(sd, f"decoder.layers.{i}", y, mem, self.H, self.norm_first)
        if self.norm_first:
            y = _ln(y, sd, "decoder.norm")
        return F.linear(y, sd["predict_layer.weight"], sd["predict_layer.bias"]), F.linear(y, sd["stop_layer.weight"], sd["stop_layer.bias"])[:, 0]

    @torch.no_grad()
    def teacher_forced(self, ids, frames):
        """transformer.py:279-300: inputs [0; frames[:-1]]."""
        frames = frames.to(self.device, self.dtype)
        y_in = torch.cat([torch.zeros(1, NUM_MEL_BINS, dtype=self.dtype, device=self.device), frames[:-1]], 0)
        return self.rows(self.encode(ids), y_in)

    @torch.no_grad()
    def inference(self, ids, max_frames=None):
        """transformer.py:353-385 -> (frames (T, 100), the stop logit of every pass (T + 1,), stop reason)."""
        mem = self.encode(ids)
        S = ids.numel()
        y = torch.zeros(1, NUM_MEL_BINS, dtype=self.dtype, device=self.device)
        stops = []
        while True:
            predict, stop = self.rows(mem, y)
            stops.append(stop[-1])
            if y.shape[0] > 10 * S:
                reason = "length"
                break
            if bool(stop[-1] > 0):
                reason = "logit"
                break
            if max_frames is not None and y.shape[0] - 1 >= max_frames:
                reason = "max_frames"
                break
            y = torch.cat([y, predict[-1:]], 0)
        return y[1:], torch.stack(stops), reason
