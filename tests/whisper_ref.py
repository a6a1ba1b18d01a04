"""The Whisper recogniser's definition (include/vallex.h, vx_wsp_*) restated in torch at a chosen dtype: fp64 is the yardstick, fp32
the floor.  test_whisper_cpu.py pins it against `transformers` (WhisperFeatureExtractor, WhisperForConditionalGeneration).  `mut`
names deliberate mistakes (MUTATIONS): test_whisper_cpu.py checks that each moves the teacher-forced logits far outside the GPU bound."""
import math

import torch
import torch.nn.functional as F

N_FFT, HOP = 400, 160
STOP_EOS, STOP_MAX_NEW, STOP_MAX_TARGET = 1, 2, 3
MUTATIONS = ("k_bias", "q_unscaled", "post_norm", "tanh_gelu", "no_decoder_positions", "conv2_shifted", "natural_log", "no_clamp",
             "drop_first_frame", "cross_before_final_norm", "no_causal_mask", "begin_suppress_always")


def logmel(wav, P, mel, dtype, mut=(), stft_complex64=False):
    """(2 P, n_mels): wav 1-D at 16 kHz, at most 320 P samples; mel (n_mels, 201).  `stft_complex64` rounds the STFT to complex64
    before the power is taken, as transformers.audio_utils.spectrogram stores it between its fp64 FFT and its fp64 power: the one
    step in which WhisperFeatureExtractor differs from this definition (test_whisper_cpu.py compares with it on and off)."""
    chunk = 320 * P
    assert wav.numel() <= chunk
    x = torch.zeros(chunk, dtype=dtype)
    x[:wav.numel()] = wav.to(dtype)
    win = torch.hann_window(N_FFT, periodic=True, dtype=dtype)
    st = torch.stft(x, N_FFT, HOP, window=win, center=True, pad_mode="reflect", return_complex=True)  # (201, 2 P + 1)
    if stft_complex64:
        st = st.to(torch.complex64).to(torch.complex128)
    pw = st.real ** 2 + st.imag ** 2
    pw = pw[:, 1:] if "drop_first_frame" in mut else pw[:, :-1]
    m = (mel.to(dtype) @ pw).clamp(min=1e-10)
    lg = m.log() if "natural_log" in mut else m.log10()
    if "no_clamp" not in mut:
        lg = torch.maximum(lg, lg.max() - 8.0)
    return ((lg + 4.0) / 4.0).T.contiguous()


def _gelu(x, mut):
    return F.gelu(x, approximate="tanh" if "tanh_gelu" in mut else "none")


def _ln(x, sd, name):
    return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"], sd[name + ".bias"], 1e-5)


def _attn(sd, name, xq, xkv, heads, mut, causal=False):
    d = xq.shape[-1]
    hd = d // heads
    q = F.linear(xq, sd[name + ".q_proj.weight"], sd[name + ".q_proj.bias"])
    k = F.linear(xkv, sd[name + ".k_proj.weight"])
    v = F.linear(xkv, sd[name + ".v_proj.weight"], sd[name + ".v_proj.bias"])
    if "k_bias" in mut:
        # how a bias lands on k in an engine that stacks q | k | v into one GEMM: the checkpoint's two bias vectors (q, v) laid onto
        # the first two projections, so that k takes v's bias and v is left without one
        k = k + sd[name + ".v_proj.bias"]
        v = F.linear(xkv, sd[name + ".v_proj.weight"])
    if "k_bias_only" in mut:  # not in MUTATIONS: a bias added to k and nothing else, which softmax cannot see (q . b is the same for every key)
        k = k + sd[name + ".v_proj.bias"]
    if "q_unscaled" not in mut:
        q = q * hd ** -0.5
    Tq, Tk = xq.shape[0], xkv.shape[0]
    q, k, v = q.view(Tq, heads, hd).transpose(0, 1), k.view(Tk, heads, hd).transpose(0, 1), v.view(Tk, heads, hd).transpose(0, 1)
    s = q @ k.transpose(1, 2)
    if causal and "no_causal_mask" not in mut:
        s = s + torch.full((Tq, Tk), float("-inf"), dtype=s.dtype).triu(1)
    o = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(Tq, d)
    return F.linear(o, sd[name + ".out_proj.weight"], sd[name + ".out_proj.bias"])


def _block(sd, pre, x, heads, mut, mem=None):
    """One layer: self-attention (causal with `mem`), cross-attention over `mem`, FFN; pre-norm unless mutated."""
    post = "post_norm" in mut

    def sub(x, norm, fn):
        return _ln(x + fn(x), sd, norm) if post else x + fn(_ln(x, sd, norm))

    x = sub(x, pre + "self_attn_layer_norm", lambda h: _attn(sd, pre + "self_attn", h, h, heads, mut, causal=mem is not None))
    if mem is not None:
        x = sub(x, pre + "encoder_attn_layer_norm", lambda h: _attn(sd, pre + "encoder_attn", h, mem, heads, mut))
    return sub(x, pre + "final_layer_norm", lambda h: F.linear(_gelu(F.linear(h, sd[pre + "fc1.weight"], sd[pre + "fc1.bias"]), mut),
                                                               sd[pre + "fc2.weight"], sd[pre + "fc2.bias"]))


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def encode(sd, cfg, wav, mel, dtype, mut=()):
    """Every tap of one utterance: logmel, conv1, features, enc0 .. enc<L>, encoder (and `pre_norm`, the last residual stream)."""
    sd = cast(sd, dtype)
    P = int(cfg.max_source_positions)
    out = {"logmel": logmel(wav, P, mel, dtype, mut)}
    x = out["logmel"].T.unsqueeze(0)
    x = _gelu(F.conv1d(x, sd["model.encoder.conv1.weight"], sd["model.encoder.conv1.bias"], padding=1), mut)
    out["conv1"] = x[0].T.contiguous()
    if "conv2_shifted" in mut:  # the window one frame late: padding (0, 2) instead of (1, 1)
        x = F.conv1d(F.pad(x, (0, 2)), sd["model.encoder.conv2.weight"], sd["model.encoder.conv2.bias"], stride=2)
    else:
        x = F.conv1d(x, sd["model.encoder.conv2.weight"], sd["model.encoder.conv2.bias"], stride=2, padding=1)
    x = _gelu(x, mut)[0].T.contiguous()
    out["features"] = x
    x = x + sd["model.encoder.embed_positions.weight"]
    out["enc0"] = x
    for l in range(int(cfg.encoder_layers)):
        x = _block(sd, f"model.encoder.layers.{l}.", x, int(cfg.encoder_attention_heads), mut)
        out[f"enc{l + 1}"] = x
    out["pre_norm"] = x
    out["encoder"] = _ln(x, sd, "model.encoder.layer_norm")
    return out


def decode_logits(sd, cfg, enc, ids, dtype, mut=()):
    """(len(ids), vocab): the raw logits of every position of the decoder input `ids`; `enc` is encode()'s result."""
    sd = cast(sd, dtype)
    mem = (enc["pre_norm"] if "cross_before_final_norm" in mut else enc["encoder"]).to(dtype)
    ids = torch.as_tensor(ids, dtype=torch.long)
    x = sd["model.decoder.embed_tokens.weight"][ids]
    if "no_decoder_positions" not in mut:
        x = x + sd["model.decoder.embed_positions.weight"][:len(ids)]
    for l in range(int(cfg.decoder_layers)):
        x = _block(sd, f"model.decoder.layers.{l}.", x, int(cfg.decoder_attention_heads), mut, mem=mem)
    x = _ln(x, sd, "model.decoder.layer_norm")
    return F.linear(x, sd["proj_out.weight"] if "proj_out.weight" in sd else sd["model.decoder.embed_tokens.weight"])


def process_row(row, g, suppress, begin_suppress, mut=()):
    """The row greedy step g reads: suppress_tokens at -inf, at g = 0 (or always, mutated) begin_suppress_tokens too."""
    row = row.clone()
    if len(suppress):
        row[list(suppress)] = float("-inf")
    if len(begin_suppress) and (g == 0 or "begin_suppress_always" in mut):
        row[list(begin_suppress)] = float("-inf")
    return row


def step_outputs(raw_row, g, suppress, begin_suppress, forced=None, mut=()):
    """(token, log-probability in fp64, top-two margin of the processed row): the argmax takes the lowest index on ties."""
    row = process_row(raw_row.double(), g, suppress, begin_suppress, mut)
    top = float(row.max())
    tok = int((row == top).nonzero()[0]) if forced is None else int(forced)
    lse = top + math.log(float(torch.exp(row - top).sum()))
    two = row.topk(2).values
    return tok, float(row[tok]) - lse, float(two[0] - two[1])


def greedy(sd, cfg, enc, prompt, max_new, suppress, begin_suppress, eos, dtype, mut=()):
    """Greedy generation of one utterance -> dict(tokens, logprobs, stop, logits (count, vocab) raw rows, margins)."""
    Tt = int(cfg.max_target_positions)
    assert 1 <= len(prompt) < Tt and max_new >= 1
    ids, toks, lps, rows, margins = list(prompt), [], [], [], []
    while True:
        raw = decode_logits(sd, cfg, enc, ids, dtype, mut)[-1]
        g = len(toks)
        tok, lp, margin = step_outputs(raw, g, suppress, begin_suppress, mut=mut)
        toks.append(tok); lps.append(lp); rows.append(raw); margins.append(margin)
        ids.append(tok)
        if tok == eos:
            stop = STOP_EOS
        elif len(toks) >= max_new:
            stop = STOP_MAX_NEW
        elif len(ids) >= Tt:
            stop = STOP_MAX_TARGET
        else:
            continue
        return dict(tokens=toks, logprobs=lps, stop=stop, logits=torch.stack(rows), margins=margins)


def forced_logits(sd, cfg, enc, prompt, tokens, dtype, mut=()):
    """(len(tokens), vocab): the raw rows teacher forcing reads, i.e. positions len(prompt) - 1 .. of the input prompt + tokens[:-1]."""
    ids = list(prompt) + list(tokens[:-1])
    return decode_logits(sd, cfg, enc, ids, dtype, mut)[len(prompt) - 1:]


def forced_logprobs(raw_rows, tokens, suppress, begin_suppress, mut=()):
    return [step_outputs(raw_rows[g], g, suppress, begin_suppress, forced=t, mut=mut)[1] for g, t in enumerate(tokens)]
