"""Test-side restatement of the EnCodec-24 kHz encoder (waveform -> codec tokens) in plain torch, run in fp64 as the yardstick
of the HIP encoder (tests/test_gpu_codec_enc.py) and pinned against `transformers.EncodecModel.encode` in
tests/test_codec_enc_cpu.py, plus the weight / codebook / waveform generator and the margin rule those tests share.  The
decoder's half (tolerance rule, weight-norm layouts, LSTM) is imported from tests/encodec_ref.py.

The steps (time runs along the last axis here, (C, L) per utterance; encoder ratios are the decoder's reversed):
  1. causal conv 1 -> filters, k = 7
  2. per ratio r: residual block shortcut_1x1(x) + conv_k1(ELU(conv_k3(ELU(x)))), ELU, strided conv k = 2r / stride r, c -> 2c
  3. LSTM (layers stacked), output + input
  4. ELU, causal conv -> hidden, k = 7
  5. residual vector quantiser: per stage argmin_j |r - e_j|^2 (first index on ties), r -= e_idx
Every convolution pads k - stride on the left and `extra` on the right, both reflect, `extra` bringing the output to
ceil(L / stride) samples; an input not longer than the larger pad is zero-extended on the right first and the extension removed
afterwards.

`variant` selects deliberately wrong restatements: the CPU tests use them to show that the test inputs tell them apart."""
import functools
import math
import os
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

import encodec_ref as R
from encodec_ref import FULL, NARROW, TOL_FACTOR, CodecGeometry  # noqa: F401  (re-exported for the tests)

# Lengths (samples) of the whole-encoder GPU tests: 1, 2, 7, 225 (3 s) and 753 frames.
GPU_LENGTHS = (1, 321, 2240, 72000, 240960)


def enc_ratios(geo: CodecGeometry):
    return tuple(reversed(geo.ratios))


def enc_layer_index(geo: CodecGeometry):
    """Indices in `encoder.layers` of the local EncodecModel: conv 0, per stage [resblock, ELU, strided conv], lstm, ELU, conv."""
    n = len(geo.ratios)
    res = [1 + 3 * s for s in range(n)]
    down = [3 + 3 * s for s in range(n)]
    return res, down, 1 + 3 * n, 3 + 3 * n


def n_frames(geo: CodecGeometry, L: int) -> int:
    return -(-L // geo.hop)


def enc_expected_shapes(geo: CodecGeometry) -> Dict[str, Tuple[int, ...]]:
    """Key -> shape of the encoder's weight-norm-free layout (plain `.weight`)."""
    res, down, li, last = enc_layer_index(geo)
    c = geo.filters
    s = {"encoder.layers.0.conv.weight": (c, 1, geo.kernel), "encoder.layers.0.conv.bias": (c,)}
    for i, r in enumerate(enc_ratios(geo)):
        p = f"encoder.layers.{res[i]}."
        s[p + "block.1.conv.weight"] = (c // 2, c, geo.res_kernel)
        s[p + "block.1.conv.bias"] = (c // 2,)
        s[p + "block.3.conv.weight"] = (c, c // 2, 1)
        s[p + "block.3.conv.bias"] = (c,)
        s[p + "shortcut.conv.weight"] = (c, c, 1)
        s[p + "shortcut.conv.bias"] = (c,)
        s[f"encoder.layers.{down[i]}.conv.weight"] = (2 * c, c, 2 * r)
        s[f"encoder.layers.{down[i]}.conv.bias"] = (2 * c,)
        c *= 2
    for l in range(geo.lstm_layers):
        s[f"encoder.layers.{li}.lstm.weight_ih_l{l}"] = (4 * c, c)
        s[f"encoder.layers.{li}.lstm.weight_hh_l{l}"] = (4 * c, c)
        s[f"encoder.layers.{li}.lstm.bias_ih_l{l}"] = (4 * c,)
        s[f"encoder.layers.{li}.lstm.bias_hh_l{l}"] = (4 * c,)
    s[f"encoder.layers.{last}.conv.weight"] = (geo.hidden, c, geo.last_kernel)
    s[f"encoder.layers.{last}.conv.bias"] = (geo.hidden,)
    return s


def codec_expected_shapes(geo: CodecGeometry) -> Dict[str, Tuple[int, ...]]:
    """Both halves, in the order codec.expected_keys(cfg, encoder=True) lists them: decoder, codebooks, encoder."""
    s = dict(R.expected_shapes(geo))
    s.update(enc_expected_shapes(geo))
    return s


def make_wave(L: int, seed: int) -> torch.Tensor:
    """(1, 1, L) fp32 test waveform: white noise (so that neighbouring frames differ in every channel and the codes spread over
    the codebooks) under a slow amplitude envelope plus a weak tone, peak below 1."""
    g = torch.Generator().manual_seed(7727 * seed + 13)
    t = torch.arange(L, dtype=torch.float64)
    env = 0.55 + 0.35 * torch.sin(t * (2 * math.pi / 9000.0) + seed)
    x = 0.22 * env * torch.randn(L, generator=g, dtype=torch.float64) + 0.08 * torch.sin(t * 0.031 + 0.5 * seed)
    return x.clamp(-0.99, 0.99).float()[None, None]


# Gains of the generator.  The model's default initialisation gives an embedding far below unit codebooks (every frame the same
# code) and the decoder generator's gains (1.6 / sqrt(fan), LSTM 2 / sqrt(in)) saturate it (a changed sample changes no code).
# Here the convolutions roughly preserve the variance through ELU (gain 1.25), the first convolution lifts the +-0.3 waveform to
# unit scale, the LSTM stays out of saturation (1 / sqrt(in)), and the codebooks are drawn at the scale the embedding has on a
# calibration signal: stage 0 around the embedding's per-channel mean with its per-channel spread, stage q > 0 zero-mean at
# RES_DECAY^q of it (a 1024-entry codebook in 128 dimensions removes about 5 % of the residual's norm per stage, so the later
# codebooks stay at the residual's scale and every stage spreads over its codebook).
CONV_GAIN = 1.25
FIRST_GAIN = 6.0
LSTM_GAIN = 1.0
RES_DECAY = 0.95
CALIBRATION_SAMPLES = 48000


@functools.lru_cache(maxsize=None)
def make_enc_weights(geo: CodecGeometry, seed: int) -> Dict[str, torch.Tensor]:
    """(Cached: callers must not modify the tensors.)  Deterministic fp32 weights of BOTH halves in the weight-norm-free layout: the decoder's from encodec_ref.make_weights,
    the encoder's and the codebooks from here (the codebooks replace the decoder generator's)."""
    g = torch.Generator().manual_seed(seed * 9176 + 11)
    out = dict(R.make_weights(geo, seed))
    for k, shp in enc_expected_shapes(geo).items():
        if ".lstm.weight" in k:
            w = torch.randn(shp, generator=g, dtype=torch.float64) * (LSTM_GAIN / shp[1] ** 0.5)
        elif k.endswith("bias") or ".lstm.bias" in k:
            w = torch.randn(shp, generator=g, dtype=torch.float64) * 0.1
        else:
            gain = FIRST_GAIN if k == "encoder.layers.0.conv.weight" else CONV_GAIN
            w = torch.randn(shp, generator=g, dtype=torch.float64) * (gain / (shp[1] * shp[2]) ** 0.5)
        out[k] = w.float()
    emb = encode_embeddings(out, geo, make_wave(CALIBRATION_SAMPLES, 1000 + seed))  # (hidden, T) fp64
    mu, sd = emb.mean(dim=1), emb.std(dim=1)
    for q in range(geo.n_codebooks):
        e = torch.randn(geo.codebook_size, geo.hidden, generator=g, dtype=torch.float64) * sd * RES_DECAY ** q
        out[f"quantizer.layers.{q}.codebook.embed"] = ((e + mu) if q == 0 else e).float()
    return out


def enc_conv(x, w, b, stride=1, variant=""):
    """x (C, L), w (O, C, k) -> (O, ceil(L / stride)): EncodecConv1d.forward for the causal model."""
    k = w.shape[-1]
    L = x.shape[-1]
    left = k - stride
    n_out = L // stride if "floor_frames" in variant else -(-L // stride)
    extra = max(0, n_out * stride - L)
    if n_out == 0:
        return x.new_zeros(w.shape[0], 0)
    if f"drop_tap_k{k}" in variant:
        w = w.clone()
        w[:, :, 1] = 0
    zl, zr = "zero_left" in variant, "zero_right" in variant
    ext = max(0, max(left, extra) - L + 1)  # zero extension of a short input, removed again below
    xe = F.pad(x[None], (0, ext))
    xp = F.pad(xe, (0 if zl else left, 0 if zr else extra), mode="reflect") if (left or extra) else xe
    xp = xp[..., : xp.shape[-1] - ext]
    if zl or zr:
        xp = F.pad(xp, (left if zl else 0, extra if zr else 0))
    return F.conv1d(xp, w, b, stride=stride)[0]


def encode_embeddings(sd, geo: CodecGeometry, wav: torch.Tensor, dtype=torch.float64, variant: str = "", taps=None) -> torch.Tensor:
    """wav (1, 1, L) or (L,) -> (hidden, T) of `dtype`, T = ceil(L / hop).  `sd`: either accepted key layout.  `taps` (optional
    dict) receives the time-major (rows, C) intermediates."""
    P = R.fold_weight_norm({k: v for k, v in sd.items() if k.startswith("encoder.")}, dtype)
    res, down, li, last = enc_layer_index(geo)
    x = wav.reshape(1, -1).to(dtype)
    x = enc_conv(x, P["encoder.layers.0.conv.weight"], P["encoder.layers.0.conv.bias"], 1, variant)
    if taps is not None:
        taps["conv0"] = x.T.clone()
    for i, r in enumerate(enc_ratios(geo)):
        p = f"encoder.layers.{res[i]}."
        h = enc_conv(F.elu(x), P[p + "block.1.conv.weight"], P[p + "block.1.conv.bias"], 1, variant)
        h = enc_conv(F.elu(h), P[p + "block.3.conv.weight"], P[p + "block.3.conv.bias"])
        x = enc_conv(x, P[p + "shortcut.conv.weight"], P[p + "shortcut.conv.bias"]) + h
        x = enc_conv(F.elu(x), P[f"encoder.layers.{down[i]}.conv.weight"], P[f"encoder.layers.{down[i]}.conv.bias"], r, variant)
        if taps is not None:
            taps[f"stage{i}"] = x.T.clone()
    if x.shape[-1] == 0:
        return x.new_zeros(geo.hidden, 0)
    y = R.lstm(x.T, P, f"encoder.layers.{li}.lstm.", geo.lstm_layers).T
    x = y if "no_skip" in variant else y + x
    if taps is not None:
        taps["lstm"] = x.T.clone()
    return enc_conv(F.elu(x), P[f"encoder.layers.{last}.conv.weight"], P[f"encoder.layers.{last}.conv.bias"], 1, variant)


def codebooks(sd, geo: CodecGeometry, n_q: int, dtype=torch.float64):
    return [sd[f"quantizer.layers.{q}.codebook.embed"].to(dtype) for q in range(n_q)]


def rvq_encode(cbs, emb: torch.Tensor, variant: str = "") -> torch.Tensor:
    """emb (T, D), cbs: list of (S, D) -> codes (n_q, T) int64, as EncodecResidualVectorQuantizer.encode: the index is
    `max(-(|r|^2 - 2 r e^T + |e|^2))`, i.e. the first index of the smallest distance."""
    r = emb.clone()
    out = []
    for cb in cbs:
        d = r.pow(2).sum(1, keepdim=True) - 2 * r @ cb.T + cb.pow(2).sum(1)[None]
        if "last_index" in variant:
            idx = d.shape[1] - 1 - d.flip(1).min(dim=1).indices
        else:
            idx = (-d).max(dim=1).indices
        out.append(idx)
        if "no_residual" not in variant:
            r = r - cb[idx]
    return torch.stack(out)


def encode(sd, geo: CodecGeometry, wav, n_q: int = 8, dtype=torch.float64, variant: str = "") -> torch.Tensor:
    """wav -> codes (n_q, T) int64."""
    emb = encode_embeddings(sd, geo, wav, dtype, variant)
    return rvq_encode(codebooks(sd, geo, n_q, dtype), emb.T.contiguous(), variant)


def embedding_floor(sd, geo, wav) -> Tuple[torch.Tensor, float, float]:
    """(fp64 embedding (T, D), fp32 floor, scale): the floor is max|fp32 restatement - fp64 restatement| on the CPU."""
    ref = encode_embeddings(sd, geo, wav, torch.float64).T.contiguous()
    f32 = encode_embeddings(sd, geo, wav, torch.float32).T
    return ref, float((f32.double() - ref).abs().max()), float(ref.abs().max())


def decided(cbs, emb64: torch.Tensor, tol: float):
    """The margin rule, teacher-forced per stage from the fp64 residual.  Returns (codes (n_q, T), decided (n_q, T) bool): stage q
    of a frame is decided when the fp64 gap between its best and second-best squared distance exceeds what a per-element error
    of `tol` in the embedding, accumulated over the q stages before it (each subtracts a codebook row, exact up to one rounding
    of an element that carries the error), can change it by:  |d_a(r + delta) - d_b(r + delta) - (d_a(r) - d_b(r))| =
    2 |delta . (e_b - e_a)| <= 2 |delta|_inf |e_a - e_b|_1 with |delta|_inf <= (q + 1) tol."""
    r = emb64.clone()
    codes, dec = [], []
    for q, cb in enumerate(cbs):
        d = r.pow(2).sum(1, keepdim=True) - 2 * r @ cb.T + cb.pow(2).sum(1)[None]
        s, ix = d.topk(2, dim=1, largest=False, sorted=True)
        first = (-d).max(dim=1).indices
        bound = 2 * tol * (q + 1) * (cb[ix[:, 0]] - cb[ix[:, 1]]).abs().sum(1)
        codes.append(first)
        dec.append((s[:, 1] - s[:, 0]) > bound)
        r = r - cb[first]
    return torch.stack(codes), torch.stack(dec)


def compare_codes(got: torch.Tensor, want: torch.Tensor, dec: torch.Tensor):
    """got / want / dec (n_q, T).  A (stage, frame) is held to exact equality when it is decided and every earlier stage of the
    frame agrees (after a differing earlier stage the residuals differ and the comparison has no meaning).  Returns
    (wrong: count of held entries that differ, held share per stage, differing-but-undecided count)."""
    agree = torch.ones_like(dec[0])
    wrong, held, loose = 0, [], 0
    for q in range(got.shape[0]):
        h = dec[q] & agree
        wrong += int((h & (got[q] != want[q])).sum())
        loose += int((~dec[q] & agree & (got[q] != want[q])).sum())
        held.append(float(h.double().mean()))
        agree = agree & (got[q] == want[q])
    return wrong, held, loose


# ---- committed fixtures (tests/golden/codec/enc_full.npz, enc_narrow.npz): waveforms, fp64 embeddings, codes and the seeds ----------
FIXTURE_LENGTHS = (1, 319, 320, 321, 2240, 24001)
FIXTURE_WEIGHT_SEED = 3


def write_fixtures(directory: str):
    import numpy as np

    for name, geo in (("enc_full", FULL), ("enc_narrow", NARROW)):
        sd = make_enc_weights(geo, FIXTURE_WEIGHT_SEED)
        z = {"weight_seed": np.int64(FIXTURE_WEIGHT_SEED), "wave_seeds": np.array([10 + i for i in range(len(FIXTURE_LENGTHS))])}
        for i, L in enumerate(FIXTURE_LENGTHS):
            wav = make_wave(L, 10 + i)
            emb = encode_embeddings(sd, geo, wav)
            z[f"wav_{L}"] = wav.numpy()
            z[f"emb_{L}"] = emb.numpy()
            z[f"codes_{L}"] = rvq_encode(codebooks(sd, geo, 8), emb.T.contiguous()).numpy()
        np.savez_compressed(os.path.join(directory, name + ".npz"), **z)


if __name__ == "__main__":
    write_fixtures(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codec"))
