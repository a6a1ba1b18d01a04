"""Test-side restatement of the EnCodec-24 kHz decoder (codes -> waveform) in plain torch, run in fp64 as the yardstick
of the HIP decoder (tests/test_gpu_codec.py) and pinned against `transformers.EncodecModel.decode` in tests/test_codec_cpu.py,
plus the deterministic weight generator and the tolerance rule those tests share.

The five steps (time runs along the last axis here, (C, L) per utterance):
  1. RVQ decode: sum over q of codebook_q[codes[q, t]]
  2. causal conv hidden -> 16 * filters, k = 7
  3. LSTM (layers stacked), output + input
  4. per ratio r: ELU, transposed conv k = 2r / stride r with the r rightmost samples trimmed, then the residual block
     shortcut_1x1(x) + conv_k1(ELU(conv_k3(ELU(x))))
  5. ELU, causal conv -> 1, k = 7
Every stride-1 convolution pads k - 1 on the left in reflect mode; an input not longer than the pad is zero-extended on the
right first and the extension removed afterwards.

`variant` selects deliberately wrong restatements: the CPU tests use them to show that the test inputs tell them apart."""
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

# The engine may differ from the fp64 restatement by TOL_FACTOR x the fp32 floor, where the floor is the max-abs difference
# of THIS restatement run in torch fp32 on the CPU against fp64 on the same inputs, both relative to the waveform's max-abs.
# fp32 dot products of up to 1024 terms rounded once per product and a 1505-step recurrence summed in another order justify a
# small multiple of that floor, not more.
TOL_FACTOR = 4.0


@dataclass(frozen=True)
class CodecGeometry:
    hidden: int = 128          # codebook_dim = decoder input channels
    filters: int = 32
    ratios: Tuple[int, ...] = (8, 5, 4, 2)
    kernel: int = 7
    last_kernel: int = 7
    res_kernel: int = 3
    lstm_layers: int = 2
    codebook_size: int = 1024
    n_codebooks: int = 8

    @property
    def width(self):  # channels of the LSTM and of the first up-sampling stage
        return self.filters * 2 ** len(self.ratios)

    @property
    def hop(self):
        h = 1
        for r in self.ratios:
            h *= r
        return h


FULL = CodecGeometry()
NARROW = CodecGeometry(hidden=16, filters=4, codebook_size=64)


def layer_index(geo: CodecGeometry):
    """Indices in `decoder.layers` of the local EncodecModel: conv 0, lstm 1, per stage [ELU, convT, resblock], ELU, conv."""
    up = [3 + 3 * s for s in range(len(geo.ratios))]
    res = [4 + 3 * s for s in range(len(geo.ratios))]
    return up, res, 3 + 3 * len(geo.ratios)


def expected_shapes(geo: CodecGeometry) -> Dict[str, Tuple[int, ...]]:
    """Key -> shape of the weight-norm-free layout (plain `.weight`)."""
    up, res, last = layer_index(geo)
    W = geo.width
    s = {"decoder.layers.0.conv.weight": (W, geo.hidden, geo.kernel), "decoder.layers.0.conv.bias": (W,)}
    for l in range(geo.lstm_layers):
        s[f"decoder.layers.1.lstm.weight_ih_l{l}"] = (4 * W, W)
        s[f"decoder.layers.1.lstm.weight_hh_l{l}"] = (4 * W, W)
        s[f"decoder.layers.1.lstm.bias_ih_l{l}"] = (4 * W,)
        s[f"decoder.layers.1.lstm.bias_hh_l{l}"] = (4 * W,)
    c = W
    for i, r in enumerate(geo.ratios):
        s[f"decoder.layers.{up[i]}.conv.weight"] = (c, c // 2, 2 * r)
        s[f"decoder.layers.{up[i]}.conv.bias"] = (c // 2,)
        c //= 2
        p = f"decoder.layers.{res[i]}."
        s[p + "block.1.conv.weight"] = (c // 2, c, geo.res_kernel)
        s[p + "block.1.conv.bias"] = (c // 2,)
        s[p + "block.3.conv.weight"] = (c, c // 2, 1)
        s[p + "block.3.conv.bias"] = (c,)
        s[p + "shortcut.conv.weight"] = (c, c, 1)
        s[p + "shortcut.conv.bias"] = (c,)
    s[f"decoder.layers.{last}.conv.weight"] = (1, c, geo.last_kernel)
    s[f"decoder.layers.{last}.conv.bias"] = (1,)
    for q in range(geo.n_codebooks):
        s[f"quantizer.layers.{q}.codebook.embed"] = (geo.codebook_size, geo.hidden)
    return s


def make_weights(geo: CodecGeometry, seed: int) -> Dict[str, torch.Tensor]:
    """Deterministic fp32 weights in the weight-norm-free layout.  Gains are above the variance-preserving ones so that the
    waveform depends on every code and on the padding rule far from the start (the model's default initialisation gives an
    almost constant output: a poor test signal)."""
    g = torch.Generator().manual_seed(seed)
    ups = layer_index(geo)[0]
    out = {}
    for k, shp in expected_shapes(geo).items():
        if k.endswith("codebook.embed"):
            w = torch.randn(shp, generator=g, dtype=torch.float64)
        elif ".lstm.weight" in k:
            w = torch.randn(shp, generator=g, dtype=torch.float64) * (2.0 / shp[1] ** 0.5)
        elif k.endswith("bias") or ".lstm.bias" in k:
            w = torch.randn(shp, generator=g, dtype=torch.float64) * 0.1
        else:
            # conv (out, in, k): fan-in in*k; transposed conv (in, out, k): every output sample has two taps -> fan-in 2*in
            fan = 2 * shp[0] if int(k.split(".")[2]) in ups else shp[1] * shp[2]
            w = torch.randn(shp, generator=g, dtype=torch.float64) * (1.6 / fan ** 0.5)
        out[k] = w.float()
    return out


def make_codes(geo: CodecGeometry, n_q: int, T: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * T + n_q)
    return torch.randint(0, geo.codebook_size, (n_q, T), generator=g, dtype=torch.int64)


def to_weight_norm_layout(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The same weights under the parametrised names of the local EncodecModel: original0 = g = |v| over all but dim 0,
    original1 = v (scaled by a per-channel factor so that folding has something to do)."""
    out = {}
    for k, v in sd.items():
        if k.endswith(".conv.weight"):
            base = k[: -len("weight")] + "parametrizations.weight."
            n = v.double().flatten(1).norm(dim=1).reshape(-1, 1, 1)
            scale = (1.0 + 0.25 * torch.arange(v.shape[0], dtype=torch.float64).reshape(-1, 1, 1) / max(1, v.shape[0]))
            out[base + "original0"] = n.to(v.dtype)
            out[base + "original1"] = (v.double() * scale).to(v.dtype)
        else:
            out[k] = v
    return out


def fold_weight_norm(sd: Dict[str, torch.Tensor], dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """Either accepted layout -> plain `.weight` tensors of `dtype` (w = g * v / |v|, norm over all dims but 0)."""
    out = {}
    for k, v in sd.items():
        if k.endswith("parametrizations.weight.original1"):
            base = k[: -len("parametrizations.weight.original1")]
            g = sd[base + "parametrizations.weight.original0"].to(dtype)
            vv = v.to(dtype)
            out[base + "weight"] = g * vv / vv.flatten(1).norm(dim=1).reshape(-1, 1, 1)
        elif k.endswith("parametrizations.weight.original0"):
            continue
        else:
            out[k] = v.to(dtype)
    return out


def causal_conv(x, w, b, variant=""):
    """x (C, L), w (O, C, k): left pad k - 1, reflect (zero-extended when L <= pad)."""
    k = w.shape[-1]
    pad = k - 1
    L = x.shape[-1]
    if pad == 0:
        return F.conv1d(x[None], w, b)[0]
    if "zero_pad" in variant:
        xp = F.pad(x[None], (pad, 0))
    else:
        extra = max(0, pad - L + 1)
        xp = F.pad(F.pad(x[None], (0, extra)), (pad, 0), mode="reflect")
        xp = xp[..., : xp.shape[-1] - extra]
    if f"drop_tap_k{k}" in variant:
        w = w.clone()
        w[:, :, 1] = 0
    return F.conv1d(xp, w, b)[0]


def up_conv(x, w, b, stride, variant=""):
    y = F.conv_transpose1d(x[None], w, b, stride=stride)[0]
    trim = w.shape[-1] - stride
    return y[..., trim:] if "trim_left" in variant else y[..., : y.shape[-1] - trim]


def lstm(x, P, prefix, layers):
    """x (L, W) -> (L, W): torch's gate order i, f, g, o; zero initial state."""
    for l in range(layers):
        wi, wh = P[f"{prefix}weight_ih_l{l}"], P[f"{prefix}weight_hh_l{l}"]
        gin = x @ wi.T + P[f"{prefix}bias_ih_l{l}"] + P[f"{prefix}bias_hh_l{l}"]
        H = wh.shape[1]
        h = x.new_zeros(H)
        c = x.new_zeros(H)
        ys = []
        for t in range(x.shape[0]):
            a = gin[t] + wh @ h
            i, f, g, o = a[:H].sigmoid(), a[H:2 * H].sigmoid(), a[2 * H:3 * H].tanh(), a[3 * H:].sigmoid()
            c = f * c + i * g
            h = o * c.tanh()
            ys.append(h)
        x = torch.stack(ys)
    return x


def decode(sd, geo: CodecGeometry, codes: torch.Tensor, dtype=torch.float64, variant: str = "", taps=None) -> torch.Tensor:
    """codes (n_q, T) int64 -> (1, 1, hop * T) of `dtype`.  `sd`: either accepted key layout.  `taps` (optional dict) receives
    the time-major (rows, C) intermediates the op-level GPU tests compare."""
    P = fold_weight_norm(sd, dtype)
    up, res, last = layer_index(geo)
    n_q, T = codes.shape
    x = sum(P[f"quantizer.layers.{q}.codebook.embed"][codes[q]] for q in range(n_q)).T  # (hidden, T)
    x = causal_conv(x, P["decoder.layers.0.conv.weight"], P["decoder.layers.0.conv.bias"], variant)
    y = lstm(x.T, P, "decoder.layers.1.lstm.", geo.lstm_layers).T
    x = y if "no_skip" in variant else y + x
    if taps is not None:
        taps["lstm"] = x.T.clone()
    for i, r in enumerate(geo.ratios):
        x = up_conv(F.elu(x), P[f"decoder.layers.{up[i]}.conv.weight"], P[f"decoder.layers.{up[i]}.conv.bias"], r, variant)
        p = f"decoder.layers.{res[i]}."
        h = causal_conv(F.elu(x), P[p + "block.1.conv.weight"], P[p + "block.1.conv.bias"], variant)
        h = causal_conv(F.elu(h), P[p + "block.3.conv.weight"], P[p + "block.3.conv.bias"])
        x = causal_conv(x, P[p + "shortcut.conv.weight"], P[p + "shortcut.conv.bias"]) + h
        if taps is not None:
            taps[f"stage{i}"] = x.T.clone()
    x = causal_conv(F.elu(x), P[f"decoder.layers.{last}.conv.weight"], P[f"decoder.layers.{last}.conv.bias"], variant)
    return x[None]


def floor_and_scale(sd, geo, codes) -> Tuple[torch.Tensor, float, float]:
    """(fp64 waveform, fp32 floor, output scale): the floor is max|decode_fp32 - decode_fp64| on the CPU."""
    ref = decode(sd, geo, codes, torch.float64)
    f32 = decode(sd, geo, codes, torch.float32)
    return ref, float((f32.double() - ref).abs().max()), float(ref.abs().max())


def tolerance(floor: float) -> float:
    return TOL_FACTOR * floor
