"""Test-side restatement of the HiFi-GAN / BigVGAN generator (log-mel frames -> waveform) as include/vallex.h defines it, in plain
torch and dtype-parametric: fp64 is the yardstick of the HIP generator (tests/test_gpu_ganvoc.py), fp32 on the host the floor.  The
leaky-ReLU mode is pinned against `transformers.SpeechT5HifiGan` in tests/test_ganvoc_cpu.py.  Also here: the deterministic weight
generator, the narrow test geometries, the tolerance rule and the deliberately wrong restatements (`variant`) that show the test
inputs tell a wrong pad, tap, crop, dilation, padding, scale or parameter apart.

Time runs along the last axis: x is (C, L) per utterance.  Weights use the canonical keys of vx_gan_set_weight (plain `weight`)."""
import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

TOL_FACTOR = 4  # engine error <= 4 x the fp32 floor, the project's rule

VARIANTS = ("zero_pad", "drop_tap", "crop_shift", "dilation_1", "p_off_by_one", "no_mean", "alpha_for_beta", "no_exp")

# The narrow geometries: the smallest shapes at which each piece can go wrong (dicts as GanVocoder takes them).
#  1: channels 24 / 12 / 6 (no multiple of 16: the scalar gather), snakebeta with log-scale parameters
#  2: channels 64 / 32 / 16 (float4 gather at 64 and 32 and 16), k = 16 / u = 8 (three input rows reach an output group), dilation 5
#     with kernel 11 (pad 25), snake with linear parameters
#  3: leaky ReLU, k = 8 / u = 4
GEOMETRIES: Dict[str, dict] = {
    "g1_snakebeta": dict(n_mels=100, rates=(2, 2), kernels=(4, 4), initial_channels=24, resblock_kernels=(3, 7),
                         dilations=((1, 3), (1, 3)), activation="snakebeta", alpha_logscale=True, lrelu_slope=0.1),
    "g2_snake": dict(n_mels=100, rates=(8, 2), kernels=(16, 4), initial_channels=64, resblock_kernels=(3, 11),
                     dilations=((1, 3, 5), (1, 3, 5)), activation="snake", alpha_logscale=False, lrelu_slope=0.1),
    "g3_lrelu": dict(n_mels=100, rates=(4, 2), kernels=(8, 4), initial_channels=32, resblock_kernels=(3, 5),
                     dilations=((1, 3), (1, 3)), activation="lrelu", alpha_logscale=False, lrelu_slope=0.1),
}
# bigvgan_base_24khz_100band's channel widths (512 .. 32): every float4 gather and both MFMA tile shapes
BASE = dict(n_mels=100, rates=(8, 8, 2, 2), kernels=(16, 16, 4, 4), initial_channels=512, resblock_kernels=(3, 7, 11),
            dilations=((1, 3, 5), (1, 3, 5), (1, 3, 5)), activation="snakebeta", alpha_logscale=True, lrelu_slope=0.1)


def hop(cfg: dict) -> int:
    h = 1
    for u in cfg["rates"]:
        h *= u
    return h


def logmel(T: int, seed: int = 0, n_mels: int = 100) -> torch.Tensor:
    """(T, n_mels) float32 in the range of the filterbank's log-mel frames."""
    g = torch.Generator().manual_seed(1000 * seed + T)
    return (torch.randn((T, n_mels), generator=g) * 2.0 - 4.0).float()


# ---- the anti-aliased activation ------------------------------------------------------------------------------------------------
def kaiser_sinc_filter(cutoff: float = 0.25, half_width: float = 0.3, K: int = 12) -> torch.Tensor:
    """(K,) float64: the low-pass both the up and the down step use."""
    delta_f = 4 * half_width
    A = 2.285 * (K // 2 - 1) * math.pi * delta_f + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50.0 else (0.5842 * (A - 21.0) ** 0.4 + 0.07886 * (A - 21.0) if A >= 21.0 else 0.0)
    w = torch.kaiser_window(K, periodic=False, beta=beta, dtype=torch.float64)
    time = torch.arange(-(K // 2), K // 2, dtype=torch.float64) + 0.5
    f = 2 * cutoff * w * torch.sinc(2 * cutoff * time)
    return f / f.sum()


def snake(u: torch.Tensor, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """u (C, L); a, b (C,): u + sin(a u)^2 / (b + 1e-9)."""
    return u + torch.sin(u * a[:, None]) ** 2 / (b[:, None] + 1e-9)


def aa_act(x: torch.Tensor, f: torch.Tensor, a: Optional[torch.Tensor], b: Optional[torch.Tensor], variant: Optional[str] = None):
    """The composition the definition names: pad, conv_transpose1d, crop, act, pad, strided conv1d.  x (C, L) -> (C, L); a = None
    is the identity activation."""
    Cc, L = x.shape
    K = f.numel()
    assert K == 12
    mode = "constant" if variant == "zero_pad" else "replicate"
    if variant == "drop_tap":
        f = f.clone()
        f[K - 1] = 0.0  # a loop that ends one tap early
    w = f.to(x.dtype).reshape(1, 1, K).expand(Cc, 1, K)
    xp = F.pad(x[None], (5, 5), mode=mode)
    full = 2.0 * F.conv_transpose1d(xp, w, stride=2, groups=Cc)
    lo = 16 if variant == "crop_shift" else 15
    u = full[0, :, lo: lo + 2 * L]
    v = u if a is None else snake(u, a.to(x.dtype), b.to(x.dtype))
    vp = F.pad(v[None], (5, 6), mode=mode)
    return F.conv1d(vp, w, stride=2, groups=Cc)[0]


def aa_act_polyphase(x: torch.Tensor, f: torch.Tensor, a: Optional[torch.Tensor], b: Optional[torch.Tensor]):
    """The fused form the kernel uses: u[2m] = 2 sum_s f[2s+1] x[cl(m+2-s)], u[2m+1] = 2 sum_s f[2s] x[cl(m+3-s)];
    y[t] = sum_j f[j] v[clamp(2t + j - 5, 0, 2L-1)]."""
    Cc, L = x.shape
    f = f.to(x.dtype)
    m = torch.arange(L)
    u = torch.zeros((Cc, 2 * L), dtype=x.dtype)
    for s in range(6):
        u[:, 0::2] += f[2 * s + 1] * x[:, (m + 2 - s).clamp(0, L - 1)]
        u[:, 1::2] += f[2 * s] * x[:, (m + 3 - s).clamp(0, L - 1)]
    u = 2.0 * u
    v = u if a is None else snake(u, a.to(x.dtype), b.to(x.dtype))
    y = torch.zeros((Cc, L), dtype=x.dtype)
    for j in range(12):
        y += f[j] * v[:, (2 * m + j - 5).clamp(0, 2 * L - 1)]
    return y


# ---- the generator --------------------------------------------------------------------------------------------------------------
def _act_params(w, name, cfg, dtype, variant):
    al = w[name + ".alpha"].to(dtype)
    be = w[name + ".beta"].to(dtype) if cfg["activation"] == "snakebeta" and variant != "alpha_for_beta" else al
    if cfg["alpha_logscale"] and variant != "no_exp":
        al, be = torch.exp(al), torch.exp(be)
    return al, be


def conv_transpose(x, W, bias, u, k, variant=None):
    """out[co][n] = b[co] + sum x[ci][t] W[ci][co][j] over n = t u - p + j, p = (k - u) / 2; n in [0, L u)."""
    p = (k - u) // 2 + (1 if variant == "p_off_by_one" else 0)
    L = x.shape[-1]
    full = F.conv_transpose1d(x[None], W, None, stride=u)[0]  # n + p = t u + j
    full = F.pad(full, (0, 1))
    return full[:, p: p + L * u] + bias[:, None]


def pre_tanh(w: Dict[str, torch.Tensor], cfg: dict, mel: torch.Tensor, dtype=torch.float64, variant: Optional[str] = None,
             taps: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mel (T, n_mels) -> the signal in front of the tanh, (T * hop,)."""
    W = {k: v.to(dtype) for k, v in w.items()}
    f = (kaiser_sinc_filter() if taps is None else taps.double()).float().to(dtype)  # the engine's taps are rounded to fp32 once
    lrelu = cfg["activation"] == "lrelu"
    slope = cfg["lrelu_slope"]
    x = mel.to(dtype).t()
    if "mean" in W:
        x = (x - W["mean"][:, None]) / W["scale"][:, None]
    x = F.conv1d(x[None], W["conv_pre.weight"], W["conv_pre.bias"], padding=3)[0]
    R = len(cfg["resblock_kernels"])

    def act(h, name):
        if lrelu:
            return F.leaky_relu(h, slope)
        a, b = _act_params(w, name, cfg, dtype, variant)
        return aa_act(h, f, a, b, variant)

    for i, (u, k) in enumerate(zip(cfg["rates"], cfg["kernels"])):
        if lrelu:
            x = F.leaky_relu(x, slope)
        x = conv_transpose(x, W[f"ups.{i}.weight"], W[f"ups.{i}.bias"], u, k, variant)
        xs = None
        for r, rk in enumerate(cfg["resblock_kernels"]):
            n = i * R + r
            h = x
            for m, d in enumerate(cfg["dilations"][r]):
                dd = 1 if variant == "dilation_1" else d
                xt = act(h, f"resblocks.{n}.activations.{2 * m}")
                xt = F.conv1d(xt[None], W[f"resblocks.{n}.convs1.{m}.weight"], W[f"resblocks.{n}.convs1.{m}.bias"], dilation=dd,
                              padding=dd * (rk - 1) // 2)[0]
                xt = act(xt, f"resblocks.{n}.activations.{2 * m + 1}")
                xt = F.conv1d(xt[None], W[f"resblocks.{n}.convs2.{m}.weight"], W[f"resblocks.{n}.convs2.{m}.bias"],
                              padding=(rk - 1) // 2)[0]
                h = h + xt
            xs = h if xs is None else xs + h
        x = xs if variant == "no_mean" else xs / R
    x = F.leaky_relu(x, 0.01) if lrelu else act(x, "activation_post")
    return F.conv1d(x[None], W["conv_post.weight"], W.get("conv_post.bias"), padding=3)[0, 0]


def forward(w, cfg, mel, dtype=torch.float64, variant=None, taps=None) -> torch.Tensor:
    """mel (T, n_mels) -> wav (T * hop,) in `dtype`."""
    return torch.tanh(pre_tanh(w, cfg, mel, dtype, variant, taps))


def expected_shapes(cfg: dict, post_bias: bool = True) -> Dict[str, tuple]:
    C0 = cfg["initial_channels"]
    s = {"conv_pre.weight": (C0, cfg["n_mels"], 7), "conv_pre.bias": (C0,)}
    ch, R = C0, len(cfg["resblock_kernels"])
    snake_, hasb = cfg["activation"] != "lrelu", cfg["activation"] == "snakebeta"
    for i, k in enumerate(cfg["kernels"]):
        s[f"ups.{i}.weight"], s[f"ups.{i}.bias"] = (ch, ch // 2, k), (ch // 2,)
        ch //= 2
        for r, rk in enumerate(cfg["resblock_kernels"]):
            n = i * R + r
            for m in range(len(cfg["dilations"][r])):
                for cv in ("convs1", "convs2"):
                    s[f"resblocks.{n}.{cv}.{m}.weight"], s[f"resblocks.{n}.{cv}.{m}.bias"] = (ch, ch, rk), (ch,)
            if snake_:
                for a in range(2 * len(cfg["dilations"][r])):
                    s[f"resblocks.{n}.activations.{a}.alpha"] = (ch,)
                    if hasb:
                        s[f"resblocks.{n}.activations.{a}.beta"] = (ch,)
    if snake_:
        s["activation_post.alpha"] = (ch,)
        if hasb:
            s["activation_post.beta"] = (ch,)
    s["conv_post.weight"] = (1, ch, 7)
    if post_bias:
        s["conv_post.bias"] = (1,)
    return s


_WEIGHTS: Dict[tuple, Dict[str, torch.Tensor]] = {}


def make_weights(cfg: dict, seed: int, post_bias: bool = True, calib_T: int = 33) -> Dict[str, torch.Tensor]:
    """Deterministic fp32 weights under the canonical keys (computed once per configuration and seed; do not modify).  Gains near
    the variance-preserving ones keep every stage at order one, so that the Snake's sin sees about a radian and no padding rule,
    tap or parameter is lost in a saturated or vanishing signal; conv_post is then scaled so that the signal in front of the tanh
    peaks at 1.5 on the T = calib_T test input (the tanh must not flatten the test; the wide configurations calibrate on fewer
    frames, the fp64 forward on the host being what it costs)."""
    key = (repr(sorted(cfg.items())), seed, post_bias, calib_T)
    if key in _WEIGHTS:
        return _WEIGHTS[key]
    g = torch.Generator().manual_seed(seed)
    ups = {f"ups.{i}.weight": (u, k) for i, (u, k) in enumerate(zip(cfg["rates"], cfg["kernels"]))}
    out = {}
    for k, shp in expected_shapes(cfg, post_bias).items():
        r = torch.randn(shp, generator=g, dtype=torch.float64)
        if k.endswith(".alpha") or k.endswith(".beta"):
            # log-scale: exp(.) in [0.55, 1.8]; linear: in [0.5, 1.5]: alpha and beta of a channel differ by tens of per cent
            w = r.clamp(-2, 2) * 0.3 if cfg["alpha_logscale"] else 1.0 + r.clamp(-2, 2) * 0.25
        elif k.endswith(".bias"):
            w = r * 0.1
        elif k == "conv_pre.weight":
            w = r / (4.5 * (shp[1] * shp[2]) ** 0.5)  # the input's rms is about 4.5
        elif k in ups:
            u, kk = ups[k]
            w = r * (1.2 / (shp[0] * kk / u) ** 0.5)  # every output sample has k / u taps
        else:
            w = r * (0.8 / (shp[1] * shp[2]) ** 0.5)
        out[k] = w.float()
    peak = float(pre_tanh(out, cfg, logmel(calib_T), torch.float64).abs().max())
    out["conv_post.weight"] = (out["conv_post.weight"].double() * (1.5 / peak)).float()
    if post_bias:
        out["conv_post.bias"] = (out["conv_post.bias"].double() * (1.5 / peak)).float()
    _WEIGHTS[key] = out
    return out


def tolerance(floor: float) -> float:
    return TOL_FACTOR * floor
