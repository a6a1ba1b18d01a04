"""Test-side restatements of the sample-rate converter in front of the EnCodec encoder (vx_resample, valle_amd.Resampler): the
mono path of `encodec.utils.convert_audio`, i.e. the channel mean and `torchaudio.transforms.Resample(orig, new)` with its
defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99).  torchaudio is not a dependency: both forms are written from
the rule and its constants.

* `resample_direct`: the definition.  y[j] = (base / o) sum_i x[i] sinc(pi t) cos^2(pi t / (2 w)), t = (i / o - j / n) base over
  |t| < w, x = 0 outside [0, L), j < ceil(n L / o); no phase table.  numpy fp64.
* `resample_polyphase`: torchaudio's organisation.  Kernel width W = ceil(w o / base), n phases of 2 W + o taps (the argument
  clamped to [-w, w], where the window is zero), the input padded by (W, W + o), conv1d with stride o, phases interleaved, cut
  to ceil(n L / o).  torch, any dtype: the kernel is computed in fp64 and rounded once, as torchaudio does.  In fp32 on the
  host, with the mean in fp32, this is the floor the GPU test measures the engine against."""
import math

import numpy as np
import torch
import torch.nn.functional as F

WIDTH = 6
ROLLOFF = 0.99
RATES_IN = (8000, 11025, 16000, 22050, 32000, 44100, 48000)  # -> 24000
RATES_OUT = (16000, 44100, 48000)                            # 24000 ->
TOL_FACTOR = 4  # engine error <= 4 x the fp32 floor, the rule of the codec's tests (encodec_ref.TOL_FACTOR)


def ratio(orig, new):
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    return o, n, min(o, n) * ROLLOFF


def out_length(orig, new, L, variant=None):
    o, n, _ = ratio(orig, new)
    return n * L // o if variant == "floor_length" else -(-n * L // o)


def mixdown(x, dtype=torch.float64):
    """(L,) or (C, L) -> (L,): the channel mean in `dtype`."""
    x = torch.as_tensor(x).to(dtype)
    return x if x.dim() == 1 else x.mean(0)


def resample_direct(x, orig, new, variant=None):
    """x (L,) or (C, L) -> (ceil(n L / o),) float64 numpy.  Variants (deliberately wrong, for the CPU test): "drop_tap" leaves out
    the input sample right after the centre of every output's window; "floor_length" returns floor(n L / o) samples;
    "mean_after_clip" resamples every channel, clips it to [-1, 1] as a 16-bit file would, and takes the mean last."""
    if variant == "mean_after_clip":
        x = torch.as_tensor(x)
        return np.mean([np.clip(resample_direct(x[c], orig, new), -1.0, 1.0) for c in range(x.shape[0])], axis=0)
    xm = mixdown(x).numpy()
    L = xm.shape[0]
    o, n, base = ratio(orig, new)
    J = out_length(orig, new, L, variant)
    if o == n:
        return xm.copy()[:J]
    half = int(math.ceil(WIDTH * o / base)) + 2
    ks = np.arange(-half, half + 1)
    y = np.zeros(J)
    for j0 in range(0, J, 8192):
        j = np.arange(j0, min(J, j0 + 8192))
        i = (j * o // n)[:, None] + ks[None, :]
        t = (i / o - j[:, None] / n) * base
        keep = (np.abs(t) < WIDTH) & (i >= 0) & (i < L)
        if variant == "drop_tap":
            keep &= i != (j * o // n)[:, None] + 1
        tp = t * math.pi
        coef = np.where(tp == 0.0, 1.0, np.sin(tp) / np.where(tp == 0.0, 1.0, tp)) * np.cos(tp / (2 * WIDTH)) ** 2
        y[j0:j0 + len(j)] = (base / o) * np.sum(np.where(keep, coef * xm[np.clip(i, 0, L - 1)], 0.0), axis=1)
    return y


def polyphase_kernel(orig, new):
    """(n, 2 W + o) float64 and W."""
    o, n, base = ratio(orig, new)
    W = int(math.ceil(WIDTH * o / base))
    idx = torch.arange(-W, W + o, dtype=torch.float64)[None, :] / o
    t = (torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx) * base
    t = t.clamp(-WIDTH, WIDTH)
    window = torch.cos(t * math.pi / WIDTH / 2) ** 2
    t = t * math.pi
    k = torch.where(t == 0, torch.ones_like(t), t.sin() / torch.where(t == 0, torch.ones_like(t), t))
    return k * window * (base / o), W


def resample_polyphase(x, orig, new, dtype=torch.float64):
    """x (L,) or (C, L) -> (ceil(n L / o),) in `dtype` (mean, kernel and convolution)."""
    xm = mixdown(x, dtype)
    o, n, _ = ratio(orig, new)
    if o == n:
        return xm.clone()
    k, W = polyphase_kernel(orig, new)
    L = xm.shape[0]
    y = F.conv1d(F.pad(xm[None, None], (W, W + o)), k.to(dtype)[:, None, :], stride=o)  # (1, n, frames)
    return y[0].T.reshape(-1)[:out_length(orig, new, L)]


def make_noise(L, seed, channels=1):
    """Unit-variance noise (C, L) float32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(channels, L, generator=g)


def tolerance(floor):
    return TOL_FACTOR * floor
