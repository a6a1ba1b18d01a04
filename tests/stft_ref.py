"""Test-side restatements of the multi-resolution STFT distance (vx_stft_*, valle_amd.stft.MultiResolutionSTFT), written from the
definition in include/vallex.h (Parallel WaveGAN / `auraloss.freq.MultiResolutionSTFTLoss`; neither package is a dependency).

* `magnitude(x, res, dtype)`: `torch.stft(center=True, pad_mode="reflect")` with a periodic Hann window of `win` samples (torch
  centres it inside the n_fft frame at (n_fft - win) // 2), sqrt(clamp(re^2 + im^2, eps)).  fp64 is the yardstick, fp32 on the
  host the floor the GPU test measures the engine against.
* `magnitude_loops(x, res)`: numpy fp64, one frame at a time, the reflection resolved by index and the DFT a matrix product with
  tables of its own.  It must equal the torch form, so the definition does not rest on `torch.stft` alone.
* `sums_from_magnitudes`, `figures_from_sums`, `distance`: the four sums of a resolution, sc / lm, and the total."""
import math

import numpy as np
import torch

SR = 24000
RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
ODD = (512, 37, 255)  # a window at an odd offset: (512 - 255) // 2 = 128, one sample left of centre
EPS = 1e-8
TOL_FACTOR = 4  # engine error <= 4 x the fp32 floor, the rule of the filterbank's, the codec's and the resampler's tests


def n_frames(L, res):
    return 1 + L // res[1]


def min_samples(resolutions=RESOLUTIONS):
    """torch's reflect-padding rule: more than n_fft / 2 samples."""
    return max(r[0] for r in resolutions) // 2 + 1


def make_noise(L, seed, amp=1.0):
    """Gaussian noise (L,) float32 of standard deviation `amp`."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(L, generator=g) * amp


def power(x, res, dtype=torch.float64):
    """(frames, n_fft / 2 + 1): re^2 + im^2 before the clamp."""
    n_fft, hop, win = res
    x = torch.as_tensor(x).reshape(-1).to(dtype)
    window = torch.hann_window(win, dtype=torch.float64).to(dtype)
    spec = torch.stft(x[None], n_fft, hop_length=hop, win_length=win, window=window, center=True, pad_mode="reflect", normalized=False,
                      onesided=True, return_complex=True)
    return torch.view_as_real(spec).pow(2).sum(-1)[0].T.contiguous()


def magnitude(x, res, dtype=torch.float64, eps=EPS):
    return torch.sqrt(torch.clamp(power(x, res, dtype), min=eps))


def share_near_clamp(x, res, eps=EPS):
    """Share of fp64 cells whose power lies below 2 eps: where the clamp could decide differently in fp32."""
    return float((power(x, res, torch.float64) < 2.0 * eps).double().mean())


def make_clear_noise(L, seed, amp, resolutions, cut=None, eps=EPS):
    """`make_noise` at the first of the seeds seed, seed + 1000003, ... that leaves no cell near the clamp (`share_near_clamp` == 0)
    at any of `resolutions` (looked at over the first `cut` samples, where a pair is compared): a property of the fp64 definition alone.  About one noise signal in ten at amplitude 0.1 has such a
    cell somewhere, and there the clamp, not the DFT, would decide what the fp32 floor is."""
    for k in range(16):
        x = make_noise(L, seed + 1000003 * k, amp)
        if all(share_near_clamp(x[:cut], r, eps) == 0.0 for r in resolutions):
            return x
    raise AssertionError(f"no clear seed for L={L} amp={amp}")


def magnitude_loops(x, res, eps=EPS):
    """numpy fp64 (frames, n_fft / 2 + 1), frame by frame."""
    n_fft, hop, win = res
    x = np.asarray(x, np.float64).reshape(-1)
    L = x.shape[0]
    assert L > n_fft // 2
    off = (n_fft - win) // 2
    j = np.arange(win)
    w = 0.5 - 0.5 * np.cos(2 * math.pi * j / win)
    k = np.arange(n_fft // 2 + 1)
    ang = 2 * math.pi * ((k[:, None] * (off + j)[None, :]) % n_fft) / n_fft
    C, S = np.cos(ang), np.sin(ang)
    out = np.empty((1 + L // hop, n_fft // 2 + 1))
    for t in range(out.shape[0]):
        fr = np.empty(win)
        for i in range(win):
            p = t * hop - n_fft // 2 + off + i
            if p < 0:
                p = -p
            if p >= L:
                p = 2 * (L - 1) - p
            fr[i] = x[p] * w[i]
        re, im = C @ fr, S @ fr
        out[t] = np.sqrt(np.maximum(re * re + im * im, eps))
    return out


def sums_from_magnitudes(X, Y):
    """fp64 (4,): sum (Y - X)^2, sum Y^2, sum |ln Y - ln X|, cells; X = pred's magnitudes, Y = target's."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    d = Y - X
    return np.array([(d * d).sum(), (Y * Y).sum(), np.abs(np.log(Y) - np.log(X)).sum(), float(X.size)])


def figures_from_sums(s):
    """(sc, lm) of one resolution."""
    return math.sqrt(s[0] / s[1]), s[2] / s[3]


def distance(pred, target, resolutions=RESOLUTIONS, dtype=torch.float64, eps=EPS):
    """(sc [R], lm [R], total) of the definition; both signals cut to the common length."""
    L = min(len(pred), len(target))
    sc, lm = [], []
    for r in resolutions:
        s = sums_from_magnitudes(magnitude(pred[:L], r, dtype, eps).numpy(), magnitude(target[:L], r, dtype, eps).numpy())
        a, b = figures_from_sums(s)
        sc.append(a)
        lm.append(b)
    return sc, lm, sum(a + b for a, b in zip(sc, lm)) / len(resolutions)


def tolerance(floor):
    return TOL_FACTOR * floor
