"""Test-side restatements of the log-mel filterbank (vx_fbank_*, valle_amd.fbank.BigVGANFbank): the reference's
`BigVGANFbank._feature_fn` (valle/data/fbank.py:80-131).  lhotse and librosa are not dependencies: the frame rule and the mel
basis are written from their definitions.

* `fbank_definition(x, basis, dtype)`: zero padding to (n_frames - 1) * 256 + 1024 samples, `torch.stft` exactly as the
  reference calls it (n_fft 1024, hop 256, periodic Hann window, center=False, one-sided), sqrt(re^2 + im^2 + 1e-9), basis @ mag,
  log(clamp(., 1e-5)), transposed to (n_frames, n_mels).  In fp64 this is the yardstick; in fp32 on the host it is the floor
  the GPU test measures the engine against (window and basis rounded to fp32, as the reference holds them).
* `fbank_four_step(x, basis, dtype)`: the kernel's organisation of the DFT, n = 32 n1 + n2, k = k1 + 32 k2: DFT32 over n1,
  twiddle W1024^(n2 k1), DFT32 over n2, k2 <= 16 kept.  In fp64 it must equal the definition.
* `mel_basis_loops`: Slaney's basis written filter by filter with scalar arithmetic, against the vectorised one of the package."""
import math

import numpy as np
import torch
import torch.nn.functional as F

SR, N_FFT, HOP, N_BINS, N_MELS = 24000, 1024, 256, 513, 100
CLIP = 1e-5
TOL_FACTOR = 4  # engine error <= 4 x the fp32 floor, the rule of the codec's and the resampler's tests


def n_frames(L):
    return (L + HOP // 2) // HOP


def make_noise(L, seed, amp=1.0):
    """Gaussian noise (L,) float32 of standard deviation `amp`."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(L, generator=g) * amp


def mel_pre_log(x, basis, dtype=torch.float64):
    """(n_mels, n_frames): basis @ magnitude, before the clamp and the log."""
    x = torch.as_tensor(x).reshape(-1).to(dtype)
    nf = n_frames(x.numel())
    y = F.pad(x[None], (0, (nf - 1) * HOP + N_FFT - x.numel()))
    window = torch.hann_window(N_FFT, dtype=torch.float32 if dtype == torch.float32 else torch.float64)
    spec = torch.stft(y, N_FFT, hop_length=HOP, win_length=N_FFT, window=window.to(dtype), center=False, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    mag = torch.sqrt(torch.view_as_real(spec).pow(2).sum(-1) + 1e-9)
    return torch.matmul(torch.as_tensor(basis).to(dtype), mag)[0]


def fbank_definition(x, basis, dtype=torch.float64, clip=CLIP):
    """x (L,) with L >= 128 -> (n_frames, n_mels) in `dtype`."""
    return torch.log(torch.clamp(mel_pre_log(x, basis, dtype), min=clip)).T.contiguous()


def share_near_clip(x, basis, clip=CLIP):
    """Share of fp64 mel cells within [clip / 2, 2 clip]: where the clamp could decide differently in fp32."""
    m = mel_pre_log(x, basis, torch.float64)
    return float(((m >= 0.5 * clip) & (m <= 2.0 * clip)).double().mean())


def fbank_four_step(x, basis, dtype=torch.float64, clip=CLIP):
    """The same features through the 32 x 32 factorisation, every product a matmul in `dtype` with tables rounded from fp64."""
    x = torch.as_tensor(x).reshape(-1).to(dtype)
    nf = n_frames(x.numel())
    y = F.pad(x, (0, (nf - 1) * HOP + N_FFT - x.numel()))
    j = torch.arange(1024, dtype=torch.float64)
    win = (0.5 - 0.5 * torch.cos(2 * math.pi * j / 1024)).to(dtype)
    frames = y.unfold(0, N_FFT, HOP) * win                      # (nf, 1024)
    X = frames.reshape(nf, 32, 32)                              # [n1][n2]
    a = torch.arange(32, dtype=torch.float64)
    ang32 = 2 * math.pi * ((a[:, None] * a[None, :]) % 32) / 32
    c32, s32 = torch.cos(ang32).to(dtype), torch.sin(ang32).to(dtype)
    ang = 2 * math.pi * (a[:, None] * a[None, :]) / 1024        # [k1][n2]
    tc, ts = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
    yr, yp = c32 @ X, s32 @ X                                   # [k1][n2]: Y = yr - i yp
    zr, zq = yr * tc - yp * ts, yr * ts + yp * tc               # Z = zr - i zq
    re, im = zr @ c32 - zq @ s32, zr @ s32 + zq @ c32           # [k1][k2]: F = re - i im
    mag2 = (re * re + im * im).transpose(1, 2).reshape(nf, 1024)[:, :N_BINS]   # bin k1 + 32 k2
    mag = torch.sqrt(mag2 + 1e-9)
    mel = mag @ torch.as_tensor(basis).to(dtype).T
    return torch.log(torch.clamp(mel, min=clip))


def _hz_to_mel(f):
    return 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0) if f >= 1000.0 else 3.0 * f / 200.0


def _mel_to_hz(m):
    return 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0)) if m >= 15.0 else 200.0 * m / 3.0


def mel_basis_loops(sr=SR, n_fft=N_FFT, n_mels=N_MELS, fmin=0.0, fmax=12000.0):
    """(n_mels, n_fft / 2 + 1) float64, one filter and one bin at a time."""
    lo, hi = _hz_to_mel(fmin), _hz_to_mel(fmax)
    pts = [_mel_to_hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    nb = n_fft // 2 + 1
    w = np.zeros((n_mels, nb))
    for m in range(n_mels):
        left, centre, right = pts[m], pts[m + 1], pts[m + 2]
        for b in range(nb):
            f = b * (sr / 2.0) / (nb - 1)
            if left < f <= centre:
                w[m, b] = (f - left) / (centre - left)
            elif centre < f < right:
                w[m, b] = (right - f) / (right - centre)
            w[m, b] *= 2.0 / (right - left)
    return w


def tolerance(floor):
    return TOL_FACTOR * floor
