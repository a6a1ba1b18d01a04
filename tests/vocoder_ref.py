"""Test-side restatement of the Griffin-Lim vocoder (vx_vocoder_*, valle_amd.vocoder.GriffinLim), written with torch.fft from the
definition in include/vallex.h.  In fp64 it is the yardstick; in fp32 on the host it is the floor the GPU test measures the engine
against (window and tables rounded to fp32).

* `mel_inverse(B)`: P = pinv(B), (513, n_mels) fp64 (numpy.linalg.pinv: an SVD, not the engine's Cholesky).
* `magnitude(logmel, P, dtype)`: max(0, exp(logmel) P^T), (T, 513).
* `inverse(X, dtype, env_floor)`: I(X), (T, 513) complex -> 256 T samples: irfft per row, window, overlap-add, floored envelope.
* `forward(y, dtype)`: S(y), 256 T samples -> (T, 513) complex: the filterbank's framing (768 zeros appended, no centring).
* `griffinlim(mag, n_iter, momentum, init, dtype)`: the iteration of torchaudio.functional.griffinlim -> (y, ang, smallest |a|).
* `spectral_convergence(y, mag)`: || |S(y)| - mag || / ||mag|| in fp64.
* `test_signal(T)`: a frequency-modulated 180 Hz tone, a 1234 Hz tone and 0.02 noise, 256 T samples."""
import math

import numpy as np
import torch

SR, N_FFT, HOP, N_BINS = 24000, 1024, 256, 513
ENV_FLOOR = 0.1
TOL_FACTOR = 4  # engine error <= 4 x the fp32 floor, the project's rule


def _complex(dtype):
    return torch.complex128 if dtype == torch.float64 else torch.complex64


def window(dtype=torch.float64):
    """Periodic Hann, computed in fp64 and rounded once."""
    j = torch.arange(N_FFT, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2 * math.pi * j / N_FFT)).to(dtype)


def mel_inverse(basis64):
    return np.linalg.pinv(np.asarray(basis64, dtype=np.float64))


def magnitude(logmel, P, dtype=torch.float64):
    mel = torch.exp(torch.as_tensor(logmel).to(dtype))
    return torch.clamp(mel @ torch.as_tensor(P).to(dtype).T, min=0.0)


def envelope(T, dtype=torch.float64):
    """env[n] = sum_f w^2[n - 256 f] over the T frames, for n in [0, 256 T + 768)."""
    w2 = window(dtype) ** 2
    env = torch.zeros(HOP * T + N_FFT - HOP, dtype=dtype)
    for f in range(T):
        env[HOP * f: HOP * f + N_FFT] += w2
    return env


def inverse(X, dtype=torch.float64, env_floor=ENV_FLOOR):
    T = X.shape[0]
    frames = torch.fft.irfft(X.to(_complex(dtype)), n=N_FFT, dim=1) * window(dtype)
    ola = torch.zeros(HOP * T + N_FFT - HOP, dtype=dtype)
    for f in range(T):
        ola[HOP * f: HOP * f + N_FFT] += frames[f]
    env = envelope(T, dtype)
    return (ola / torch.clamp(env, min=env_floor))[: HOP * T]


def forward(y, dtype=torch.float64):
    y = torch.as_tensor(y).to(dtype)
    T = y.numel() // HOP
    assert y.numel() == HOP * T
    padded = torch.cat([y, torch.zeros(N_FFT - HOP, dtype=dtype)])
    return torch.fft.rfft(padded.unfold(0, N_FFT, HOP) * window(dtype), dim=1)


def unit_phase(init_phase, dtype=torch.float64):
    """(T, 513) radians (fp32, as the engine receives them) -> unit complex."""
    p = torch.as_tensor(init_phase).to(dtype)
    return torch.complex(torch.cos(p), torch.sin(p))


def griffinlim(mag, n_iter, momentum=0.99, init=None, dtype=torch.float64, env_floor=ENV_FLOOR):
    """-> (y (256 T,), ang (T, 513) complex, a (T, 513) complex of the last iteration or None)."""
    mag = mag.to(dtype)
    ang = torch.ones(mag.shape, dtype=_complex(dtype)) if init is None else init.to(_complex(dtype))
    tprev = torch.zeros_like(ang)
    c = torch.tensor(momentum / (1.0 + momentum), dtype=dtype)
    a = None
    for _ in range(n_iter):
        reb = forward(inverse(mag * ang, dtype, env_floor), dtype)
        a = reb - tprev * c
        ang = a / (a.abs() + 1e-16)
        tprev = reb
    return inverse(mag * ang, dtype, env_floor), ang, a


def spectral_convergence(y, mag):
    mag = mag.double()
    return float(torch.linalg.norm(forward(y.double()).abs() - mag) / torch.linalg.norm(mag))


def test_signal(T, seed=0):
    """256 T samples, float32."""
    n = torch.arange(HOP * T, dtype=torch.float64)
    t = n / SR
    g = torch.Generator().manual_seed(seed)
    x = 0.4 * torch.sin(2 * math.pi * 180.0 * t + 3.0 * torch.sin(2 * math.pi * 3.0 * t)) + 0.2 * torch.sin(2 * math.pi * 1234.0 * t)
    return (x + 0.02 * torch.randn(HOP * T, generator=g).double()).float()


test_signal.__test__ = False  # a helper, not a test


def tolerance(floor):
    return TOL_FACTOR * floor
