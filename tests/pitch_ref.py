"""Test-side restatement of the pitch tracker as include/vallex.h defines it (vx_pitch_*, valle_amd.pitch.PitchTracker), in numpy.

* `half_diffs(x, tau_max, dtype)`: h_u(tau) = sum_{j < 256} (x[256 u + j] - x[256 u + j + tau])^2 for u = 0 .. T, on differences.
  In fp64 (the fp32 samples widened, every operation in fp64) this is the yardstick; in fp32 (differences, squares and numpy's
  sum in fp32) it is the floor the GPU tests measure the kernel against.
* `cmnd(x, fmin, fmax, dtype)`: d = h_t + h_{t+1} in `dtype`, then d'(tau) = d tau / sum_{k <= tau} d(k) with the running sum
  and the quotient in fp64 (1 where the sum is 0, and at tau = 0); with dtype fp32 the result is rounded to fp32 as the engine's
  is, with fp64 it is left as it is.
* `pick(dp, ...)` (vectorised) and `pick_loops(dp, ...)` (the definition's loops) must agree: lag, voiced, and per frame the
  MARGIN, the smallest |lhs - rhs| over every comparison the search evaluated on that frame: each d' < threshold up to and
  including the first hit, each step of the descent including the one that ends it, and for an unvoiced frame the gap between
  the minimum and the runner-up.  A frame whose margin exceeds the error of d' is decided: another d' within that error takes the
  same decisions.
* `refine(dp, lag, voiced, tau_max)`: the parabolic offset and f0, in fp64.
* `track(x, ...)`: all of it.  `compare_sums(fa, fb, path)`: the 11 sums of vx_pitch_compare in fp64."""
import math

import numpy as np

from dtw_ref import TOL_FACTOR, tolerance  # noqa: F401  (the same rule: engine error <= 4 x the fp32 floor)

RATE, HOP = 24000, 256
# The GPU test's inputs (tests/test_gpu_pitch.py): 127 has no frame, 128 one; 4095 / 4096 / 4097 sit on the edge of a 16-frame
# tile and of a half; 24000 and 36001 hold every segment of `make_signal`.  The bands: the default, and the widest one served
# (tau_min = 12, tau_max = 511).  The seed of a length is the first of L, L + 1, ... with which the fp32 restatement meets the
# decided-frame rule on both bands (test_pitch_cpu asserts that it does).
LENGTHS = (127, 128, 1000, 4095, 4096, 4097, 24000, 36001)
BANDS = ((60.0, 600.0), (47.0, 2000.0))
SEEDS = {127: 127, 128: 128, 1000: 1000, 4095: 4095, 4096: 4096, 4097: 4098, 24000: 24000, 36001: 36001}


def lag_range(fmin, fmax):
    return int(math.floor(RATE / float(np.float32(fmax)))), int(math.ceil(RATE / float(np.float32(fmin))))


def num_frames(L):
    return (int(L) + HOP // 2) // HOP


def half_diffs(x, tau_max, dtype=np.float64):
    x = np.asarray(x, dtype=np.float32)
    T = num_frames(x.shape[0])
    xp = np.zeros((T + 1) * HOP + tau_max, dtype=dtype)
    n = min(x.shape[0], xp.shape[0])
    xp[:n] = x[:n]
    h = np.empty((T + 1, tau_max + 1), dtype=dtype)
    for u in range(T + 1):
        seg = xp[HOP * u: HOP * u + HOP + tau_max]
        win = np.lib.stride_tricks.sliding_window_view(seg, HOP)  # row tau = seg[tau : tau + 256]
        diff = seg[None, :HOP] - win
        h[u] = (diff * diff).sum(-1, dtype=dtype)
    return h


def cmnd(x, fmin=60.0, fmax=600.0, dtype=np.float64):
    """-> d' (T, tau_max + 1), float32 for dtype fp32 and float64 for fp64."""
    _, tau_max = lag_range(fmin, fmax)
    h = half_diffs(x, tau_max, dtype)
    d = (h[:-1] + h[1:]).astype(np.float64)
    T = d.shape[0]
    dp = np.ones((T, tau_max + 1))
    if T:
        cs = np.cumsum(d[:, 1:], axis=1)
        tau = np.arange(1, tau_max + 1, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            dp[:, 1:] = np.where(cs > 0, d[:, 1:] * tau / cs, 1.0)
    return dp.astype(np.float32) if dtype == np.float32 else dp


def pick_loops(dp, tau_min, tau_max, threshold):
    """The definition, one frame and one comparison at a time -> (lag int32, voiced bool, margin float64), each (T,)."""
    thr = float(np.float32(threshold))
    T = dp.shape[0]
    lag, voiced, margin = np.zeros(T, np.int32), np.zeros(T, bool), np.zeros(T)
    for t in range(T):
        r = dp[t].astype(np.float64)
        m, tau, hit = np.inf, tau_min, False
        while tau <= tau_max:
            m = min(m, abs(r[tau] - thr))
            if r[tau] < thr:
                hit = True
                break
            tau += 1
        if hit:
            while tau < tau_max:
                m = min(m, abs(r[tau + 1] - r[tau]))
                if not (r[tau + 1] < r[tau]):
                    break
                tau += 1
        else:
            tau = tau_min
            for k in range(tau_min + 1, tau_max + 1):
                if r[k] < r[tau]:
                    tau = k
            others = np.delete(r[tau_min:tau_max + 1], tau - tau_min)
            m = min(m, float(others.min() - r[tau]))
        lag[t], voiced[t], margin[t] = tau, hit, m
    return lag, voiced, margin


def pick(dp, tau_min, tau_max, threshold):
    """`pick_loops` on whole arrays."""
    thr = float(np.float32(threshold))
    r = np.asarray(dp).astype(np.float64)
    T = r.shape[0]
    if T == 0:
        return np.zeros(0, np.int32), np.zeros(0, bool), np.zeros(0)
    idx = np.arange(tau_max + 1)[None, :]
    in_range = idx >= tau_min
    under = (r < thr) & in_range
    voiced = under.any(1)
    first = np.where(voiced, under.argmax(1), tau_max)  # unvoiced: every lag of the range was compared
    m_thr = np.where(in_range & (idx <= first[:, None]), np.abs(r - thr), np.inf).min(1)
    step = np.full_like(r, np.inf)            # |d'(tau + 1) - d'(tau)| at tau < tau_max
    step[:, :-1] = np.abs(r[:, 1:] - r[:, :-1])
    stops = np.ones(r.shape, bool)            # the descent ends at tau
    stops[:, :-1] = ~(r[:, 1:] < r[:, :-1])
    stop = (stops & (idx >= first[:, None])).argmax(1)
    m_desc = np.where((idx >= first[:, None]) & (idx <= stop[:, None]), step, np.inf).min(1)
    rng = r[:, tau_min:]
    amin = rng.argmin(1)
    two = np.partition(rng, 1, axis=1)[:, :2]
    m_gap = two[:, 1] - two[:, 0]
    lag = np.where(voiced, stop, amin + tau_min).astype(np.int32)
    margin = np.minimum(m_thr, np.where(voiced, m_desc, m_gap))
    return lag, voiced, margin


def refine(dp, lag, voiced, tau_max):
    """-> (f0 float64 (T,), aperiodicity (T,) in dp's type)."""
    r = np.asarray(dp)
    T = r.shape[0]
    t = np.arange(T)
    lag = np.asarray(lag).astype(np.int64)
    b = r[t, lag].astype(np.float64)
    a = r[t, lag - 1].astype(np.float64)
    c = r[t, np.minimum(lag + 1, tau_max)].astype(np.float64)
    den = a - 2.0 * b + c
    ok = (lag < tau_max) & (den > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        off = np.where(ok, np.clip((a - c) / (2.0 * np.where(ok, den, 1.0)), -0.5, 0.5), 0.0)
    f0 = np.where(voiced, RATE / (lag + off), 0.0)
    return f0, r[t, lag]


def track(x, fmin=60.0, fmax=600.0, threshold=0.1, dtype=np.float64):
    """-> dict(dp, f0, aperiodicity, lag, voiced, margin); with dtype fp32, f0 is rounded to fp32 as the engine's is."""
    tau_min, tau_max = lag_range(fmin, fmax)
    dp = cmnd(x, fmin, fmax, dtype)
    lag, voiced, margin = pick(dp, tau_min, tau_max, threshold)
    f0, ap = refine(dp, lag, voiced, tau_max)
    if dtype == np.float32:
        f0 = f0.astype(np.float32)
    return dict(dp=dp, f0=f0, aperiodicity=ap, lag=lag, voiced=voiced, margin=margin)


def undecided_allowed(T):
    """At most 5 % of an utterance's frames may be undecided; utterances of fewer than 20 frames allow one."""
    return 1 if T < 20 else int(0.05 * T)


def compare_sums(fa, fb, path):
    """The 11 sums of vx_pitch_compare along `path` (length, 2), cells clamped into the tracks; numpy fp64."""
    fa, fb = np.asarray(fa, np.float32).astype(np.float64), np.asarray(fb, np.float32).astype(np.float64)
    p = np.asarray(path).astype(np.int64)
    a = fa[np.clip(p[:, 0], 0, fa.shape[0] - 1)]
    b = fb[np.clip(p[:, 1], 0, fb.shape[0] - 1)]
    va, vb = a > 0, b > 0
    both = va & vb
    a, b = a[both], b[both]
    c, la, lb = 1200.0 * np.log2(a / b), np.log(a), np.log(b)
    return np.array([p.shape[0], both.sum(), (va != vb).sum(), math.fsum(c), math.fsum(c * c), math.fsum((a - b) ** 2), math.fsum(la),
                     math.fsum(lb), math.fsum(la * la), math.fsum(lb * lb), math.fsum(la * lb)], dtype=np.float64)


# ---- signals ---------------------------------------------------------------------------------------------------------------------
def harmonic(L, f0_hz, n_harm=5, seed=0, phase=True):
    """A tone of `n_harm` harmonics with amplitudes 1 / k and (seeded) random phases; f0_hz a scalar or an (L,) array."""
    g = np.random.default_rng(seed)
    ph = 2.0 * np.pi * np.cumsum(np.broadcast_to(np.asarray(f0_hz, dtype=np.float64), (L,))) / RATE
    x = np.zeros(L)
    for k in range(1, n_harm + 1):
        x += np.sin(k * ph + (g.uniform(0, 2 * np.pi) if phase else 0.0)) / k
    return (0.3 * x).astype(np.float32)


def make_signal(L, seed, f0_hz=140.0):
    """Speech-like in structure: a vibrato'd 5-harmonic segment (45 %), a silent one (25 %), a noise-only one (30 %), over a
    1e-3 noise floor.  (L,) float32."""
    g = np.random.default_rng(seed)
    n1, n2 = int(0.45 * L), int(0.70 * L)
    t = np.arange(L) / RATE
    f = f0_hz * (1.0 + 0.03 * np.sin(2 * np.pi * 5.0 * t + g.uniform(0, 2 * np.pi)))
    x = harmonic(L, f, 5, seed).astype(np.float64)
    x[n1:] = 0.0
    x[n2:] += 0.1 * g.standard_normal(L - n2)
    x += 1e-3 * g.standard_normal(L)
    return x.astype(np.float32)


def segments(L):
    """The frames lying wholly inside the harmonic segment of make_signal(L, ...): slice(0, n)."""
    return slice(0, max(0, (int(0.45 * L) - 1024) // HOP))


def voice(L, seed, f0_hz=150.0):
    """A voiced utterance for the comparisons under a warp: 8 harmonics whose tilt moves (amplitudes k^-p(t), p between 0.5 and
    2 at 3 Hz: the cepstra change along the utterance, so a warp path has something to hold on to) at a steady `f0_hz`, over a
    1e-3 noise floor.  (L,) float32."""
    g = np.random.default_rng(seed)
    t = np.arange(L) / RATE
    ph = 2.0 * np.pi * f0_hz * t
    p = 1.25 + 0.75 * np.sin(2 * np.pi * 3.0 * t + g.uniform(0, 2 * np.pi))
    x = np.zeros(L)
    for k in range(1, 9):
        x += np.sin(k * ph + g.uniform(0, 2 * np.pi)) * k ** -p
    return (0.2 * x + 1e-3 * g.standard_normal(L)).astype(np.float32)


def resampled(x, ratio):
    """x read `ratio` times as fast (linear interpolation): every frequency times `ratio`, the duration divided by it."""
    x = np.asarray(x, dtype=np.float64)
    pos = np.arange(int((x.shape[0] - 1) / ratio)) * ratio
    return np.interp(pos, np.arange(x.shape[0]), x).astype(np.float32)


SYLLABLE = 3072  # samples: 512 of pause, 2048 voiced, 512 of pause; 12 hops


def syllables(n, seed):
    """`n` syllables of SYLLABLE samples, each a steady 6-harmonic tone of its own pitch (whole tones apart, in a seeded order)
    and tilt between two pauses, over a 1e-3 noise floor.  (n SYLLABLE,) float32."""
    g = np.random.default_rng(seed)
    pitches = 110.0 * 2.0 ** (g.permutation(n) / 6.0)
    x = 1e-3 * g.standard_normal(n * SYLLABLE)
    for s, f in enumerate(pitches):
        ph = 2.0 * np.pi * f * np.arange(2048) / RATE
        tilt = g.uniform(0.5, 2.0)
        for k in range(1, 7):
            x[s * SYLLABLE + 512: s * SYLLABLE + 2560] += 0.2 * np.sin(k * ph + g.uniform(0, 2 * np.pi)) * k ** -tilt
    return x.astype(np.float32)


def stretched(x, block=SYLLABLE, every=3):
    """A time-stretched copy: every `every`-th block of `block` samples (a multiple of the hop) is played twice.  With `syllables`
    the cuts fall inside the pauses: every voiced stretch of the copy is, sample for sample, one of the original."""
    x = np.asarray(x, dtype=np.float32)
    out = []
    for k, i in enumerate(range(0, x.shape[0], block)):
        out.append(x[i:i + block])
        if k % every == every - 1 and i + block <= x.shape[0]:
            out.append(x[i:i + block])
    return np.concatenate(out)
