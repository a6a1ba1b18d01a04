"""Test-side restatement of CTC forced alignment and text likelihood as include/vallex.h defines them (vx_falign, vx_falign_asr,
valle_amd.asr.ctc_forced_align / ctc_nll), in numpy fp64.  test_ctc_align_cpu.py pins it against F.ctc_loss and against exhaustive
enumeration; test_gpu_ctc_align.py holds the kernels against it.

`mutation` states a deliberate mistake, for the test that shows the likelihood's bound tells each from the definition:
  no_skip         no transition from s - 2
  skip_repeats    the transition from s - 2 also across a repeated label
  end_last_blank  the end in the last blank only
  start_blank     the start in the first blank only"""
import numpy as np

MUTATIONS = ("no_skip", "skip_repeats", "end_last_blank", "start_blank")
NEG = -np.inf


def extended(y, blank):
    z = np.full(2 * len(y) + 1, int(blank), dtype=np.int64)
    z[1::2] = np.asarray(y, dtype=np.int64)
    return z


def feasible(T, y):
    y = list(y)
    repeats = sum(1 for k in range(1, len(y)) if y[k] == y[k - 1])
    return T >= len(y) + repeats and not (T == 0 and len(y) > 0)


def lse_rows(x):
    """lse[t] = m + log sum_c exp(x[t][c] - m), m the row's maximum, the sum in fp64."""
    x = np.asarray(x, dtype=np.float32)
    m = x.max(axis=1).astype(np.float64)
    return m + np.log(np.exp(x.astype(np.float64) - m[:, None]).sum(axis=1))


def _skips(z, blank, mutation=None):
    S = len(z)
    sk = np.zeros(S, dtype=bool)
    if mutation != "no_skip":
        for s in range(2, S):
            sk[s] = z[s] != blank and (mutation == "skip_repeats" or z[s] != z[s - 2])
    return sk


def _shift(a, k):
    return np.concatenate([np.full(k, NEG), a[:len(a) - k]]) if k <= len(a) else np.full(len(a), NEG)


def nll(x, y, blank=0, mutation=None):
    """-log p(y | x) by the forward algorithm; +inf when infeasible; 0 for no frames and no targets."""
    x = np.asarray(x, dtype=np.float32)
    T = x.shape[0]
    if not feasible(T, y):
        return np.inf
    if T == 0:
        return 0.0
    z = extended(y, blank)
    S = len(z)
    e = x[:, z].astype(np.float64) - lse_rows(x)[:, None]
    sk = _skips(z, blank, mutation)
    a = np.full(S, NEG)
    a[0] = e[0, 0]
    if S > 1 and mutation != "start_blank":
        a[1] = e[0, 1]
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            a = e[t] + np.logaddexp(np.logaddexp(a, _shift(a, 1)), np.where(sk, _shift(a, 2), NEG))
        if S == 1 or mutation == "end_last_blank":
            return float(-a[S - 1])
        return float(-np.logaddexp(a[S - 1], a[S - 2]))


def align(x, y, blank=0):
    """Everything vx_falign reports for one utterance, as a dict: nll, path_logprob, feasible, frame_tokens (T,), starts / ends (L,),
    scores (L,) float32, and states (T,), the best path itself."""
    x = np.asarray(x, dtype=np.float32)
    T, L = x.shape[0], len(y)
    out = dict(nll=nll(x, y, blank), feasible=feasible(T, y))
    if not out["feasible"] or T == 0:
        bad = not out["feasible"]
        out.update(path_logprob=-np.inf if bad else 0.0, frame_tokens=np.full(T, -1), starts=np.full(L, -1), ends=np.full(L, -1),
                   scores=np.full(L, -np.inf, dtype=np.float32), states=np.full(T, -1))
        return out
    z = extended(y, blank)
    S = len(z)
    lse = lse_rows(x)
    r = x[:, z].astype(np.float64)  # the raw emissions
    sk = _skips(z, blank)
    v = np.full(S, NEG)
    v[0] = r[0, 0]
    if S > 1:
        v[1] = r[0, 1]
    moves = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        best, mv = v.copy(), np.zeros(S, dtype=np.int8)
        p1 = _shift(v, 1)
        take = p1 > best
        best[take], mv[take] = p1[take], 1
        p2 = _shift(v, 2)
        take = sk & (p2 > best)
        best[take], mv[take] = p2[take], 2
        v = best + r[t]
        moves[t] = mv
    s = S - 1
    if S >= 2 and v[S - 2] > v[S - 1]:
        s = S - 2
    v_end = v[s]
    states = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(moves[t, s])
    out["path_logprob"] = float(v_end - lse.sum())
    out["states"] = states
    out["frame_tokens"] = np.where(states % 2 == 1, states // 2, -1)
    starts, ends, scores = np.full(L, -1), np.full(L, -1), np.full(L, -np.inf, dtype=np.float32)
    for k in range(L):
        at = np.nonzero(states == 2 * k + 1)[0]
        starts[k], ends[k] = at[0], at[-1] + 1
        assert len(at) == ends[k] - starts[k]
        total = 0.0
        for t in at:  # in frame order
            total += float(r[t, 2 * k + 1]) - float(lse[t])
        scores[k] = np.float32(total / len(at))
    out.update(starts=starts, ends=ends, scores=scores)
    return out


def bound(T, value):
    """The bound of include/vallex.h's fp64 quantities: per frame one log, at most three exp and a few additions, each within an
    ulp or two of a magnitude that never exceeds the total."""
    return 16.0 * T * 2.0 ** -52 * max(1.0, abs(value))
