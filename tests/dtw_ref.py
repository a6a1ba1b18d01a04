"""Test-side restatement of dynamic time warping as include/vallex.h defines it (vx_dtw_*, valle_amd.dtw.DTW), in numpy.

* `dct_table(D, n_ceps)`: sqrt(2 / D) cos(pi k (n + 1/2) / D), k = 1 .. n_ceps, in fp64, rounded once to fp32: (D, n_ceps).
* `cepstra(x, n_ceps, dtype)` and `local_cost(A, B, dtype)`: rows times that table, and d(i, j) = sqrt(sum_k (a_ik - b_jk)^2) on
  differences.  In fp64 (the fp32 table and the fp32 inputs widened, every operation in fp64) this is the yardstick; in fp32
  (a BLAS product, differences, squares, sum and root in fp32) it is the floor the GPU tests measure the kernels against.
* `warp(cost)`: the recurrence in fp64 over a cost matrix, one anti-diagonal per numpy step, with the tie rule (the diagonal
  predecessor unless another is strictly smaller, then (i-1, j) unless (i, j-1) is strictly smaller) and the back-trace from the
  last cell: (total, path (len, 2) int32 ascending).  `warp_loops` is the same written cell by cell.
* `chain(A, B, n_ceps, dtype)`: cepstra -> cost -> warp."""
import math

import numpy as np

TOL_FACTOR = 4  # engine error <= 4 x the fp32 floor (fbank_ref.TOL_FACTOR, the rule of the codec's and the resampler's tests)
MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)


def dct_table(D, n_ceps):
    n = np.arange(D, dtype=np.float64)[:, None]
    k = np.arange(1, n_ceps + 1, dtype=np.float64)[None, :]
    return (math.sqrt(2.0 / D) * np.cos(math.pi * k * (n + 0.5) / D)).astype(np.float32)


def cepstra(x, n_ceps, dtype=np.float64):
    x = np.asarray(x, dtype=np.float32)
    if n_ceps == 0:
        return x.astype(dtype)
    return x.astype(dtype) @ dct_table(x.shape[1], n_ceps).astype(dtype)


def local_cost(A, B, dtype=np.float64):
    A, B = np.asarray(A).astype(dtype), np.asarray(B).astype(dtype)
    out = np.empty((A.shape[0], B.shape[0]), dtype=dtype)
    for i0 in range(0, A.shape[0], 64):  # row blocks: the (rows, Tb, K) differences stay small
        diff = A[i0:i0 + 64, None, :] - B[None, :, :]
        out[i0:i0 + 64] = np.sqrt((diff * diff).sum(-1, dtype=dtype))
    return out


def _backtrace(bp, Ta, Tb):
    i, j = Ta - 1, Tb - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        b = 2 if i == 0 else (1 if j == 0 else int(bp[i, j]))
        if b != 2:
            i -= 1
        if b != 1:
            j -= 1
        path.append((i, j))
    return np.asarray(path[::-1], dtype=np.int32)


def warp(cost):
    """cost (Ta, Tb), any float type -> (total: float, path (len, 2) int32)."""
    c = np.asarray(cost).astype(np.float64)
    Ta, Tb = c.shape
    G = np.full((Ta + 1, Tb + 1), np.inf)  # one row and one column of +inf in front: a predecessor that does not exist never wins
    bp = np.zeros((Ta, Tb), dtype=np.uint8)
    G[1, 1] = c[0, 0]
    for d in range(1, Ta + Tb - 1):
        i = np.arange(max(0, d - (Tb - 1)), min(d, Ta - 1) + 1)
        j = d - i
        best = G[i, j].copy()                 # (i-1, j-1)
        up, left = G[i, j + 1], G[i + 1, j]   # (i-1, j), (i, j-1)
        b = np.zeros(i.shape, dtype=np.uint8)
        m = up < best
        best[m], b[m] = up[m], 1
        m = left < best
        best[m], b[m] = left[m], 2
        G[i + 1, j + 1] = best + c[i, j]
        bp[i, j] = b
    return float(G[Ta, Tb]), _backtrace(bp, Ta, Tb)


def warp_loops(cost):
    """`warp` one cell at a time, the predecessors that exist enumerated as the definition lists them."""
    c = np.asarray(cost).astype(np.float64)
    Ta, Tb = c.shape
    G = np.zeros((Ta, Tb))
    bp = np.zeros((Ta, Tb), dtype=np.uint8)
    for i in range(Ta):
        for j in range(Tb):
            if i == 0 and j == 0:
                G[i, j] = c[i, j]
                continue
            cands = []  # in the order of preference
            if i > 0 and j > 0:
                cands.append((G[i - 1, j - 1], 0))
            if i > 0:
                cands.append((G[i - 1, j], 1))
            if j > 0:
                cands.append((G[i, j - 1], 2))
            best, b = cands[0]
            for v, code in cands[1:]:
                if v < best:
                    best, b = v, code
            G[i, j] = best + c[i, j]
            bp[i, j] = b
    return float(G[Ta - 1, Tb - 1]), _backtrace(bp, Ta, Tb)


def path_sum(cost, path):
    """The costs of the path's cells added in path order in fp64: what G(Ta-1, Tb-1) is along the best path."""
    c = np.asarray(cost)
    acc = 0.0
    for i, j in np.asarray(path).tolist():
        acc += float(c[i, j])
    return acc


def path_is_valid(path, Ta, Tb):
    p = np.asarray(path).astype(np.int64)
    if p.ndim != 2 or p.shape[1] != 2 or not (max(Ta, Tb) <= p.shape[0] <= Ta + Tb - 1):
        return False
    if tuple(p[0]) != (0, 0) or tuple(p[-1]) != (Ta - 1, Tb - 1):
        return False
    steps = {tuple(s) for s in np.diff(p, axis=0).tolist()}
    return steps <= {(1, 1), (1, 0), (0, 1)}


def chain(A, B, n_ceps, dtype=np.float64):
    """-> (cost (Ta, Tb) in `dtype`, total, path)."""
    cost = local_cost(cepstra(A, n_ceps, dtype), cepstra(B, n_ceps, dtype), dtype)
    total, path = warp(cost)
    return cost, total, path


def make_feats(T, D, seed, scale=1.0):
    """Log-mel-like rows: Gaussian around -4 with a smooth component across the channels; (T, D) float32."""
    g = np.random.default_rng(seed)
    smooth = np.cumsum(g.standard_normal((T, D)), axis=1) / math.sqrt(D)
    return (-4.0 + scale * (2.0 * smooth + g.standard_normal((T, D)))).astype(np.float32)


def tolerance(floor):
    return TOL_FACTOR * floor
