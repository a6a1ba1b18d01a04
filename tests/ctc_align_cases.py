"""The forced alignment's test cases, shared by test_ctc_align_cpu.py and test_gpu_ctc_align.py: seeded logits and targets, and the
restatement's results (computed once per case and left unchanged).

A group is one ragged batch (one call of vx_falign): a kind of logits x a vocabulary.  Kinds: "randn" = 4 x randn in fp32;
"int" = small integers in [-3, 3], which make exact ties, and every sum of which is exact.  Per frame count T of FRAMES a group
holds: a random target of every length of LENGTHS (one longer than T is infeasible); the longest target T allows (T tokens
without an adjacent repeat: one path, no blank); a target with many adjacent repeats at about half the frames; a target whose
L + repeats is exactly T (one feasible path); the same target at T - 1 frames (infeasible).  One utterance has no frames and no
targets, one no frames and a target."""
import numpy as np

import ctc_align_ref as R

KINDS = ("randn", "int")
VOCABS = (5, 32, 70)
FRAMES = (1, 2, 3, 17, 255, 256, 257, 600)
LENGTHS = (0, 1, 2, 127, 128, 129)  # S = 2 L + 1 crosses 256
BLANK = {5: 0, 32: 0, 70: 3}        # a blank that is not id 0 too
GROUPS = [(k, v) for k in KINDS for v in VOCABS]


def _logits(g, kind, T, V):
    if kind == "int":
        return g.integers(-3, 4, (T, V)).astype(np.float32)
    return (4.0 * g.standard_normal((T, V))).astype(np.float32)


def _ids(g, n, V, blank):
    return [int(i) + (int(i) >= blank) for i in g.integers(0, V - 1, n)]  # [0, V) without the blank


def _no_repeat(g, n, V, blank):
    y = []
    while len(y) < n:
        t = _ids(g, 1, V, blank)[0]
        if not y or t != y[-1]:
            y.append(t)
    return y


def _exact(g, T, V, blank):
    """A target with adjacent repeats and L + repeats == T."""
    y, need = [], 0
    while need < T:
        if y and need + 2 <= T and g.random() < 0.4:
            y.append(y[-1])
            need += 2
        else:
            t = _no_repeat(g, 1, V, blank)[0]
            if y and t == y[-1]:
                continue
            y.append(t)
            need += 1
    return y


_GROUPS = {}


def group(kind, V):
    """(names, frames per utterance, logits (sum frames, V) float32, targets per utterance, blank)."""
    key = (kind, V)
    if key in _GROUPS:
        return _GROUPS[key]
    g = np.random.default_rng(1000 * KINDS.index(kind) + V)
    blank = BLANK[V]
    names, frames, rows, targets = [], [], [], []

    def add(name, T, y):
        names.append(name)
        frames.append(T)
        rows.append(_logits(g, kind, T, V))
        targets.append(list(y))

    for T in FRAMES:
        for L in LENGTHS:
            add(f"T{T}_L{L}", T, _ids(g, L, V, blank))
        add(f"T{T}_longest", T, _no_repeat(g, T, V, blank))
        rep = [t for t in _no_repeat(g, max(T // 4, 1), V, blank) for _ in (0, 1)]  # every token twice
        add(f"T{T}_repeats", T, rep)
        y = _exact(g, T, V, blank)
        add(f"T{T}_exact", T, y)
        add(f"T{T}_one_less", T - 1, y)
        if T == 17:  # between the two halves of the batch
            add("T0_L0", 0, [])
            add("T0_L3", 0, _ids(g, 3, V, blank))
    _GROUPS[key] = (names, frames, np.concatenate(rows), targets, blank)
    return _GROUPS[key]


def split(frames, x):
    out, o = [], 0
    for T in frames:
        out.append(x[o:o + T])
        o += T
    return out


_REF = {}


def reference(kind, V):
    """The restatement's `align` of every utterance of the group."""
    key = (kind, V)
    if key not in _REF:
        names, frames, x, targets, blank = group(kind, V)
        _REF[key] = [R.align(xi, y, blank) for xi, y in zip(split(frames, x), targets)]
    return _REF[key]
