"""Writes tests/golden/topp/*.npz: the reference's nucleus (top-p) filter on a fixed set of logits rows, the vectors the top-p
tests check the engine's sampler against.  Imports the UNMODIFIED reference function ``top_k_top_p_filtering``
(valle/models/valle.py:1241-1284) through oracle/ref_harness.py, so it runs only where the reference tree is present; the
tests read nothing but the files it writes.  CPU only, deterministic: a second run writes byte-identical files.

    python tools/gen_topp_golden.py

rows.npz          logits (R, 1025) fp32 and kind (R,) int8: 0 peaked, 1 flat, 2 tied (one token in 20 repeats another's
                  logit, tied maxima in a quarter of them), 3 model-like (Gaussian, sigma 2)
cases_t<T>.npz    one file per temperature T (1.0 -> t100, 0.7 -> t070): top_p (C,), top_k (C,) int32, temperature (), and
                  for every (row, case) the reference's kept mask packed along the vocabulary (R, C, 129) uint8 (np.packbits,
                  big-endian bit order) and the margin (R, C) fp32
The margin of a (row, case) is how far the cumulative probabilities next to the boundary lie from top_p:
min(|c[m] - top_p|, |c[m-1] - top_p|) with m the first sorted position whose c exceeds top_p (|c[-1] - top_p| when none
does), c = cumsum(softmax(sorted logits)) exactly as the reference computes it.  It is 0 when the boundary position is
followed by a logit equal to it: torch's order among equal logits is unspecified, so the reference's mask then depends on
it, while the engine keeps every token tied with the boundary.  A (row, case) is decided when margin > 1e-6.
"""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

OUT = os.path.join(ROOT, "tests", "golden", "topp")
V = 1025
TOP_P = [0.1, 0.5, 0.8, 0.9, 0.95, 0.999]
TOP_K = [-100, 1, 10, 64, 200]
TEMPS = [(1.0, "t100"), (0.7, "t070")]
N_PER_KIND = 50


def make_rows():
    g = torch.Generator().manual_seed(20261016)
    rows, kinds = [], []
    for i in range(N_PER_KIND):  # peaked: a few tokens far above a wide body
        x = torch.randn(V, generator=g) * (1.0 + 0.05 * i)
        hot = torch.randint(0, V, (1 + i % 4,), generator=g)
        x[hot] += 4.0 + 0.2 * i
        rows.append(x); kinds.append(0)
    for i in range(N_PER_KIND):  # flat: nearly uniform, the nucleus holds hundreds of tokens
        rows.append(torch.randn(V, generator=g) * (0.02 + 0.01 * i)); kinds.append(1)
    for i in range(N_PER_KIND):  # tied: one token in 20 copies another's logit; tied maxima in a quarter of the rows
        x = torch.randn(V, generator=g) * (1.0 + 0.1 * i)
        src, dst = torch.randint(0, V, (V // 20,), generator=g), torch.randint(0, V, (V // 20,), generator=g)
        x[dst] = x[src]
        if i % 4 == 0:
            x[torch.randint(0, V, (2 + i % 5,), generator=g)] = float(x.max())
        rows.append(x); kinds.append(2)
    for i in range(N_PER_KIND):  # model-like
        rows.append(torch.randn(V, generator=g) * 2.0 + 0.5 * torch.randn(1, generator=g)); kinds.append(3)
    return torch.stack(rows).to(torch.float32), np.asarray(kinds, dtype=np.int8)


def margin(x: torch.Tensor, top_k: int, top_p: float) -> float:
    """The reference's own intermediate values (valle.py:1254-1276) on one tempered row: top-k, sort, cumsum of softmax."""
    x = x.clone()
    if top_k > 0:
        k = min(max(top_k, 1), x.numel())
        x[x < torch.topk(x, k)[0][..., -1, None]] = -float("inf")
    s = torch.sort(x, descending=True)[0]
    c = torch.cumsum(F.softmax(s, dim=-1), dim=-1)
    tp = float(torch.tensor(top_p, dtype=torch.float32))
    over = torch.nonzero(c > top_p)
    if over.numel() == 0:
        return abs(float(c[-1]) - tp)
    m = int(over[0])
    if m + 1 < s.numel() and bool(torch.isfinite(s[m])) and float(s[m + 1]) == float(s[m]):
        return 0.0  # the boundary splits a run of equal logits
    mg = abs(float(c[m]) - tp)
    if m >= 1:
        mg = min(mg, abs(float(c[m - 1]) - tp))
    return mg


def main():
    from oracle.ref_harness import load_reference

    load_reference()
    ref = importlib.import_module("valle.models.valle")
    torch.set_num_threads(1)
    logits, kinds = make_rows()
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "rows.npz"), logits=logits.numpy(), kind=kinds)
    cases = [(p, k) for k in TOP_K for p in TOP_P]
    for temp, tag in TEMPS:
        R, C = logits.shape[0], len(cases)
        masks = np.zeros((R, C, (V + 7) // 8), dtype=np.uint8)
        margins = np.zeros((R, C), dtype=np.float32)
        for r in range(R):
            x = logits[r : r + 1]
            if temp != 1.0:  # topk_sampling, valle.py:1296-1297
                x = x / temp
            for c, (p, k) in enumerate(cases):
                out = ref.top_k_top_p_filtering(x.clone(), top_k=k, top_p=p)
                masks[r, c] = np.packbits(torch.isfinite(out[0]).numpy())
                margins[r, c] = margin(x[0], k, p)
        np.savez_compressed(os.path.join(OUT, f"cases_{tag}.npz"), top_p=np.asarray([p for p, _ in cases], dtype=np.float32),
                            top_k=np.asarray([k for _, k in cases], dtype=np.int32), temperature=np.float32(temp), masks=masks,
                            margin=margins)
        dec = float((margins > 1e-6).mean())
        print(f"{tag}: {R} rows x {C} cases, decided {dec:.4f}")


if __name__ == "__main__":
    main()
