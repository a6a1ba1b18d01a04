"""Torch restatement of the reference's nucleus (top-p) filter (top_k_top_p_filtering, valle/models/valle.py:1241-1284) in the
form the engine's sampler computes it, and a top-p-aware ``topk_sampling`` with the oracle's signature
(oracle/valle_oracle.py) plus ``top_p``.

The reference sorts the (tempered, top-k-filtered) logits, takes c = cumsum(softmax(sorted)) and removes sorted position
k >= 1 when c[k-1] > top_p.  Restated without a sort: a token is kept iff the probability mass of the tokens with a strictly
larger logit is <= top_p (top_p as an fp32 number).  Tokens tied with the boundary token are all kept (torch's order among
equal logits is unspecified); tokens top-k removed have probability 0 and stay removed.  Masses are summed in float64 here.
"""
from typing import Optional

import torch
import torch.nn.functional as F


def fp32(top_p: float) -> float:
    """top_p as torch compares it against an fp32 tensor."""
    return float(torch.tensor(float(top_p), dtype=torch.float32))


def top_k_filter_(logits: torch.Tensor, top_k: int) -> torch.Tensor:
    """valle.py:1254-1260 in place: keep logits >= the k-th largest (ties kept)."""
    if top_k > 0:
        k = min(max(top_k, 1), logits.size(-1))
        logits[logits < torch.topk(logits, k)[0][..., -1, None]] = -float("inf")
    return logits


def exclusive_mass(logits: torch.Tensor) -> torch.Tensor:
    """Per token: the softmax mass (float64) of the tokens with a strictly larger logit.  logits (..., V)."""
    p = F.softmax(logits.double(), dim=-1)
    s, order = torch.sort(logits, dim=-1, descending=True)
    cs = torch.cumsum(torch.gather(p, -1, order), dim=-1)
    # number of strictly larger logits = position of the first equal one in descending order
    n_gt = torch.searchsorted(-s.contiguous(), -logits.contiguous(), right=False)
    prev = torch.cat([torch.zeros_like(cs[..., :1]), cs], dim=-1)
    return torch.gather(prev, -1, n_gt)


def top_p_filter_(logits: torch.Tensor, top_p: float) -> torch.Tensor:
    """valle.py:1262-1282 in place, restated: -inf where the mass of the strictly larger logits exceeds top_p."""
    if top_p < 1.0:
        logits[exclusive_mass(logits) > fp32(top_p)] = -float("inf")
    return logits


def kept_mask(logits: torch.Tensor, top_k: int, temperature: float, top_p: float) -> torch.Tensor:
    """Tokens that survive temperature, top-k and top-p (valle.py:1296-1299)."""
    x = logits.clone().float()
    if temperature != 1.0:
        x = x / temperature
    return torch.isfinite(top_p_filter_(top_k_filter_(x, top_k), top_p))


def topk_sampling(logits: torch.Tensor, top_k: int, temperature: float, exp_noise: Optional[torch.Tensor] = None,
                  top_p: float = 1.0):
    """oracle.valle_oracle.topk_sampling with the nucleus filter: argmax(p / q) over the kept tokens with ``exp_noise`` q,
    torch.multinomial(p, 1) without."""
    if temperature != 1.0:
        logits = logits / temperature
    logits = top_p_filter_(top_k_filter_(logits, top_k), top_p)
    p = F.softmax(logits, dim=-1)
    if exp_noise is None:
        return torch.multinomial(p, num_samples=1)
    return torch.argmax(p / exp_noise, dim=-1, keepdim=True)


def expected_sample(logits: torch.Tensor, top_k: int, temperature: float, top_p: float, exp_noise: torch.Tensor) -> int:
    """The token the sampler must draw from one (V,) logits row with Exp(1) noise (V,)."""
    return int(topk_sampling(logits.float().reshape(1, -1).clone(), top_k, temperature, exp_noise.reshape(1, -1), top_p)[0, 0])


def boundary_margin(logits: torch.Tensor, top_k: int, temperature: float, top_p: float) -> float:
    """How far the kept set of one (V,) row lies from changing: min |E - top_p| over the tokens top-k left (E = exclusive
    mass, each token's decision is E <= top_p); float('inf') with top-p off."""
    if top_p >= 1.0:
        return float("inf")
    x = logits.clone().float()
    if temperature != 1.0:
        x = x / temperature
    x = top_k_filter_(x, top_k)
    fin = torch.isfinite(x)
    e = exclusive_mass(x)
    d = (e - fp32(top_p)).abs()
    return float(d[fin].min()) if bool(fin.any()) else 0.0
