"""Host emulation of the engine's fp8 slot caches (VX_FLAG_KV_FP8; vall-e_amd/csrc/batch_kernels.hpp: kv8_block_scale, the QKV
epilogue of bgemm_kernel, kv8_scatter_kernel, attn_batch8_kernel).

Format: every K / V row of a head is split into blocks of 16 consecutive channels; a block is 16 OCP e4m3 codes
(torch.float8_e4m3fn) and one E8M0 scale byte, value = code * 2^(byte - 127).  The byte is the smallest one in [0, 254] with
amax <= 448 * 2^(byte - 127), so no value is clipped; codes are RNE(x * 2^(127 - byte)).  The source values are the bf16 values
the bf16 cache would hold.

Also a teacher-forced KV-cached AR decoder on the fp32 oracle whose cache holds quantise-dequantised rows: what the batched
step computes with fp8 slot caches, up to the bf16 rounding of its GEMM operands."""
import math

import torch
import torch.nn.functional as F

BLOCK = 16
E4M3_MAX = 448.0
# Largest error of the emulated fp8-cache decoder against the plain fp32 oracle at the probe passes of tests/golden/kv8/, as a
# fraction of the row's largest |logit|: tools/gen_kv8_golden.py measured 0.00181 (cfg1_topk10, pass 1); rounded up to 0.0025.
KV8_EMU_ERR_MAX = 0.0025
# The engine with fp8 slot caches against the plain fp32 oracle: the batched step's bf16 tolerance (3 % of the row scale) plus the
# fp8 cache's own error with a safety factor of 4.
KV8_TOL = 0.03 + 4 * KV8_EMU_ERR_MAX


def kv8_scale_bytes(amax: torch.Tensor) -> torch.Tensor:
    """amax (...) fp32 >= 0 -> E8M0 scale bytes (...) int32: the smallest byte with amax <= 448 * 2^(byte - 127)."""
    amax = amax.float().contiguous()
    E = (amax.view(torch.int32) >> 23) & 0xFF
    byte = torch.clamp(E, min=8) - 8
    inv = ((254 - byte) << 23).to(torch.int32).view(torch.float32)
    return byte + (amax * inv > E4M3_MAX).to(torch.int32)


def kv8_quant(x: torch.Tensor):
    """x (..., K) with K % 16 == 0 (values already bf16-representable) -> (codes uint8 (..., K) e4m3 bit patterns,
    scales uint8 (..., K/16) E8M0)."""
    K = x.shape[-1]
    xb = x.float().reshape(*x.shape[:-1], K // BLOCK, BLOCK)
    byte = kv8_scale_bytes(xb.abs().amax(-1))
    inv = ((254 - byte) << 23).to(torch.int32).view(torch.float32)  # 2^(127 - byte), exact
    q = (xb * inv[..., None]).to(torch.float8_e4m3fn)  # |x * inv| <= 448: RNE, never out of range
    return q.reshape(x.shape).view(torch.uint8), byte.to(torch.uint8)


def kv8_dequant(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """inverse of kv8_quant: the exact fp32 values the attention kernel multiplies."""
    K = codes.shape[-1]
    v = codes.view(torch.float8_e4m3fn).float().reshape(*codes.shape[:-1], K // BLOCK, BLOCK)
    s = torch.ldexp(torch.ones((), dtype=torch.float32), scales.to(torch.int32) - 127)
    return (v * s[..., None]).reshape(codes.shape)


def kv8_qdq(x: torch.Tensor) -> torch.Tensor:
    """the value an fp8 slot cache returns for the fp32 row x: bf16 rounding (the bf16 cache's value), then kv8 quant / dequant."""
    return kv8_dequant(*kv8_quant(x.to(torch.bfloat16).float()))


class Kv8ArCache:
    """The oracle's ArCache (pre-norm VALL-E) with an fp8 slot cache: the prefill attends over its own unquantised rows (the
    engine's prefill attention reads the QKV rows, not the cache) and stores every K / V row quantise-dequantised; each step
    quantise-dequantises its new K / V row as it is appended, before that row is used."""

    def __init__(self, m):
        assert m.norm_first and not m.add_prenet
        self.m = m

    def prefill(self, text: torch.Tensor, yy: torch.Tensor) -> torch.Tensor:
        from oracle import valle_oracle as vo

        m = self.m
        S = text.shape[0]
        self.n_audio = yy.shape[0]
        x = torch.cat([m.ar_text(text), m.ar_audio(yy)], dim=0)
        mask = vo.ar_mask(S, yy.shape[0])
        self.k, self.v = [], []
        for L in m.ar_layers:
            x, (k, v) = vo.encoder_layer(L, x, m.nhead, mask, None, True)
            self.k.append(kv8_qdq(k))  # (H, rows, hd): blocks of 16 channels of one head's row
            self.v.append(kv8_qdq(v))
        return m.ar_logits(m.ar_final_norm(x[-1:]))

    def step(self, token: torch.Tensor) -> torch.Tensor:
        m = self.m
        x = m.ar_audio(token, start=self.n_audio)
        self.n_audio += 1
        d, H = m.d, m.nhead
        hd = d // H
        for li, L in enumerate(m.ar_layers):
            qkv = F.linear(L.norm(0, x, None), L.in_w, L.in_b)
            q, k, v = qkv.chunk(3, dim=-1)
            q = q.reshape(1, H, hd).transpose(0, 1)
            self.k[li] = torch.cat([self.k[li], kv8_qdq(k.reshape(1, H, hd).transpose(0, 1))], dim=1)
            self.v[li] = torch.cat([self.v[li], kv8_qdq(v.reshape(1, H, hd).transpose(0, 1))], dim=1)
            s = torch.matmul(q, self.k[li].transpose(1, 2)) / math.sqrt(hd)
            a = torch.matmul(F.softmax(s, dim=-1), self.v[li]).transpose(0, 1).reshape(1, d)
            x = x + F.linear(a, L.out_w, L.out_b)
            x = x + F.linear(F.relu(F.linear(L.norm(1, x, None), L.w1, L.b1)), L.w2, L.b2)
        return m.ar_logits(m.ar_final_norm(x))


@torch.no_grad()
def kv8_forced_logits(m, text: torch.Tensor, prompt_cb0: torch.Tensor, forced: torch.Tensor, passes) -> torch.Tensor:
    """Teacher-forced decode of one utterance (no BOS): text (S,), prompt_cb0 (P,), forced (T,) tokens appended at passes
    0..T-1.  Returns the logits rows (len(passes), 1025) of the requested passes (pass 0 = the prefill's)."""
    want = sorted(set(int(p) for p in passes))
    assert want[-1] <= forced.numel()
    cache = Kv8ArCache(m)
    rows = {}
    logits = cache.prefill(text, prompt_cb0)
    for p in range(want[-1] + 1):
        if p in want:
            rows[p] = logits[0].clone()
        if p == want[-1]:
            break
        logits = cache.step(forced[p].reshape(1))
    return torch.stack([rows[int(p)] for p in passes])
