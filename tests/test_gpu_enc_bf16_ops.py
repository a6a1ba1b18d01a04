"""GPU: the kernels of the recognisers' bf16 encoder mode (enc_bf16_kernels.hpp: ebf_gemm, ebf_add_layernorm, ebf_attention) on caller
data, through the launchers the recognisers use (vx_op_enc16_*, valle_amd.whisper.op_enc16_*).

Exact cases (small integers: every sum is exact in fp32, so any order of accumulation gives the same bits): bitwise equality.
Real-valued cases: yardstick fp64 on the bf16-rounded operands, floor the same operation in torch on the host with the mode's
roundings (fp32 arithmetic, bf16 stores), bound kernel max-abs error <= 4 x floor (the project's rule).  err, floor and ratio are
printed before they are asserted and written to the file VX_ENC_BF16_OPS_PARITY_OUT names.  Every output sits between NaN guards
that must survive: the last row tile, the last column tile and the last query tile are ragged in most cases.

1. GEMM, M in {1, 50, 129, 300} x (N, K) in {(384, 128), (128, 128), (256, 128), (128, 256), (1152, 384), (1536, 384), (384, 1536)}:
   all three epilogues bitwise on integers, and within the bound on real operands (the GELU one on those alone);
2. add-LayerNorm to bf16, d in {128, 384, 1280} x M in {1, 5, 130}, with a second operand of M rows, a periodic one (Whisper's
   positions) and none: the fp32 sum bitwise, the bf16 rows within one bf16 ulp of the fp64 result rounded;
3. attention, 2 and 3 heads of 64, one segment of 1, 50, 64, 65, 75, 260 rows and the ragged batches (1, 65, 17), (130, 2, 64):
   bitwise on a dominant key (at the first, a middle and the last row) and on equal scores with integer values whose mean is
   exact; within the bound on real inputs; every segment of a batch bitwise what it is alone."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
TOL_FACTOR = 4.0
_PARITY = {}

GEMM_M = (1, 50, 129, 300)
GEMM_NK = ((384, 128), (128, 128), (256, 128), (128, 256), (1152, 384), (1536, 384), (384, 1536))
LN_D = (128, 384, 1280)
LN_M = (1, 5, 130)
ATT_HEADS = (2, 3)
ATT_SEGS = ((1,), (50,), (64,), (65,), (75,), (260,), (1, 65, 17), (130, 2, 64))


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    yield
    out = os.environ.get("VX_ENC_BF16_OPS_PARITY_OUT")
    if out and _PARITY:
        with open(out, "w") as f:
            json.dump(_PARITY, f, indent=1, sort_keys=True)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (1 << 31))


def _guarded(shape, dtype, fill=None):
    """A device tensor of `shape` between two NaN guards -> (the whole buffer, the view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def _record(kind, name, err, floor):
    ratio = err / floor if floor else (0.0 if err == 0 else float("inf"))
    print(f"{kind} {name}: kernel {err:.3e}, floor {floor:.3e}, ratio {ratio:.2f}")
    _PARITY.setdefault(kind, {})[name] = {"err": err, "floor": floor, "ratio": ratio}
    return ratio


def _bf(x):
    return x.to(torch.bfloat16)


# ---- 1. GEMM --------------------------------------------------------------------------------------------------------------------
def _run_gemm(A, W, bias, epi, res=None):
    from valle_amd.whisper import op_enc16_gemm

    M, N = A.shape[0], W.shape[0]
    buf, out = _guarded((M, N), torch.float32 if epi == 2 else torch.bfloat16, res)  # the residual is aliased to the output
    op_enc16_gemm(A.to(DEV), W.to(DEV), bias.to(DEV), epi, out if res is not None else None, out)
    torch.cuda.synchronize()
    assert _guards_intact(buf), "a store outside the output"
    return out.cpu()


@pytest.mark.parametrize("N,K", GEMM_NK)
def test_gemm_integers_bitwise(N, K):
    for M in GEMM_M:
        g = _gen(1, M, N, K)
        A = torch.randint(-4, 5, (M, K), generator=g).float()
        W = torch.randint(-3, 4, (N, K), generator=g).float()
        bias = torch.randint(-9, 10, (N,), generator=g).float()
        res = torch.randint(-50, 51, (M, N), generator=g).float()
        exact = A.double() @ W.double().T + bias.double()  # |.| <= 12 K + 9 < 2^24: exact in fp32 in any order
        assert float(exact.abs().max()) < 2 ** 24
        got = _run_gemm(_bf(A), _bf(W), bias, 0)
        assert _bits(got, _bf(exact.float())), f"bias -> bf16, M {M}"
        got = _run_gemm(_bf(A), _bf(W), bias, 2, res)
        assert _bits(got, (exact + res.double()).float()), f"bias + residual -> fp32, M {M}"
        # the GELU epilogue on integers: gelu(x) = x to the last bit of fp32 wherever x >= 8, and gelu(0) = 0
        got = _run_gemm(_bf(A), _bf(W), bias, 1)
        ref = _bf(F.gelu(exact.float()))
        far = (exact >= 8) | (exact == 0)
        assert torch.equal(got[far].view(torch.int16), ref[far].view(torch.int16)), f"gelu -> bf16 where it is the identity, M {M}"


@pytest.mark.parametrize("N,K", GEMM_NK)
def test_gemm_real_within_bound(N, K):
    for M in GEMM_M:
        g = _gen(2, M, N, K)
        A = _bf(torch.randn(M, K, generator=g))
        W = _bf(torch.randn(N, K, generator=g) * (1.5 / math.sqrt(K)))
        bias = torch.randn(N, generator=g) * 0.1
        res = torch.randn(M, N, generator=g)
        z64 = A.double() @ W.double().T + bias.double()
        z32 = A.float() @ W.float().T + bias
        for epi, name, ref, host in ((0, "bias", z64, _bf(z32).double()), (1, "gelu", F.gelu(z64), _bf(F.gelu(z32)).double()),
                                     (2, "resid", z64 + res.double(), (z32 + res).double())):
            got = _run_gemm(A, W, bias, epi, res if epi == 2 else None).double()
            ratio = _record("gemm", f"{name}_M{M}_N{N}_K{K}", float((got - ref).abs().max()), float((host - ref).abs().max()))
            assert ratio <= TOL_FACTOR, (name, M, N, K, ratio)


def test_gemm_row_is_bitwise_what_it_is_alone():
    g = _gen(3)
    N, K = 384, 384
    A = _bf(torch.randn(300, K, generator=g))
    W = _bf(torch.randn(N, K, generator=g) * 0.08)
    bias = torch.randn(N, generator=g)
    full = _run_gemm(A, W, bias, 0)
    for m in (0, 127, 128, 299):
        assert _bits(_run_gemm(A[m:m + 1].contiguous(), W, bias, 0), full[m:m + 1])
    assert _bits(_run_gemm(A, W, bias, 0), full), "a call is repeatable bit for bit"


def test_gemm_refusals():
    from valle_amd import engine as e
    from valle_amd.whisper import op_enc16_gemm

    A, b = torch.zeros(4, 128, dtype=torch.bfloat16, device=DEV), torch.zeros(128, device=DEV)
    with pytest.raises(e.VxError, match="K = 96"):
        op_enc16_gemm(A[:, :96].contiguous(), torch.zeros(128, 96, dtype=torch.bfloat16, device=DEV), b, 0)
    with pytest.raises(e.VxError, match="N = 4 "):
        op_enc16_gemm(A, torch.zeros(4, 128, dtype=torch.bfloat16, device=DEV), b[:4].contiguous(), 0)
    with pytest.raises(e.VxError, match="null operand"):
        op_enc16_gemm(A, torch.zeros(128, 128, dtype=torch.bfloat16, device=DEV), b, 2)  # no residual


# ---- 2. add-LayerNorm -----------------------------------------------------------------------------------------------------------
def _ulp_bf16(x):
    """The spacing of bf16 at |x| (fp64 tensor): 2^(floor(log2 |x|) - 7), the smallest normal's below it."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 1 - 7)


@pytest.mark.parametrize("d", LN_D)
@pytest.mark.parametrize("M", LN_M)
def test_add_layernorm(M, d):
    from valle_amd.whisper import op_enc16_add_ln

    g = _gen(4, M, d)
    a = torch.randn(M, d, generator=g) * 2.0 + 0.3
    w = 1.0 + 0.2 * torch.randn(d, generator=g)
    beta = 0.3 * torch.randn(d, generator=g)
    bmod = 3
    for kind, b, mod in (("rows", torch.randn(M, d, generator=g), 0), ("periodic", torch.randn(bmod, d, generator=g) * 1.5, bmod), ("none", None, 0)):
        bfull = None if b is None else (b[torch.arange(M) % mod] if mod else b)
        s32 = a if b is None else a + bfull
        s, y = op_enc16_add_ln(a.to(DEV), None if b is None else b.to(DEV), w.to(DEV), beta.to(DEV), 1e-5, mod)
        torch.cuda.synchronize()
        assert _bits(s.cpu(), s32), f"the fp32 sum, {kind}"
        ref = F.layer_norm(s32.double(), (d,), w.double(), beta.double(), 1e-5)
        rounded = _bf(ref.float()).double()
        diff = (y.cpu().double() - rounded).abs()
        ulp = torch.maximum(_ulp_bf16(rounded), _ulp_bf16(y.cpu().double()))
        worst = float((diff / ulp).max())
        print(f"add_ln {kind} M {M} d {d}: worst {worst:.2f} bf16 ulp")
        assert worst <= 1.0, (kind, M, d, worst)
        # without a sum buffer the rows are the same bits
        _, y2 = op_enc16_add_ln(a.to(DEV), None if b is None else b.to(DEV), w.to(DEV), beta.to(DEV), 1e-5, mod, want_sum=False)
        assert _bits(y2.cpu(), y.cpu())


# ---- 3. attention ---------------------------------------------------------------------------------------------------------------
def _run_attn(qkv, segs, heads):
    from valle_amd.whisper import op_enc16_attn

    rows = qkv.shape[0]
    buf, out = _guarded((rows, 64 * heads), torch.bfloat16)
    op_enc16_attn(qkv.to(DEV), list(segs), heads, out)
    torch.cuda.synchronize()
    assert _guards_intact(buf), "a store outside the output"
    got = out.cpu()
    assert not bool(torch.isnan(got.float()).any()), "a row was not written"
    return got


def _attn_ref(qkv, segs, heads, dtype, rounded):
    """softmax(q k^T / 8) v per segment and head on the given (bf16-valued) operands; `rounded`: the mode's roundings (the normalised
    probabilities and the output to bf16)."""
    d = 64 * heads
    out, lo = [], 0
    for T in segs:
        x = qkv[lo:lo + T].to(dtype)
        q, k, v = (x[:, i * d:(i + 1) * d].view(T, heads, 64).transpose(0, 1) for i in range(3))
        p = torch.softmax((q * 0.125) @ k.transpose(1, 2), -1)
        if rounded:
            p = _bf(p).to(dtype)
        o = (p @ v).transpose(0, 1).reshape(T, d)
        out.append(_bf(o).to(dtype) if rounded else o)
        lo += T
    return torch.cat(out)


@pytest.mark.parametrize("heads", ATT_HEADS)
@pytest.mark.parametrize("segs", ATT_SEGS, ids=lambda s: "x".join(map(str, s)))
def test_attention_dominant_key_bitwise(segs, heads):
    d, rows = 64 * heads, sum(segs)
    g = _gen(5, heads, *segs)
    for where in ("first", "middle", "last"):
        qkv = torch.zeros(rows, 3 * d)
        qkv[:, 2 * d:] = torch.randn(rows, d, generator=g)
        want = torch.empty(rows, d, dtype=torch.bfloat16)
        lo = 0
        for T in segs:
            for h in range(heads):
                j = {"first": 0, "middle": (T // 2 + h) % T, "last": T - 1}[where]
                c = (7 * h + 3) % 64
                qkv[lo:lo + T, h * 64 + c] = 16.0        # every query of the segment
                qkv[lo + j, d + h * 64 + c] = 64.0       # its score is 128, the others' 0: exp(-128) is 0 in fp32
                want[lo:lo + T, h * 64:(h + 1) * 64] = _bf(qkv[lo + j, 2 * d + h * 64:2 * d + (h + 1) * 64])
            lo += T
        assert _bits(_run_attn(_bf(qkv), segs, heads), want), where


@pytest.mark.parametrize("heads", ATT_HEADS)
@pytest.mark.parametrize("segs", ATT_SEGS, ids=lambda s: "x".join(map(str, s)))
def test_attention_equal_scores_bitwise(segs, heads):
    d, rows = 64 * heads, sum(segs)
    g = _gen(6, heads, *segs)
    qkv = torch.zeros(rows, 3 * d)
    qkv[:, d:2 * d] = torch.randint(-3, 4, (rows, d), generator=g).float()  # any keys: the queries are zero
    want = torch.empty(rows, d)
    lo = 0
    for T in segs:
        mean = torch.randint(-8, 9, (d,), generator=g).float()
        delta = torch.zeros(T, d)
        pairs = T // 2
        if pairs:
            k = torch.randint(0, 4, (pairs, d), generator=g).float()
            delta[0:2 * pairs:2], delta[1:2 * pairs:2] = k, -k  # the values of a pair cancel: the sum is T x mean, exactly
        qkv[lo:lo + T, 2 * d:] = mean + delta
        want[lo:lo + T] = mean
        lo += T
    assert _bits(_run_attn(_bf(qkv), segs, heads), _bf(want))


@pytest.mark.parametrize("heads", ATT_HEADS)
@pytest.mark.parametrize("segs", ATT_SEGS, ids=lambda s: "x".join(map(str, s)))
def test_attention_real_within_bound_and_alone(segs, heads):
    d, rows = 64 * heads, sum(segs)
    g = _gen(7, heads, *segs)
    qkv = _bf(torch.randn(rows, 3 * d, generator=g) * torch.tensor([2.0, 1.5, 1.0]).repeat_interleave(d))
    got = _run_attn(qkv, segs, heads)
    ref = _attn_ref(qkv, segs, heads, torch.float64, False)
    host = _attn_ref(qkv, segs, heads, torch.float32, True).double()
    ratio = _record("attention", f"h{heads}_" + "x".join(map(str, segs)), float((got.double() - ref).abs().max()), float((host - ref).abs().max()))
    assert ratio <= TOL_FACTOR, (segs, heads, ratio)
    assert _bits(_run_attn(qkv, segs, heads), got), "a call is repeatable bit for bit"
    if len(segs) > 1:
        lo = 0
        for T in segs:
            assert _bits(_run_attn(qkv[lo:lo + T].contiguous(), (T,), heads), got[lo:lo + T]), f"the segment of {T} rows alone"
            lo += T
