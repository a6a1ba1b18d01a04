"""GPU: the batched decode step's GEMM (bgemm_kernel in all six epilogues, through vx_op_bgemm) and LayerNorm (ln_batch_kernel<KG>
and ln_batch_map_kernel, through vx_op_ln_batch) against plain fp64 torch on the bf16 values the kernels read.

GEMM errors are measured in units of u = 2^-24 sum_k |a_k w_k| (+ |bias|) per element - fp32 accumulation of exact bf16
products - plus, for bf16 outputs, the output's own rounding 2^-8 |ref|.  LayerNorm: the written-back residual must equal a
float32 emulation of the kernel's fixed order bitwise; the bf16 output is measured in units of 2^-8 |ref| + 2^-22 |gamma| (|xhat|
+ |mean| / sigma + 1) (its rounding, and fp32 centring / normalisation).

Shapes are the step's forms at d in {128, 256, 512, 1024}: QKV (N = 3 d), FFN1 (RELU, N = 4 d), the VALL-F query (BIAS, N = d),
the out-projection (PARTIAL, K = d, kgroups_for(d)), FFN2 (PARTIAL, K = 4 d, 4 groups) and the head (N = 1025: one column in the
last 16-wide tile) - ns = 1, 2, 4 and 8 steps per wave, kgroups 1 and 4 - at B in {1, 5, 16, 17, 32, 33, 48, 64} (both NH forms,
every 16-row half).  Inputs have a non-zero mean, one heavy K column in A and one heavy output row in W.

Every test also checks that the nearest wrong answers, computed in fp64 from the same data, lie at least WRONG_MARGIN bounds away:
one 32-wide K step of one wave dropped, a neighbouring slot row of the same 16-row half, one partial group missing, the bias
shifted by one column.  Output buffers start as NaN / 0x7fc0 / 0xFF sentinels; everything the kernel must not write (rows >= B,
columns >= N, done slots' logits / trace / K / V rows, other cache rows, trace rows at pass >= trace_rows) must stay bitwise
untouched, and A rows >= B hold NaN: the outputs must equal, bitwise, those of a run with finite stale rows.

Worst errors measured on the MI355X (units as above), and the bounds at about 4x:
  GEMM fp32 outputs (PARTIAL, BIAS, QKV q, LOGITS)  1.57 (out-projection / query; FFN2 1.50)  -> F32_BOUND 6.5
  GEMM bf16 outputs (RELU f, QKV K / V)             0.996 (the output's own rounding)         -> BF16_BOUND 4
  ln_batch / ln_batch_map h                         0.996 (the output's own rounding)         -> LN_BOUND 4
The nearest wrong answers measured at least 248 bounds away (FFN1 at d = 1024, one K step dropped)."""
import numpy as np
import pytest
import torch

from kv8_ref import kv8_quant

pytestmark = pytest.mark.gpu

F32_BOUND = 6.5
BF16_BOUND = 4.0
LN_BOUND = 4.0
WRONG_MARGIN = 4.0  # the nearest wrong answer must be at least this many bounds away

BMAX = 64
F32_SENT = 0x7FCAFE00  # quiet NaN with a payload no kernel produces
BF16_SENT = 0x7FC0
U8_SENT = 0xFF
WIDTHS = (128, 256, 512, 1024)
# B per width: every width runs one NH = 2 and one NH = 4 form; all eight values appear for every epilogue
B_SETS = {128: (1, 17, 33, 64), 256: (5, 32, 48, 1), 512: (16, 33, 64, 5), 1024: (17, 32, 48, 16)}
VOCAB, LOGITS_STRIDE = 1025, 1088
CTX_MAX, TRACE_ROWS = 8, 6


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    engine.load_library()
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return engine


def kgroups_for(K):  # engine.hip
    return 4 if K // 128 >= 4 else 1


def _f32_fill(*shape):
    return torch.full(shape, F32_SENT, dtype=torch.int32, device="cuda").view(torch.float32)


def _bf16_fill(*shape):
    return torch.full(shape, BF16_SENT, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _bits(t):
    return t.view({torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}[t.dtype]).clone()


def _assert_sentinel(t, what):
    want = {torch.float32: F32_SENT, torch.bfloat16: BF16_SENT, torch.uint8: U8_SENT}[t.dtype]
    bits = _bits(t)
    if t.dtype == torch.bfloat16:
        bits = bits.int() & 0xFFFF
    assert bool((bits == want).all()), (what, "written outside its rows / columns / slots", int((bits != want).sum()))


def _gemm_data(B, N, K, seed):
    """A (32 or 64, K) bf16 with rows >= B returned twice (NaN / finite), W (N, K) bf16, bias (N,) fp32"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rows = 32 if B <= 32 else 64
    A = 0.5 + torch.randn(rows, K, generator=g, device="cuda")
    A[:, int(torch.randint(0, K, (1,), generator=g, device="cuda"))] *= 8  # heavy K column
    W = (0.3 + torch.randn(N, K, generator=g, device="cuda")) / K ** 0.5
    W[int(torch.randint(0, N, (1,), generator=g, device="cuda"))] *= 8  # heavy output row
    bias = torch.randn(N, generator=g, device="cuda")
    A, W = A.bfloat16(), W.bfloat16().contiguous()
    A_nan = A.clone()
    A_nan[B:] = float("nan")
    return A_nan.contiguous(), A.contiguous(), W, bias


class Ref:
    """fp64 C = A W^T over K groups, its unit u, and the K-step blocks for the dropped-step answers"""

    def __init__(self, A, W, B, kgroups=1):
        a, w = A[:B].double(), W.double()
        K = a.shape[1]
        self.kg = K // kgroups
        self.C = torch.stack([a[:, g * self.kg:(g + 1) * self.kg] @ w[:, g * self.kg:(g + 1) * self.kg].T for g in range(kgroups)])
        self.U = torch.stack([a[:, g * self.kg:(g + 1) * self.kg].abs() @ w[:, g * self.kg:(g + 1) * self.kg].abs().T
                              for g in range(kgroups)]) * 2.0 ** -24
        self.blocks = torch.einsum("bjk,njk->jbn", a.reshape(B, K // 32, 32), w.reshape(-1, K // 32, 32))  # (K/32, B, N)

    def step_blocks(self, g):
        """the 32-wide K steps of group g: (steps, B, N)"""
        s = self.kg // 32
        return self.blocks[g * s:(g + 1) * s]


def _units(err, unit):
    return float((err / unit).max()) if err.numel() else 0.0


def _neighbours(B):
    """row maps b -> b' inside b's 16-row half (the other rows of its group of 4, and b +- 4): a slot row swapped inside one half"""
    maps = []
    for f in (lambda b: b ^ 1, lambda b: b ^ 2, lambda b: b ^ 3, lambda b: (b & ~15) | ((b + 4) & 15)):
        src = [f(b) for b in range(B)]
        live = [b for b in range(B) if src[b] < B]
        if live:
            maps.append((live, [src[b] for b in live]))
    return maps


class Meas:
    """worst measured errors / nearest wrong distances of the module (printed at the end of each test)"""
    worst = {"f32": 0.0, "bf16": 0.0, "ln": 0.0}
    wrong = float("inf")

    @classmethod
    def err(cls, kind, v):
        cls.worst[kind] = max(cls.worst[kind], v)

    @classmethod
    def far(cls, v):
        cls.wrong = min(cls.wrong, v)

    @classmethod
    def show(cls, tag):
        print(f"[{tag}] worst f32 {cls.worst['f32']:.3f} bf16 {cls.worst['bf16']:.3f} ln {cls.worst['ln']:.3f} "
              f"nearest wrong {cls.wrong:.1f} bounds")


def _run_twice(launch, A_nan, A_fin, outs):
    """launch(A) with every output buffer reset to its sentinels; returns the outputs of the NaN-stale run after checking that
    the finite-stale run wrote exactly the same bits"""
    init = [o.clone() for o in outs]
    launch(A_fin)
    fin = [_bits(o) for o in outs]
    for o, i in zip(outs, init):
        o.copy_(i)
    launch(A_nan)
    for o, f in zip(outs, fin):
        assert torch.equal(_bits(o), f), "outputs depend on the stale A rows >= B"
    return outs


def _step_distance(ref, unit, steps, act=None):
    """nearest 'one 32-wide K step dropped' answer: steps (S, ...) are the steps' contributions to the pre-activation ref"""
    if act is None:
        return float((steps.abs() / unit).amax(dim=tuple(range(1, steps.dim()))).min())
    return float(((act(ref - steps) - act(ref)).abs() / unit).amax(dim=tuple(range(1, steps.dim()))).min())


def _row_distance(want, unit):
    """nearest 'slot row swapped inside its 16-row half' answer (inf at B = 1: no other row)"""
    return min((float(((want[src] - want[live]).abs() / unit[live]).max()) for live, src in _neighbours(want.shape[0])),
               default=float("inf"))


def _shift(v):
    """v shifted by one column (the last column keeps its own value)"""
    return torch.cat([v[..., 1:], v[..., -1:]], dim=-1)


def _check_far(what, bound, **dists):
    for name, dist in dists.items():
        assert dist >= WRONG_MARGIN * bound, (what, name, dist, bound)
        Meas.far(dist / bound)


def _check_err(what, kind, got, want, unit, bound):
    assert torch.isfinite(got).all(), what
    e = _units((got - want).abs(), unit)
    Meas.err(kind, e)
    assert e <= bound, (what, e, bound)


# ---- GEMM: PARTIAL (out-projection, FFN2), RELU (FFN1), BIAS (VALL-F query) ------------------------------------------------------------
FORMS = {  # name: (epi, N(d), K(d), kgroups(d))
    "out_partial": (2, lambda d: d, lambda d: d, kgroups_for),
    "ffn2_partial": (2, lambda d: d, lambda d: 4 * d, lambda d: kgroups_for(4 * d)),
    "ffn1_relu": (1, lambda d: 4 * d, lambda d: d, lambda d: 1),
    "query_bias": (5, lambda d: d, lambda d: d, lambda d: 1),
}


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_bgemm_partial_relu_bias(eng, form, d):
    epi, fN, fK, fkg = FORMS[form]
    N, K, kgroups = fN(d), fK(d), fkg(d)
    for B in B_SETS[d]:
        what = (form, d, B)
        A_nan, A_fin, W, bias = _gemm_data(B, N, K, seed=1000 * d + 10 * B + epi)
        ref = Ref(A_nan, W, B, kgroups)
        if epi == eng.BE_PARTIAL:
            part = _f32_fill(4, BMAX, N)
            _run_twice(lambda A: eng.op_bgemm(epi, A, W, None, B, kgroups=kgroups, part=part), A_nan, A_fin, [part])
            _check_err(what, "f32", part[:kgroups, :B].double(), ref.C, ref.U, F32_BOUND)
            _assert_sentinel(part[:, B:], what)
            _assert_sentinel(part[kgroups:], what)
            _check_far(what, F32_BOUND,
                       step=min(_step_distance(None, ref.U[g], ref.step_blocks(g)) for g in range(kgroups)),
                       row=min(_row_distance(ref.C[g], ref.U[g]) for g in range(kgroups)))
            continue
        x = ref.C[0] + bias.double()
        u = ref.U[0] + 2.0 ** -24 * bias.double().abs()
        if epi == eng.BE_RELU:
            out = _bf16_fill(BMAX, N)
            _run_twice(lambda A: eng.op_bgemm(epi, A, W, bias, B, f=out), A_nan, A_fin, [out])
            act = lambda v: v.clamp(min=0)  # noqa: E731
            want = act(x)
            unit, bound, kind = u + 2.0 ** -8 * want.abs(), BF16_BOUND, "bf16"
        else:
            out = _f32_fill(BMAX, N)
            _run_twice(lambda A: eng.op_bgemm(epi, A, W, bias, B, q=out), A_nan, A_fin, [out])
            act = lambda v: v  # noqa: E731
            want, unit, bound, kind = x, u, F32_BOUND, "f32"
        _check_err(what, kind, out[:B].double(), want, unit, bound)
        _assert_sentinel(out[B:], what)
        _check_far(what, bound, step=_step_distance(x, unit, ref.step_blocks(0), act), row=_row_distance(want, unit),
                   bias=float(((act(ref.C[0] + _shift(bias.double())) - want).abs() / unit).max()))
    Meas.show(f"{form} d{d}")


# ---- GEMM: QKV with bf16 and fp8 slot caches --------------------------------------------------------------------------------------------
def _slot_states(B, seed, every=5):
    g = torch.Generator().manual_seed(seed)
    done = [int(b % every == every - 2) for b in range(B)]
    row = torch.randint(0, CTX_MAX, (B,), generator=g).tolist()
    return done, row


@pytest.mark.parametrize("d", WIDTHS)
def test_bgemm_qkv_bf16_and_fp8_caches(eng, d):
    """q (B, d) fp32 for every slot; K / V at cache row row[b] of live slots only (bf16); the fp8 form's codes and scale bytes equal
    kv8_quant of exactly those bf16 rows, bitwise; every other cache element keeps its sentinel."""
    N, K, H = 3 * d, d, d // 64
    for B in B_SETS[d]:
        what = ("qkv", d, B)
        A_nan, A_fin, W, bias = _gemm_data(B, N, K, seed=7000 * d + B)
        ref = Ref(A_nan, W, B)
        done, row = _slot_states(B, d + B)
        live = [b for b in range(B) if not done[b]]
        q = _f32_fill(BMAX, d)
        kv = _bf16_fill(B, 2, H, CTX_MAX, 64)
        _run_twice(lambda A: eng.op_bgemm(eng.BE_QKV, A, W, bias, B, done=done, row=row, q=q, kv=kv, d=d, ctx_max=CTX_MAX),
                   A_nan, A_fin, [q, kv])
        x = ref.C[0] + bias.double()
        u = ref.U[0] + 2.0 ** -24 * bias.double().abs()
        unit = u.clone()
        unit[:, d:] += 2.0 ** -8 * x[:, d:].abs()  # K / V: bf16 outputs
        _check_err(what, "f32", q[:B].double(), x[:, :d], unit[:, :d], F32_BOUND)
        _assert_sentinel(q[B:], what)
        written = torch.zeros(kv.shape, dtype=torch.bool, device="cuda")
        for b in live:
            written[b, :, :, row[b]] = True
        _assert_sentinel(kv[~written], what)  # done slots, other rows
        got_kv = torch.stack([kv[b, :, :, row[b]].reshape(2 * d) for b in live]).double() if live else None
        if live:
            _check_err(what, "bf16", got_kv, x[live, d:], unit[live, d:], BF16_BOUND)
        _check_far(what, BF16_BOUND, step=_step_distance(None, unit, ref.step_blocks(0)), row=_row_distance(x, unit),
                   bias=float(((_shift(bias.double()) - bias.double()).abs() / unit).max()))
        # fp8 slot caches from the same A, W and states
        q8 = _f32_fill(BMAX, d)
        codes = torch.full((B, 2, H, CTX_MAX, 64), U8_SENT, dtype=torch.uint8, device="cuda")
        scales = torch.full((B, 2, H, CTX_MAX, 4), U8_SENT, dtype=torch.uint8, device="cuda")
        _run_twice(lambda A: eng.op_bgemm(eng.BE_QKV, A, W, bias, B, done=done, row=row, q=q8, kv=codes, kv_scale=scales, d=d,
                                          ctx_max=CTX_MAX), A_nan, A_fin, [q8, codes, scales])
        assert torch.equal(_bits(q8), _bits(q)), what
        _assert_sentinel(codes[~written], what)
        _assert_sentinel(scales[~written[..., :4]], what)
        for b in live:
            wc, ws = kv8_quant(kv[b, :, :, row[b]].float())  # (2, H, 64) the bf16 rows -> codes, (2, H, 4) scale bytes
            assert torch.equal(codes[b, :, :, row[b]], wc), (what, b, "codes")
            assert torch.equal(scales[b, :, :, row[b]], ws), (what, b, "scales")
    Meas.show(f"qkv d{d}")


# ---- GEMM: the head (BE_LOGITS with trace) and batched prefill's mapped head (BE_LOGITS_MAP) ---------------------------------------------
def _check_logits(what, logits, trace, rows_to_slot, done, pass_, ref):
    """logits / trace written exactly at the live slots (trace: pass < TRACE_ROWS), every other element a sentinel"""
    lw = torch.zeros(logits.shape, dtype=torch.bool, device="cuda")
    tw = torch.zeros(trace.shape, dtype=torch.bool, device="cuda")
    rows = [z for z, s in enumerate(rows_to_slot) if not done[s]]
    for z in rows:
        s = rows_to_slot[z]
        lw[s, :VOCAB] = True
        if pass_[s] < TRACE_ROWS:
            tw[s, pass_[s]] = True
            assert torch.equal(_bits(trace[s, pass_[s]]), _bits(logits[s, :VOCAB])), (what, z, s)
    _assert_sentinel(logits[~lw], what)  # done slots, rows >= B, columns 1025 .. 1087
    _assert_sentinel(trace[~tw], what)
    if rows:
        got = torch.stack([logits[rows_to_slot[z], :VOCAB] for z in rows]).double()
        _check_err(what, "f32", got, ref.C[0][rows], ref.U[0][rows], F32_BOUND)
    _check_far(what, F32_BOUND, step=_step_distance(None, ref.U[0], ref.step_blocks(0)), row=_row_distance(ref.C[0], ref.U[0]))


@pytest.mark.parametrize("d", WIDTHS)
def test_bgemm_head_logits_and_trace(eng, d):
    for B in B_SETS[d]:
        what = ("head", d, B)
        A_nan, A_fin, W, _ = _gemm_data(B, VOCAB, d, seed=9000 * d + B)
        ref = Ref(A_nan, W, B)
        done, _ = _slot_states(B, B, every=7)
        pass_ = [(3 * b) % (TRACE_ROWS + 2) for b in range(B)]  # some at pass >= TRACE_ROWS
        logits, trace = _f32_fill(BMAX, LOGITS_STRIDE), _f32_fill(BMAX, TRACE_ROWS, VOCAB)
        _run_twice(lambda A: eng.op_bgemm(eng.BE_LOGITS, A, W, None, B, done=done, pass_=pass_, logits=logits, trace=trace),
                   A_nan, A_fin, [logits, trace])
        _check_logits(what, logits, trace, list(range(B)), done, pass_, ref)
    Meas.show(f"head d{d}")


def _slot_map(B, g):
    """B distinct slots in random order, at least one of them >= 32"""
    m = torch.randperm(BMAX, generator=g)[:B].tolist()
    if max(m) < 32:
        m[0] = BMAX - 1
    assert m != list(range(B))
    return m


@pytest.mark.parametrize("d", WIDTHS)
def test_bgemm_mapped_head_writes_the_mapped_slots(eng, d):
    """row z of the mapped head lands in slot slot_map[z] (a non-identity map with slots >= 32; done / pass indexed by slot)"""
    for B in B_SETS[d][1:3]:
        what = ("mapped head", d, B)
        A_nan, A_fin, W, _ = _gemm_data(B, VOCAB, d, seed=11000 * d + B)
        ref = Ref(A_nan, W, B)
        g = torch.Generator().manual_seed(d * B)
        slot_map = _slot_map(B, g)
        done = [int(s % 6 == 1) for s in range(BMAX)]
        pass_ = [(5 * s) % (TRACE_ROWS + 2) for s in range(BMAX)]
        logits, trace = _f32_fill(BMAX, LOGITS_STRIDE), _f32_fill(BMAX, TRACE_ROWS, VOCAB)
        _run_twice(lambda A: eng.op_bgemm(eng.BE_LOGITS_MAP, A, W, None, B, done=done, pass_=pass_, logits=logits, trace=trace,
                                          slot_map=slot_map), A_nan, A_fin, [logits, trace])
        _check_logits(what, logits, trace, slot_map, done, pass_, ref)
    Meas.show(f"mapped head d{d}")


# ---- ln_batch<KG> and ln_batch_map ---------------------------------------------------------------------------------------------------
def _ln_ref(x, gamma, beta):
    """fp64 LayerNorm (eps 1e-5) of the fp32 rows x, and its unit (see the module docstring)"""
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    sig = (xd.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    xh = (xd - mean) / sig
    ref = xh * gamma.double() + beta.double()
    unit = 2.0 ** -8 * ref.abs() + 2.0 ** -22 * gamma.double().abs() * (xh.abs() + mean.abs() / sig + 1)
    return ref, unit


def _ln_inputs(d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x0 = 1.0 + torch.randn(BMAX, d, generator=g, device="cuda")
    x0[:, int(torch.randint(0, d, (1,), generator=g, device="cuda"))] *= 6
    gamma = 1.0 + 0.2 * torch.randn(d, generator=g, device="cuda")
    beta = 0.1 * torch.randn(d, generator=g, device="cuda")
    return g, x0, gamma, beta


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("KG", [0, 1, 4])
def test_ln_batch_fixed_order_residual_and_layernorm(eng, KG, d):
    """x[b] += ((pbias + p_0) + ...) + p_{KG-1} written back bitwise as a float32 emulation of that order; h = bf16 LN(x) within
    its bound of fp64; part rows of other slots (and groups >= KG) are NaN and must not be read; rows >= B untouched."""
    for B in B_SETS[d]:
        what = ("ln_batch", KG, d, B)
        g, x0, gamma, beta = _ln_inputs(d, 100 * d + 10 * KG + B)
        part = _f32_fill(4, BMAX, d)
        part[:KG, :B] = 0.5 * torch.randn(KG, B, d, generator=g, device="cuda")
        pbias = 0.3 * torch.randn(d, generator=g, device="cuda")
        x, h = x0.clone(), _bf16_fill(BMAX, d)
        eng.op_ln_batch(x, gamma, beta, h, B, part=part if KG else None, pbias=pbias if KG else None, kgroups=KG)
        xn, pn, bn = x0.cpu().numpy(), part.cpu().numpy(), pbias.cpu().numpy()
        t = np.broadcast_to(bn, (B, d)).astype(np.float32)
        for gi in range(KG):
            t = t + pn[gi, :B]
        want_x = xn.copy()
        if KG:
            want_x[:B] = xn[:B] + t
        assert np.array_equal(x.cpu().numpy().view(np.int32), want_x.view(np.int32)), what  # rows >= B (and KG = 0: all) unchanged
        ref, unit = _ln_ref(x[:B], gamma, beta)
        _check_err(what, "ln", h[:B].double(), ref, unit, LN_BOUND)
        _assert_sentinel(h[B:], what)
        wrong = {"row": _row_distance(ref, unit)}
        if KG:
            sums = [torch.from_numpy(pn[gi, :B]).cuda() for gi in range(KG)]
            total = sum(sums)
            wrong["group"] = min(float(((_ln_ref(x0[:B] + pbias + total - p, gamma, beta)[0] - ref).abs() / unit).max()) for p in sums)
            wrong["bias"] = float(((_ln_ref(x0[:B] + _shift(pbias) + total, gamma, beta)[0] - ref).abs() / unit).max())
        _check_far(what, LN_BOUND, **wrong)
    Meas.show(f"ln_batch KG{KG} d{d}")


@pytest.mark.parametrize("d", WIDTHS)
def test_ln_batch_map_reads_the_mapped_slots(eng, d):
    """batched prefill's final LayerNorm: h row z = LN(x[slot_map[z]]); x is only read"""
    for B in B_SETS[d][1:3]:
        what = ("ln_batch_map", d, B)
        g, x0, gamma, beta = _ln_inputs(d, 200 * d + B)
        slot_map = _slot_map(B, torch.Generator().manual_seed(B + d))
        x, h = x0.clone(), _bf16_fill(BMAX, d)
        eng.op_ln_batch(x, gamma, beta, h, B, slot_map=slot_map)
        assert torch.equal(_bits(x), _bits(x0)), what
        ref, unit = _ln_ref(x0[slot_map], gamma, beta)
        _check_err(what, "ln", h[:B].double(), ref, unit, LN_BOUND)
        _assert_sentinel(h[B:], what)
        _check_far(what, LN_BOUND, row=_row_distance(ref, unit),
                   unmapped=float(((_ln_ref(x0[:B], gamma, beta)[0] - ref).abs() / unit).max()))
    Meas.show(f"ln_batch_map d{d}")
