"""GPU: the row path's split-K construction piece by piece against plain fp64 torch on the values the kernels read - the
split-K launch of the N = d GEMMs (mfma_gemm_kernel<GE_PLAIN, true, RING> with gridDim.z slices, through vx_op_gemm_partial), the
LayerNorm that folds the slabs (layernorm_rows_kernel with part / xout / out == NULL, through vx_op_ln_fold) and the two
together against the residual epilogue the stack takes without slabs (vx_op_gemm_rows form 1).

Data as in test_gpu_batch_kernels.py: non-zero means, one heavy K column in A, one heavy output row in W, a bias of order 1,
bf16 operands; the reference is fp64 on exactly those values.

  partial GEMM   slab z against A[:, z K / s : (z + 1) K / s] W[:, same]^T in units of 2^-24 sum |a| |w| over that slice;
                 N = d in {128, 256, 512, 1024}, K in {d, 4 d}, every admissible slice count, M in {1, 127, 128, 129, 300, 1025}.
                 RING: 64 when (N / 128) ceil(M / 128) s <= CU count, else 32.  On 256 CUs every case of the grid runs RING = 64
                 except d = 1024, M = 1025, s = 4 (288 workgroups; slices of 256 and 1024 k); the engine's own plan never leaves
                 RING = 64.  RING_32_SHORT adds tall cases that reach RING = 32 at slices of 64 and 128 k (two and four ring
                 stages).  test_partial_cases_cover_both_rings_and_every_slice asserts, from the device's CU count, that RING = 64
                 sees slices of 64, 128, 256, 512, 1024 k (1, 2, 4, 8, 16 stages) and RING = 32 slices of 64, 128, 256, 1024.
                 The buffer starts as NaN sentinels and ends in a guard of 128 N floats that must stay untouched; a spill past
                 row M - 1 of slab z lands in slab z + 1 and is a value error there.  Two calls agree bitwise.
  fold LayerNorm d in {128, 256, 384, 512, 1024} (384: lanes masked in the second float4 group), rows in {1, 3, 4, 5, 1025},
                 nsplit in {1, 2, 4}, bf16 / fp32 output, plain / adaptive, in the four modes: written back to x; xout aliasing
                 x; separate xout; fold only.  part holds exactly nsplit slabs and NaN sentinels after them.  The written-back
                 residual (and the fold-only result) equals the float32 host evaluation x + (((pbias + p0) + p1) + ...) bitwise;
                 out in units of u |ref| + 2^-22 |gamma| (|xhat| + |mean| / sigma + 1) [x |w| for AdaLN], u = 2^-8 (bf16) or
                 2^-24 (fp32 out, and xout); with a separate xout x stays bitwise as it was; rows >= rows keep their sentinels.
  composition    partial, then fold only, on a residual X0 against fp64 X0 + A W^T + b, in units of 2^-24 (sum |a| |w| + |b| +
                 |X0|); the same for vx_op_gemm_rows(resid=X0); d = 1024, K in {1024, 4096}, M in {300, 1025}, the slice counts
                 vx_op_rows_plan gives.
  wrong answers  computed in fp64 from the same data, each at least WRONG_MARGIN bounds from what the kernel returned: one slab
                 missing, the last slab twice, bias missing, bias twice, slices of A and W paired off by one, the row below
                 folded into row r.

Worst errors measured on the MI355X (units as above) and the bounds at about 4x:
  partial fp32 slabs      6.77 (d = 1024, K = 4096 in one slice; 2.75 / 3.86 / 5.13 at d = 128 / 256 / 512)  -> PARTIAL_BOUND 27
  LN bf16 out             0.996 (the output's own rounding)                                            -> LN_BF16_BOUND 4
  LN fp32 out and xout    0.716                                                                        -> LN_F32_BOUND 3
  composition             3.17 (M = 1025, K = 4096, two slices; the residual epilogue included)        -> COMP_BOUND 12.5
The nearest wrong answers measured 487 bounds away for the bf16 LayerNorm (the last slab twice), 85 000 for the composition
(bias missing / twice), 88 000 for the partial GEMM (the row below) and 390 000 for the fp32 LayerNorm."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PARTIAL_BOUND = 27.0
LN_BF16_BOUND = 4.0
LN_F32_BOUND = 3.0
COMP_BOUND = 12.5
WRONG_MARGIN = 4.0  # the nearest wrong answer must be at least this many bounds away

U16, U32 = 2.0 ** -8, 2.0 ** -24
F32_SENT = 0x7FCAFE00  # quiet NaN with a payload no kernel produces
BF16_SENT = 0x7FC0
WIDTHS = (128, 256, 512, 1024)
M_SET = (1, 127, 128, 129, 300, 1025)
LN_WIDTHS = (128, 256, 384, 512, 1024)
LN_ROWS = (1, 3, 4, 5, 1025)
RING_32_SHORT = ((256, 256, 4, 4200), (256, 256, 2, 8300))  # (d, K, splits, M): RING = 32 at slices of 64 / 128 k on <= 256 CUs


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    engine.load_library()
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return engine


def _cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _f32_fill(n):
    return torch.full((n,), F32_SENT, dtype=torch.int32, device="cuda").view(torch.float32)


def _fill(shape, dtype):
    if dtype == torch.float32:
        return torch.full(shape, F32_SENT, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full(shape, BF16_SENT, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _bits(t):
    return t.view({torch.float32: torch.int32, torch.bfloat16: torch.int16}[t.dtype])


def _is_sentinel(t):
    bits = _bits(t)
    if t.dtype == torch.bfloat16:
        return bool(((bits.int() & 0xFFFF) == BF16_SENT).all())
    return bool((bits == F32_SENT).all())


def _units(err, unit):
    return float((err / unit).max()) if err.numel() else 0.0


class Meas:
    """worst measured errors and nearest wrong answers (in bounds) of the module, printed by every test"""
    worst = {}
    wrong = {}

    @classmethod
    def err(cls, kind, v):
        cls.worst[kind] = max(cls.worst.get(kind, 0.0), v)

    @classmethod
    def far(cls, kind, name, v):
        k = f"{kind}/{name}"
        cls.wrong[k] = min(cls.wrong.get(k, float("inf")), v)

    @classmethod
    def show(cls, tag):
        print(f"\n[{tag}] worst " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(cls.worst.items())))
        print(f"[{tag}] nearest wrong (bounds) " + ", ".join(f"{k} {v:.1f}" for k, v in sorted(cls.wrong.items())))


def _check_err(fails, what, kind, got, want, unit, bound):
    if not bool(torch.isfinite(got).all()):
        fails.append((what, kind, "not finite"))
        return
    e = _units((got - want).abs(), unit)
    Meas.err(kind, e)
    if e > bound:
        fails.append((what, kind, round(e, 3), bound))


def _check_far(fails, what, kind, bound, got, unit, **wrongs):
    """every wrong answer (fp64, the shape of got) at least WRONG_MARGIN bounds from what the kernel returned"""
    for name, w in wrongs.items():
        dist = _units((w - got).abs(), unit) / bound
        Meas.far(kind, name, dist)
        if dist < WRONG_MARGIN:
            fails.append((what, kind, "wrong answer " + name, round(dist, 3)))


def _gemm_data(M, N, K, seed):
    """A (M, K), W (N, K) bf16, bias (N,) fp32"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = 0.5 + torch.randn(M, K, generator=g, device="cuda")
    A[:, int(torch.randint(0, K, (1,), generator=g, device="cuda"))] *= 8  # heavy K column
    W = (0.3 + torch.randn(N, K, generator=g, device="cuda")) / K ** 0.5
    W[int(torch.randint(0, N, (1,), generator=g, device="cuda"))] *= 8  # heavy output row
    bias = torch.randn(N, generator=g, device="cuda")
    return A.bfloat16().contiguous(), W.bfloat16().contiguous(), bias


class SliceRef:
    """fp64 products of the K slices of A W^T and their units 2^-24 sum |a| |w|, for 1, 2 and 4 slices (from quarters of K)"""

    def __init__(self, A, W):
        self.a, self.w = A.double(), W.double()
        K = self.a.shape[1]
        q = K // 4
        self.Cq = torch.stack([self.a[:, i * q:(i + 1) * q] @ self.w[:, i * q:(i + 1) * q].T for i in range(4)])
        self.Uq = torch.stack([self.a[:, i * q:(i + 1) * q].abs() @ self.w[:, i * q:(i + 1) * q].abs().T for i in range(4)]) * U32

    def C(self, s):
        return self.Cq.view(s, 4 // s, *self.Cq.shape[1:]).sum(1)

    def U(self, s):
        return self.Uq.view(s, 4 // s, *self.Uq.shape[1:]).sum(1)

    def mispaired(self, s):
        """slice z of A with slice z + 1 of W (the last with the first)"""
        k = self.a.shape[1] // s
        return torch.stack([self.a[:, z * k:(z + 1) * k] @ self.w[:, ((z + 1) % s) * k:((z + 1) % s + 1) * k].T for z in range(s)])


def _run_partial(eng, A, W, M, splits):
    """(slabs (splits, M, N) fp32, ok) after two launches into fresh sentinel buffers with a guard of 128 N floats"""
    N = W.shape[0]
    n = splits * M * N
    bufs = []
    for _ in range(2):
        buf = _f32_fill(n + 128 * N)
        eng.op_gemm_partial(A, W, buf, splits, M=M)
        bufs.append(buf)
    return bufs[0][:n].view(splits, M, N), _is_sentinel(bufs[0][n:]), torch.equal(_bits(bufs[0]), _bits(bufs[1]))


def _partial_case(eng, fails, what, A, W, ref, M, splits):
    got, guard_ok, same = _run_partial(eng, A, W, M, splits)
    if not guard_ok:
        fails.append((what, "guard after the last slab written"))
    if not same:
        fails.append((what, "two calls differ"))
    got = got.double()
    want, unit = ref.C(splits)[:, :M], ref.U(splits)[:, :M]
    _check_err(fails, what, "partial", got, want, unit, PARTIAL_BOUND)
    wrongs = {}
    if splits > 1:
        wrongs["mispaired"] = ref.mispaired(splits)[:, :M]
    if M > 1:
        wrongs["row_below"] = torch.cat([want[:, 1:], want[:, -1:]], 1)
    _check_far(fails, what, "partial", PARTIAL_BOUND, got, unit, **wrongs)


def _splits_for(K):
    return [s for s in (1, 2, 4) if K % (64 * s) == 0]


def _ring(d, M, splits, cu):
    return 64 if (d // 128) * ((M + 127) // 128) * splits <= cu else 32


@pytest.mark.parametrize("d", WIDTHS)
def test_partial_gemm_slabs_match_fp64(eng, d):
    fails = []
    for K in (d, 4 * d):
        A, W, _ = _gemm_data(max(M_SET), d, K, seed=31 * d + K)
        ref = SliceRef(A, W)
        for splits in _splits_for(K):
            for M in M_SET:
                _partial_case(eng, fails, (d, K, splits, M, f"ring {_ring(d, M, splits, _cu_count())}"), A, W, ref, M, splits)
    Meas.show(f"partial d{d}")
    assert not fails, fails[:20]


@pytest.mark.parametrize("d,K,splits,M", RING_32_SHORT)
def test_partial_gemm_ring32_at_short_slices(eng, d, K, splits, M):
    """more workgroups than CUs at a slice of 64 / 128 k: the RING = 32 kernel's prologue and tail alone (2 stages), then one
    steady-state pair (4 stages) - reachable through the entry only (the stack's plan keeps slices x tiles within the CUs)"""
    assert _ring(d, M, splits, _cu_count()) == 32, "the case no longer reaches RING = 32 on this device"
    fails = []
    A, W, _ = _gemm_data(M, d, K, seed=77 * d + splits)
    _partial_case(eng, fails, (d, K, splits, M, "ring 32"), A, W, SliceRef(A, W), M, splits)
    Meas.show(f"partial ring32 K/s {K // splits}")
    assert not fails, fails[:20]


def test_partial_cases_cover_both_rings_and_every_slice():
    """a condition on the case lists above: with this device's CU count they reach both kernels at every slice length"""
    cu = _cu_count()
    seen = {64: set(), 32: set()}
    for d in WIDTHS:
        for K in (d, 4 * d):
            for s in _splits_for(K):
                for M in M_SET:
                    seen[_ring(d, M, s, cu)].add(K // s)
    for d, K, s, M in RING_32_SHORT:
        seen[_ring(d, M, s, cu)].add(K // s)
    assert seen[64] >= {64, 128, 256, 512, 1024}, seen
    assert seen[32] >= {64, 128, 256, 1024}, seen


# ---- the folding LayerNorm ---------------------------------------------------------------------------------------------------------
def _ln_ref(x, gamma, beta, w=None, c=None):
    """fp64 (Adaptive)LayerNorm (eps 1e-5) of the fp32 rows x, and the arithmetic part of its unit (see the module docstring)"""
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    sig = (xd.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    xh = (xd - mean) / sig
    ref = xh * gamma.double() + beta.double()
    arith = 2.0 ** -22 * gamma.double().abs() * (xh.abs() + mean.abs() / sig + 1)
    if w is not None:
        ref, arith = w.double() * ref + c.double(), arith * w.double().abs()
    return ref, arith


def _fold_data(rows, d, nsplit, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda")  # noqa: E731
    x0 = 1.0 + r(rows, d)
    x0[:, int(torch.randint(0, d, (1,), generator=g, device="cuda"))] *= 6
    part = _f32_fill((nsplit + 1) * rows * d)  # exactly nsplit slabs, then sentinels that must not enter the sum
    part[:nsplit * rows * d] = 0.5 * r(nsplit * rows * d)
    return dict(x0=x0, part=part, pbias=r(d), gamma=1.0 + 0.2 * r(d), beta=0.1 * r(d), ada_w=1.0 + 0.3 * r(d), ada_b=0.2 * r(d))


def _host_fold(D, rows, d, nsplit):
    """float32 host evaluation of x + (((pbias + p0) + p1) + ...)"""
    p = D["part"][:nsplit * rows * d].cpu().numpy().reshape(nsplit, rows, d)
    t = np.broadcast_to(D["pbias"].cpu().numpy(), (rows, d)).astype(np.float32)
    for z in range(nsplit):
        t = t + p[z]
    want = D["x0"].cpu().numpy() + t
    assert want.dtype == np.float32
    return torch.from_numpy(want).cuda()


PAD = 7  # sentinel rows after the last row of every buffer
MODES = ("write_back", "xout_alias", "xout_separate", "fold_only")


def _fold_case(eng, fails, what, D, rows, d, nsplit, want_x, dtype, ada, mode):
    x = _fill((rows + PAD, d), torch.float32)
    x[:rows] = D["x0"]
    fold_only = mode == "fold_only"
    out = None if fold_only else _fill((rows + PAD, d), dtype)
    xout = {"xout_alias": x, "xout_separate": _fill((rows + PAD, d), torch.float32)}.get(mode)
    aw, ab = (D["ada_w"], D["ada_b"]) if ada else (None, None)
    eng.op_ln_fold(x, rows, d, out=out, gamma=D["gamma"], beta=D["beta"], ada_w=aw, ada_b=ab, part=D["part"], nsplit=nsplit,
                   part_stride=rows * d, pbias=D["pbias"], xout=xout, out_dtype=dtype)
    for name, t in (("x", x), ("out", out), ("xout", xout)):
        if t is not None and not _is_sentinel(t[rows:]):
            fails.append((what, name, "rows past the last written"))
    if mode in ("write_back", "fold_only") and not torch.equal(_bits(x[:rows]), _bits(want_x)):
        fails.append((what, "the written-back residual differs from the float32 evaluation in the kernel's order",
                      int((_bits(x[:rows]) != _bits(want_x)).sum())))
    if mode == "xout_separate" and not torch.equal(_bits(x[:rows]), _bits(D["x0"])):
        fails.append((what, "x written although xout redirects the result"))
    if fold_only:
        return
    kind, bound, u = ("ln_bf16", LN_BF16_BOUND, U16) if dtype == torch.bfloat16 else ("ln_f32", LN_F32_BOUND, U32)
    ref, arith = _ln_ref(want_x, D["gamma"], D["beta"], aw, ab)
    unit = u * ref.abs() + arith
    got = out[:rows].double()
    _check_err(fails, what, kind, got, ref, unit, bound)
    if xout is not None:
        _check_err(fails, what, "ln_f32", xout[:rows].double(), ref, U32 * ref.abs() + arith, LN_F32_BOUND)
    if mode != "write_back":
        return
    # the nearest wrong folds, normalised in fp64
    x0, b = D["x0"].double(), D["pbias"].double()
    P = D["part"][:nsplit * rows * d].view(nsplit, rows, d).double()
    total = P.sum(0)
    ln = lambda v: _ln_ref(v, D["gamma"], D["beta"], aw, ab)[0]  # noqa: E731
    wrongs = {"slab_twice": ln(x0 + b + total + P[-1]), "no_bias": ln(x0 + total), "bias_twice": ln(x0 + 2 * b + total)}
    for z in range(nsplit):
        wrongs[f"slab_missing{z}"] = ln(x0 + b + total - P[z])
    if rows > 1:
        wrongs["row_below"] = ln(x0 + b + torch.cat([total[1:], total[-1:]], 0))
    _check_far(fails, what, kind, bound, got, unit, **wrongs)


@pytest.mark.parametrize("d", LN_WIDTHS)
def test_fold_layernorm_every_mode(eng, d):
    fails = []
    for rows in LN_ROWS:
        for nsplit in (1, 2, 4):
            D = _fold_data(rows, d, nsplit, seed=1000 * d + 10 * rows + nsplit)
            want_x = _host_fold(D, rows, d, nsplit)
            for dtype in (torch.bfloat16, torch.float32):
                for ada in (False, True):
                    for mode in MODES:
                        _fold_case(eng, fails, (d, rows, nsplit, str(dtype)[6:], "ada" if ada else "plain", mode), D, rows, d, nsplit,
                                   want_x, dtype, ada, mode)
    Meas.show(f"fold d{d}")
    assert not fails, fails[:20]


# ---- partial, then fold only == the residual epilogue ------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1024, 4096])
@pytest.mark.parametrize("M", [300, 1025])
def test_partial_then_fold_matches_fp64_and_the_residual_epilogue(eng, M, K):
    d = 1024
    splitk, sp_d, sp_ff = eng.op_rows_plan(M, d)
    splits = sp_d if K == d else sp_ff
    assert splitk == 1
    if _cu_count() == 256:
        assert splits == {300: 4, 1025: 2}[M], (sp_d, sp_ff)
    fails, what = [], (M, K, splits)
    A, W, bias = _gemm_data(M, d, K, seed=5 * M + K)
    g = torch.Generator(device="cuda").manual_seed(M + K)
    X0 = 1.0 + torch.randn(M, d, generator=g, device="cuda")
    ref = SliceRef(A, W)
    prod, b, x0 = ref.C(1)[0], bias.double(), X0.double()
    want = x0 + prod + b
    unit = ref.U(1)[0] + U32 * (b.abs() + x0.abs())
    # the stack's way with slabs
    slabs, guard_ok, same = _run_partial(eng, A, W, M, splits)
    assert guard_ok and same, what
    x = _fill((M + PAD, d), torch.float32)
    x[:M] = X0
    eng.op_ln_fold(x, M, d, part=slabs, nsplit=splits, part_stride=M * d, pbias=bias)
    assert _is_sentinel(x[M:]), what
    got = x[:M].double()
    _check_err(fails, what, "comp", got, want, unit, COMP_BOUND)
    # ... and without: the residual added in the GEMM epilogue
    x2 = _fill((M + PAD, d), torch.float32)
    x2[:M] = X0
    eng.op_gemm_rows(A, W, bias, resid=x2[:M])
    assert _is_sentinel(x2[M:]), what
    _check_err(fails, what + ("epilogue",), "comp", x2[:M].double(), want, unit, COMP_BOUND)
    C = ref.C(splits)
    wrongs = {"no_bias": x0 + prod, "bias_twice": want + b, "slab_twice": want + C[-1],
              "row_below": x0 + b + torch.cat([prod[1:], prod[-1:]], 0)}
    if splits > 1:
        wrongs["mispaired"] = x0 + b + ref.mispaired(splits).sum(0)
    for z in range(splits):
        wrongs[f"slab_missing{z}"] = want - C[z]
    _check_far(fails, what, "comp", COMP_BOUND, got, unit, **wrongs)
    Meas.show(f"composition M{M} K{K}")
    assert not fails, fails[:20]
