"""GPU: the batched decode attention (attn_batch_kernel / attn_batch8_kernel, through vx_op_attn_slots) and the segmented flash
attention of batched NAR / batched prefill (mfma_attn_kernel with row segments, through vx_op_attention_segs) against plain
fp64 torch: softmax(q.K^T / 8).V over exactly the visible keys (fp8 caches: the dequantised codes, tests/kv8_ref.py).

Errors are measured in units of u = 2^-9 (|ref| + vbar) (slots: 2^-9 |ref| + 2^-16 vbar), vbar = sum_j p_j |v_j| the
softmax-weighted magnitude of the values: one bf16 rounding of the output (up to 2 u: bf16's unit roundoff is 2^-8) and, in the
MFMA kernel, of every weight P, plus fp32 accumulation.  Every test also checks that the nearest wrong answer - one key more or one key less, another segment's mask - is
farther from the kernel's output than its bound, so the bound cannot hide an off-by-one."""
import pytest
import torch

from kv8_ref import kv8_dequant, kv8_quant

pytestmark = pytest.mark.gpu

# Worst error in units u measured on the MI355X, and the bounds at about 4x that: slots 1.97 (bf16 caches) / 1.97 (fp8 caches),
# i.e. the output's own bf16 rounding; segments 1.27 - 1.64 (<2,2> 1.38, <2,1> 1.39, <4,1> 1.64).  The nearest wrong answers
# measured 526 units (slots) and 1668 units (segments) away.
SLOT_BOUND = 8.0
SEG_BOUND = 6.5
WRONG_MARGIN = 4.0  # the nearest wrong answer must be at least this many bounds away


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    engine.load_library()
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return engine


# ---- batched decode attention over slot caches ----------------------------------------------------------------------------------
# Keys per wave and per pass (STEP) of the two kernels: bf16 8 keys per wave x 4 waves x 4 unrolled = 128; fp8 16 x 4 x 4 = 256.
KPW = {0: 8, 1: 16}
SLOT_CTX = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 511, 512, 513, 1024]
SLOT_GEOM = {"d1024": (16, 1920), "d256": (4, 300)}  # (H, ctx_max): configs[4]'s cache (max_text 128 + max_audio 1792); a small one


def _slot_ctx(B, ctx_max):
    """(ctx, wide) per slot: every straddling ctx value once with each construction, then seeded random ones."""
    if B == 1:
        return [ctx_max], [True]
    base = [c for c in SLOT_CTX if c < ctx_max - 1] + [ctx_max - 1, ctx_max]
    ctx = base + base
    wide = [i % 2 == 1 for i in range(len(base))] + [i % 2 == 0 for i in range(len(base))]
    g = torch.Generator().manual_seed(ctx_max)
    while len(ctx) < B:
        ctx.append(int(torch.randint(1, ctx_max + 1, (1,), generator=g)))
        wide.append(len(ctx) % 2 == 0)
    return ctx[:B], wide[:B]


def _late_wave3_key(c, kpw):
    """a key < c - 1 of wave 3 in the last pass over c keys (the running maximum moves there, after waves 0-2 have settled),
    else the key before c - 1"""
    step = 16 * kpw
    cand = [j for j in range((c - 1) // step * step, c - 1) if (j // kpw) % 4 == 3]
    return cand[-1] if cand else (c - 2 if c >= 2 else None)


def _slot_ref(q, K, V, n):
    """fp64 attention of one slot over its first n keys: q (H, 64), K / V (H, >= n, 64) -> (out, vbar) (H, 64)"""
    s = torch.einsum("hc,hjc->hj", q.double(), K[:, :n].double()) / 8
    p = torch.softmax(s, dim=-1)
    v = V[:, :n].double()
    return torch.einsum("hj,hjc->hc", p, v), torch.einsum("hj,hjc->hc", p, v.abs())


def _slot_data(fp8, B, H, ctx_max, ctx, wide, seed):
    """q (B, H, 64) fp32 and clean K / V (B, H, ctx_max, 64) (bf16 values).  Two constructions make keys ctx-1 and ctx matter:
    - not wide: keys ctx-1 and ctx (if it exists) score 9 above every other key (k = alpha q) and carry distinct V rows;
    - wide: q is scaled so that the random keys' scores spread over about +-60; the largest score sits in wave 3's keys of
      the last pass, key ctx-1 one below it and key ctx half a unit below it."""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    q = torch.randn(B, H, 64, generator=g, device=dev)
    K = torch.randn(B, H, ctx_max, 64, generator=g, device=dev).bfloat16().float()
    V = torch.randn(B, H, ctx_max, 64, generator=g, device=dev).bfloat16().float()
    for b, (c, w) in enumerate(zip(ctx, wide)):
        if w:
            q[b] *= 160.0 / q[b].norm(dim=-1, keepdim=True)  # score std |q| / 8 = 20
        qb = q[b].double()
        s = torch.einsum("hc,hjc->hj", qb, K[b, :, :c].double()) / 8

        def put(j, score):  # key j of every head scores `score` (H,) (up to the bf16 rounding of k)
            K[b, :, j] = (8 * score / (qb * qb).sum(-1))[:, None].mul(qb).bfloat16().float()

        if not w:
            top = s[:, : c - 1].amax(-1) if c > 1 else torch.zeros(H, dtype=torch.float64, device=dev)
            for j in (c - 1, c):
                if j < ctx_max:
                    put(j, top + 9)
                    V[b, :, j] = (3 * torch.randn(H, 64, generator=g, device=dev)).bfloat16().float()
        else:
            top = s.amax(-1)
            p = _late_wave3_key(c, KPW[fp8])
            if p is not None:
                put(p, top + 4)
            put(c - 1, top + 3)
            if c < ctx_max:
                put(c, top + 3.5)
    return q, K, V


def _slot_cache(fp8, K, V):
    """two-layer caches [slot][layer][K|V][head][ctx_max][64], the data in layer 1 and NaN in layer 0 (a kernel that assumed a
    one-layer slot stride would read it); returns (codes or bf16 cache, scales or None) and the values the kernel multiplies"""
    B, H, T, _ = K.shape
    if not fp8:
        kv = torch.empty((B, 2, 2, H, T, 64), dtype=torch.bfloat16, device=K.device)
        kv.view(torch.int16).fill_(-1)  # 0xFFFF: NaN
        kv[:, 1, 0], kv[:, 1, 1] = K.bfloat16(), V.bfloat16()
        return kv, None, K, V
    codes = torch.full((B, 2, 2, H, T, 64), 0x7F, dtype=torch.uint8, device=K.device)  # e4m3 NaN
    scales = torch.full((B, 2, 2, H, T, 4), 0xFF, dtype=torch.uint8, device=K.device)  # E8M0 NaN
    for i, X in enumerate((K, V)):
        c, s = kv8_quant(X)
        codes[:, 1, i], scales[:, 1, i] = c, s
    return codes, scales, kv8_dequant(codes[:, 1, 0], scales[:, 1, 0]), kv8_dequant(codes[:, 1, 1], scales[:, 1, 1])


def _poison_past_ctx(kv1, sc1, ctx, nan):
    """every cache row >= ctx[b] of layer 1: NaN (bf16 0xFFFF; fp8 code 0x7F, scale 0xFF) or huge finite values"""
    T = kv1.shape[3]
    dead = (torch.arange(T, device=kv1.device)[None, :] >= torch.tensor(ctx, device=kv1.device)[:, None])[:, None, None, :, None]
    if sc1 is None:
        kv1.view(torch.int16).masked_fill_(dead, -1 if nan else 0x7F7F)
    else:
        kv1.masked_fill_(dead, 0x7F if nan else 0x7E)
        sc1.masked_fill_(dead, 0xFF if nan else 0xF0)


@pytest.mark.parametrize("geom,B", [("d1024", 64), ("d1024", 33), ("d1024", 1), ("d256", 64)])
@pytest.mark.parametrize("fp8", [0, 1], ids=["bf16", "fp8"])
def test_attn_slots_matches_fp64(eng, fp8, geom, B):
    """Per-slot ctx values straddling the kernels' pass boundaries in one launch, on layer 1 of a two-layer cache whose rows past
    ctx are poisoned; then done slots (NaN q and caches) must be skipped without disturbing the live ones."""
    H, ctx_max = SLOT_GEOM[geom]
    ctx, wide = _slot_ctx(B, ctx_max)
    q, K, V = _slot_data(fp8, B, H, ctx_max, ctx, wide, seed=17 + B + fp8)
    kv, sc, Kx, Vx = _slot_cache(fp8, K, V)
    kv1, sc1 = kv[:, 1], (None if sc is None else sc[:, 1])
    q2 = q.reshape(B, H * 64).contiguous()
    run = lambda **kw: eng.op_attn_slots(q2, kv1, sc1, ctx, kw.get("done"), ctx_max, out=kw.get("out"))

    _poison_past_ctx(kv1, sc1, ctx, nan=True)
    out = run()
    assert torch.equal(run().view(torch.int16), out.view(torch.int16)), "not deterministic"
    _poison_past_ctx(kv1, sc1, ctx, nan=False)
    out_huge = run()
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out_huge.view(torch.int16), out.view(torch.int16)), "a cache row past ctx reached the output"

    o = out.float().reshape(B, H, 64).double()
    worst, nearest_wrong = 0.0, float("inf")
    for b, c in enumerate(ctx):
        ref, vbar = _slot_ref(q[b], Kx[b], Vx[b], c)
        if not wide[b]:  # the construction holds on the values the kernel multiplies
            s = torch.einsum("hc,hjc->hj", q[b].double(), Kx[b, :, :c].double()) / 8
            assert c == 1 or (s[:, c - 1] - s[:, : c - 1].amax(-1)).min() >= 8, (b, c)
        unit = 2.0 ** -9 * ref.abs() + 2.0 ** -16 * vbar
        err = ((o[b] - ref).abs() / unit).max().item()
        worst = max(worst, err)
        assert err <= SLOT_BOUND, f"slot {b} ctx {c} {'wide' if wide[b] else 'dominant'}: error {err:.3f} units"
        for n in (c - 1, c + 1):  # one key less / more: every head must see the difference
            if 1 <= n <= ctx_max:
                alt, _ = _slot_ref(q[b], Kx[b], Vx[b], n)
                d = ((o[b] - alt).abs() / unit).amax(-1).min().item()
                nearest_wrong = min(nearest_wrong, d)
                assert d > WRONG_MARGIN * SLOT_BOUND, f"slot {b} ctx {c}: the {n}-key answer is only {d:.2f} units away"
    print(f"\nattn_slots {'fp8' if fp8 else 'bf16'} {geom} B={B}: worst {worst:.3f} units (bound {SLOT_BOUND}), "
          f"nearest wrong answer {nearest_wrong:.1f} units")

    # done slots: NaN q rows and NaN caches; their out rows keep a sentinel, the live rows are bitwise those of the run above
    done = [int(b % 3 == 1 or b == B - 1) for b in range(B)]
    if B == 1:
        done = [1]
    dmask = torch.tensor(done, dtype=torch.bool, device=q.device)
    q2[dmask] = float("nan")
    if sc is None:
        kv.view(torch.int16)[dmask] = -1
    else:
        kv[dmask], sc[dmask] = 0x7F, 0xFF
    sentinel = torch.full((B, H * 64), 0x3C5A, dtype=torch.int16, device=q.device)
    out_d = run(done=done, out=sentinel.clone().view(torch.bfloat16)).view(torch.int16)
    assert torch.equal(out_d[dmask], sentinel[dmask]), "a done slot's output row was written"
    assert torch.equal(out_d[~dmask], out.view(torch.int16)[~dmask]), "done slots changed a live slot's output"


# ---- segmented flash attention (batched NAR / batched prefill) -----------------------------------------------------------------
def _instance(max_len, H, nseg):
    """mfma_attn_dispatch's choice of mfma_attn_kernel<NW, KG> for a launch over nseg segments"""
    nwg2 = -(-max_len // 64) * H * nseg
    return (2, 2) if nwg2 < 512 else ((2, 1) if nwg2 < 2048 else (4, 1))


_L32 = [300, 1, 31, 32, 63, 64, 65, 127]
SEG_LAYOUTS = {  # name: (H, segment lengths, segments followed by an extra gap tile, the kernel instance the launch must reach)
    "h4_short": (4, [300, 31, 127], (0,), (2, 2)),
    "h4_long": (4, [1800, 64, 1025], (0,), (2, 2)),
    "h16_8seg": (16, [1, 31, 32, 63, 64, 65, 127, 300], (2, 5), (2, 1)),
    "h16_32seg": (16, [_L32[(5 * i) % 8] for i in range(32)], (7, 20), (4, 1)),
    "h16_cfg4": (16, [1800, 1025, 1800, 1800, 1, 1800, 1800, 300, 1800, 64, 1800, 1800, 127, 1800, 1800, 65], (3, 9), (4, 1)),
}
POISON_V = 8192.0


def _seg_layout(lens, gaps):
    """starts at the next 64-row boundary, plus a gap tile after the listed segments and after every segment that ends on a
    tile boundary (so row start + len is always a poisoned row); at least 64 poisoned rows after the last segment"""
    starts, r = [], 0
    for z, n in enumerate(lens):
        starts.append(r)
        r = -(-(r + n) // 64) * 64 + (64 if (z in gaps or n % 64 == 0) else 0)
    return starts, -(-r // 64) * 64 + 64


def _seg_qkv(H, starts, lens, rows, seed):
    """random bf16 q / k / v in the segments; every other row (gaps, tail) has K = 0 and V = +-8192: finite, but a single
    leaked key of it moves an output by far more than the bound"""
    d = 64 * H
    g = torch.Generator(device="cuda").manual_seed(seed)
    qkv = torch.randn(rows, 3 * d, generator=g, device="cuda")
    inseg = torch.zeros(rows, dtype=torch.bool, device="cuda")
    for s, n in zip(starts, lens):
        inseg[s : s + n] = True
    gap = ~inseg
    qkv[gap, d : 2 * d] = 0.0
    sign = torch.randint(0, 2, (int(gap.sum()), d), generator=g, device="cuda") * 2 - 1
    qkv[gap, 2 * d :] = POISON_V * sign.float()
    return qkv.bfloat16(), inseg


def _seg_ref(qkv, H, s, n, text, nkeys=None):
    """fp64 attention of the n query rows of the segment at row s over its first nkeys (default n) keys, prefix mask `text`
    (None: no mask) -> (out, vbar) (n, H, 64)"""
    d = 64 * H
    nk = n if nkeys is None else nkeys
    x = qkv[s : s + max(n, nk)].double()
    qh = x[:n, :d].reshape(n, H, 64).transpose(0, 1)
    kh = x[:nk, d : 2 * d].reshape(nk, H, 64).transpose(0, 1)
    vh = x[:nk, 2 * d :].reshape(nk, H, 64).transpose(0, 1)
    sc = qh @ kh.transpose(1, 2) / 8
    if text is not None:
        i = torch.arange(n, device=qkv.device)[:, None]
        limit = torch.where(i < text, torch.full_like(i, text), i + 1)
        sc = sc.masked_fill(torch.arange(nk, device=qkv.device)[None, :] >= limit, float("-inf"))
    p = torch.softmax(sc, dim=-1)
    return (p @ vh).transpose(0, 1), (p @ vh.abs()).transpose(0, 1)


def _seg_texts(lens):
    """the prefix-mask runs: every segment at text 0, 1, 63, 64, len-1, len (clamped to [0, len]), and a per-segment mix whose
    segment 0 is causal (text 0) and the others are not"""
    runs = {f"text{t}": [min(t, n) for n in lens] for t in (0, 1, 63, 64)}
    runs["text_len-1"] = [n - 1 for n in lens]
    runs["text_len"] = list(lens)
    mix = [lambda n: n, lambda n: 64, lambda n: n - 1, lambda n: 63, lambda n: n // 2]
    runs["mixed"] = [0] + [min(n, max(0, mix[z % len(mix)](n))) for z, n in enumerate(lens[1:])]
    return runs


@pytest.mark.parametrize("layout", sorted(SEG_LAYOUTS))
def test_attention_segs_matches_fp64(eng, layout):
    """Every segment against fp64 over exactly its own rows, without a mask (batched NAR) and with per-segment prefix masks
    (batched prefill); gap rows of `out` stay bitwise untouched."""
    H, lens, gaps, inst = SEG_LAYOUTS[layout]
    assert _instance(max(lens), H, len(lens)) == inst, "the layout no longer reaches its kernel instance"
    starts, rows = _seg_layout(lens, gaps)
    qkv, inseg = _seg_qkv(H, starts, lens, rows, seed=len(lens) * H)
    d = 64 * H
    sentinel = torch.full((rows, d), 0x3C5A, dtype=torch.int16, device="cuda")
    worst, nearest_wrong = 0.0, float("inf")
    for name, texts in [("nar", None)] + sorted(_seg_texts(lens).items()):
        out = eng.op_attention_segs(qkv, H, starts, lens, texts, out=sentinel.clone().view(torch.bfloat16))
        assert torch.equal(out.view(torch.int16)[~inseg], sentinel[~inseg]), f"{name}: a row outside the segments was written"
        o = out.double().reshape(rows, H, 64)
        for z, (s, n) in enumerate(zip(starts, lens)):
            t = None if texts is None else texts[z]
            ref, vbar = _seg_ref(qkv, H, s, n, t)
            unit = 2.0 ** -9 * (ref.abs() + vbar)
            err = ((o[s : s + n] - ref).abs() / unit).max().item()
            worst = max(worst, err)
            assert err <= SEG_BOUND, f"{name}: segment {z} (start {s}, len {n}, text {t}): error {err:.3f} units"
            # the nearest wrong answers: one more key (a poisoned row) without a mask; segment 0's causal mask in the mix
            wrong = None
            if texts is None:
                wrong = _seg_ref(qkv, H, s, n, None, nkeys=n + 1)[0]
            elif name == "mixed" and z > 0 and t >= 2:
                wrong = _seg_ref(qkv, H, s, n, texts[0])[0]
            if wrong is not None:
                dist = ((o[s : s + n] - wrong).abs() / unit).max().item()
                nearest_wrong = min(nearest_wrong, dist)
                assert dist > WRONG_MARGIN * SEG_BOUND, f"{name}: segment {z}: the wrong answer is only {dist:.2f} units away"
    print(f"\nattention_segs {layout} {inst}: worst {worst:.3f} units (bound {SEG_BOUND}), nearest wrong answer {nearest_wrong:.1f} units")


@pytest.mark.parametrize("n,H,inst", [(300, 4, (2, 2)), (1800, 16, (2, 2)), (4000, 16, (2, 1)), (9000, 16, (4, 1))])
@pytest.mark.parametrize("text", [-1, 128])
def test_attention_single_segment_equals_unsegmented(eng, n, H, inst, text):
    """One segment at row 0 (with poisoned rows after it) runs the same instance as the segment-free launch: bitwise equal."""
    assert _instance(n, H, 1) == inst
    qkv, _ = _seg_qkv(H, [0], [n], n + 64, seed=n + H)
    seg = eng.op_attention_segs(qkv, H, [0], [n], None if text < 0 else [text])
    plain = eng.op_attention(qkv[:n].contiguous(), H, text, mfma=True)
    assert torch.equal(seg[:n].view(torch.int16), plain.view(torch.int16))
