"""GPU: alignment (vx_op_attn_text_rows, vx_op_mono_path, vx_align, VALLE.align) against the fp64 restatement align_ref.py.

The engine bounds.  An error of delta on every score of a row changes each of its softmax probabilities by at most the factor
exp(2 delta) (once through the entry's own exponent, once through the sum), so |p - p64| <= (exp(2 delta) - 1) p64, and a
head-weighted map is off by at most sum_lh w_lh (exp(2 delta_lh(t)) - 1) P64_lh[t, s].  delta is what the project already asserts
for logits of the same scale (score_cases.py): FP32_AR_TOL absolute on fp32 engines, BF16_REL_TOL x the row's largest |score| on
bf16 engines.  1e-7 is added for the fp32 rounding of the stored probability itself."""
import ctypes as C

import numpy as np
import pytest
import torch

import align_ref as ar
import score_cases as sc
import score_ref as sr

pytestmark = pytest.mark.gpu

_MODELS = {}
_REF = {}


def _model(cfg, sd, precision, **kw):
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.models import VALLE, VALLF

    key = (repr(cfg), precision, tuple(sorted(kw.items())))
    if key not in _MODELS:
        kw.setdefault("max_text", 32)
        kw.setdefault("max_audio", 192)
        cls = VALLF if cfg.is_vallf else VALLE
        m = cls(cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers, norm_first=cfg.norm_first, add_prenet=cfg.add_prenet,
                prefix_mode=cfg.prefix_mode, share_embedding=cfg.share_embedding, nar_scale_factor=cfg.scale_factor,
                prepend_bos=cfg.prepend_bos, num_quantizers=cfg.num_quantizers, precision=precision, print_eos=False, **kw)
        m.load_state_dict(sd)
        _MODELS[key] = m.to("cuda:0").eval()
    return _MODELS[key]


def _ref(u):
    """(P64 (L, H, T, S), smax (L, H, T)) of an utterance of score_cases, computed once."""
    key = id(u)
    if key not in _REF:
        _REF[key] = ar.text_attention(sr.oracle(u["cfg"], u["sd"]), u["text"], u["codes"], u["P"])
    return _REF[key]


def _align(m, u, **kw):
    return m.align(u["x"].cuda(), u["x_lens"].cuda(), u["y"].cuda(), u["P"], **kw)


def _uniform(P64):
    L, H = P64.shape[:2]
    return torch.full((L, H), 1.0 / (L * H), dtype=torch.float64)


def _want_bound(P64, delta, w):
    """(reference map (T, S), bound (T, S)) of head weights w (L, H) and per-score errors delta (L, H, T) or a number."""
    delta = torch.as_tensor(delta, dtype=torch.float64)
    if delta.dim() == 0:
        delta = delta.expand(P64.shape[:3])
    want = (w[:, :, None, None] * P64).sum((0, 1))
    bound = (w[:, :, None, None] * torch.expm1(2 * delta)[..., None] * P64).sum((0, 1)) + 1e-7
    return want, bound


# ------------------------------------------------------------------------------------ case 1: the attention kernel
TEXT_LENS = (1, 7, 33)


def _rows_cases():
    from valle_amd.engine import ALIGN_TILE_ROWS as TR

    return (1, TR, TR + 1, 70)


def _operands(dtype, H, hd, text_len, rows, row0, causal, seed):
    """Random q / k in the layout the engine taps: causal -> packed (M, 3 d) rows, M = text_len + row0 + rows, q rows the last
    `rows`; else q (rows, d) and K in the memory layout (H, max_text, hd), max_text = text_len + 3 (the tail is NaN: never read).
    Returns (q tensor, k tensor, ldk, k_head_stride, q (H, rows, hd) and k (H, keys, hd) as fp64)."""
    g = torch.Generator().manual_seed(seed)
    d = H * hd
    if causal:
        M = text_len + row0 + rows
        qkv = torch.randn(M, 3 * d, generator=g).to(dtype)
        qkv[:, 2 * d :] = float("nan")  # V is not the tap's business
        q, k = qkv[M - rows :], qkv.flatten()[d:]
        q64 = qkv[M - rows :, :d].double().reshape(rows, H, hd).transpose(0, 1)
        k64 = qkv[:, d : 2 * d].double().reshape(M, H, hd).transpose(0, 1)
        return q.contiguous(), k.contiguous(), 3 * d, hd, q64, k64
    q = torch.randn(rows, d, generator=g).to(dtype)
    mem = torch.full((H, text_len + 3, hd), float("nan")).to(dtype)
    mem[:, :text_len] = torch.randn(H, text_len, hd, generator=g).to(dtype)
    return q, mem, hd, (text_len + 3) * hd, q.double().reshape(rows, H, hd).transpose(0, 1), mem[:, :text_len].double()


def _run_tap(q, k, ldk, khs, H, hd, text_len, causal, row0, c0, c1, w, first=True, prior=None, per_head=True):
    """Launches the kernel into NaN-poisoned buffers with a guard row on either side; returns (attn, mass, per_head) on the host."""
    from valle_amd.engine import op_attn_text_rows

    rows, Sw = q.shape[0], c1 - c0
    big = torch.full((rows + 2, Sw), float("nan"), device="cuda")
    bigm = torch.full((rows + 2,), float("nan"), device="cuda")
    bigp = torch.full((H * rows + 2, Sw), float("nan"), device="cuda") if per_head else None
    if prior is not None:
        big[1 : rows + 1] = prior[0].cuda()
        bigm[1 : rows + 1] = prior[1].cuda()
    ph = bigp[1 : H * rows + 1].view(H, rows, Sw) if per_head else None
    op_attn_text_rows(q.cuda(), k.cuda(), H, hd, text_len, causal, c0, c1, w.cuda(), big[1 : rows + 1], bigm[1 : rows + 1], ph,
                      first=first, row0=row0, ldk=ldk, k_head_stride=khs)
    torch.cuda.synchronize()
    big, bigm = big.cpu(), bigm.cpu()
    assert bool(torch.isnan(big[0]).all() and torch.isnan(big[-1]).all() and torch.isnan(bigm[0]) and torch.isnan(bigm[-1]))
    assert not bool(torch.isnan(big[1:-1]).any() or torch.isnan(bigm[1:-1]).any())
    if per_head:
        bigp = bigp.cpu()
        assert bool(torch.isnan(bigp[0]).all() and torch.isnan(bigp[-1]).all()) and not bool(torch.isnan(bigp[1:-1]).any())
        ph = bigp[1:-1].view(H, rows, Sw)
    return big[1:-1], bigm[1:-1], ph


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "memory"])
@pytest.mark.parametrize("dtype,hd", [(torch.float32, 64), (torch.float32, 4), (torch.bfloat16, 64)], ids=["fp32-hd64", "fp32-hd4", "bf16-hd64"])
def test_attn_text_rows_kernel_against_fp64(dtype, hd, causal):
    """Floor rule: the worst error against fp64 is at most 4 x that of the same formula in torch fp32 on the host, softmax(q k^T
    scale) on the same values (bf16 inputs are exact in both).  3 heads, one of weight zero; every text length x row count; the
    70-row causal case walks 70 + text_len keys, i.e. more than one 64-key LDS tile.  A window inside the text where it has room."""
    import __graft_entry__ as ge

    ge.build()
    H, row0 = 3, 2
    w = torch.tensor([0.25, 0.0, 0.75])
    worst_k = worst_t = worst_m = 0.0
    for text_len in TEXT_LENS:
        c0, c1 = (1, text_len - 1) if text_len >= 3 else (0, text_len)
        for rows in _rows_cases():
            q, k, ldk, khs, q64, k64 = _operands(dtype, H, hd, text_len, rows, row0, causal, seed=1000 * text_len + rows)
            p64 = ar.head_map(q64, k64, text_len, causal, row0)                                    # (H, rows, text_len)
            p32 = ar.head_map(q64.float(), k64.float(), text_len, causal, row0)                    # torch fp32, same values
            want = (w.double()[:, None, None] * p64).sum(0)
            floor = (w[:, None, None] * p32).sum(0)
            attn, mass, ph = _run_tap(q, k, ldk, khs, H, hd, text_len, causal, row0, c0, c1, w)
            worst_k = max(worst_k, float((attn.double() - want[:, c0:c1]).abs().max()), float((ph.double() - p64[:, :, c0:c1]).abs().max()))
            worst_t = max(worst_t, float((floor.double() - want)[:, c0:c1].abs().max()), float((p32.double() - p64)[:, :, c0:c1].abs().max()))
            worst_m = max(worst_m, float((mass.double() - want.sum(-1)).abs().max()))
            if not causal:
                assert float((mass - 1.0).abs().max()) <= 1e-5
            if rows == 70:
                # a row's result does not depend on the launch: rows 5 .. 39 by themselves, bit for bit
                sub = slice(5, 40)
                if causal:
                    M = text_len + row0 + rows
                    qs, ks = q[sub], k[: (M - rows + 40) * ldk - H * hd]  # the keys those rows may see, no more
                    a2, m2, p2 = _run_tap(qs.contiguous(), ks.contiguous(), ldk, khs, H, hd, text_len, True, row0 + 5, c0, c1, w)
                else:
                    a2, m2, p2 = _run_tap(q[sub].contiguous(), k, ldk, khs, H, hd, text_len, False, 0, c0, c1, w)
                assert torch.equal(a2.view(torch.int32), attn[sub].view(torch.int32)) and torch.equal(m2.view(torch.int32), mass[sub].view(torch.int32))
                assert torch.equal(p2.view(torch.int32), ph[:, sub].view(torch.int32))
                # first = 0 adds to what is there, one fp32 addition per cell; without per_head the zero-weight head is skipped
                prior = (torch.randn(rows, c1 - c0), torch.randn(rows))
                a3, m3, _ = _run_tap(q, k, ldk, khs, H, hd, text_len, causal, row0, c0, c1, w, first=False, prior=prior, per_head=False)
                assert torch.equal(a3.view(torch.int32), (prior[0] + attn).view(torch.int32)) and torch.equal(m3.view(torch.int32), (prior[1] + mass).view(torch.int32))
    print(f"attn_text_rows {dtype} hd={hd} causal={causal}: kernel worst |err| {worst_k:.3e}, torch fp32 {worst_t:.3e}, "
          f"ratio {worst_k / max(worst_t, 1e-300):.3f}; text mass worst |err| {worst_m:.3e}")
    assert worst_k <= 4 * worst_t
    # the mass is a sum of at most 33 probabilities, each within a few ulp, of total at most 1: (a few + log2 33) x 2^-24 < 2e-6
    assert worst_m <= 2e-6


# ------------------------------------------------------------------------------------------- case 2: the path kernel
def _gpu_path(a):
    from valle_amd.engine import op_mono_path

    path, score = op_mono_path(torch.as_tensor(a, dtype=torch.float32).cuda().contiguous())
    torch.cuda.synchronize()
    return path.cpu().numpy().astype(np.int64), float(score.cpu()[0])


def _check_path(a, path, score):
    """Rule 2: a valid path whose score is the optimum of align_ref.mono_path within 1e-9 relative (fp64 rounding over a few
    hundred additions is ~1e-13; the margin covers the device log being within an ulp of numpy's), and the returned score is
    that of the returned path."""
    T, Sw = a.shape
    _, best = ar.mono_path(a)
    assert ar.valid_path(path, T, Sw)
    got = ar.path_score(a, path)
    assert abs(got - best) <= 1e-9 * abs(best) and abs(score - got) <= 1e-9 * abs(got)


@pytest.mark.parametrize("T,Sw", [(1, 1), (5, 5), (6, 5), (70, 7), (300, 65)])
def test_mono_path_kernel(T, Sw):
    import __graft_entry__ as ge

    ge.build()
    rng = np.random.default_rng(T * 100 + Sw)
    a = rng.random((T, Sw)).astype(np.float32)
    a[rng.random((T, Sw)) < 0.1] = 0.0  # clamped at FLT_MIN
    _check_path(a, *_gpu_path(a))
    # all equal: every advance as early as it can (ties stay); exact
    path, _ = _gpu_path(np.full((T, Sw), 0.125, dtype=np.float32))
    assert path.tolist() == [min(t, Sw - 1) for t in range(T)]
    # diagonal-dominant: token j spoken over frames [j T / Sw, (j + 1) T / Sw)
    want = (np.arange(T) * Sw) // T
    dom = np.full((T, Sw), 1e-3, dtype=np.float32)
    dom[np.arange(T), want] = 0.9
    path, score = _gpu_path(dom)
    assert path.tolist() == want.tolist() and score == pytest.approx(T * float(np.log(np.float64(np.float32(0.9)))), rel=1e-9)


def test_mono_path_kernel_without_a_path():
    path, score = _gpu_path(np.random.default_rng(0).random((4, 6)).astype(np.float32))
    assert path.tolist() == [-1] * 4 and score == float("-inf")


# ------------------------------------------------------------------------------- case 3: fp32 engine against the oracle
CONFIGS = {
    "default": dict(),
    "bos": dict(prepend_bos=True),
    "postnorm": dict(norm_first=False),
    "prenet": dict(add_prenet=True),
    "reftest": dict(decoder_dim=64, nhead=16, num_decoder_layers=4),  # the reference's own test geometry: head_dim 4
    "vallf": dict(model_name="VALL-F", prepend_bos=True),
}


def _check_engine(u, al, delta, w=None, label=""):
    P64, _ = _ref(u)
    w = _uniform(P64) if w is None else w.double()
    want, bound = _want_bound(P64, delta, w)
    err = (al.attn.cpu().double() - want).abs()
    merr = (al.text_mass.cpu().double() - want.sum(-1)).abs()
    ratio = float((err / bound).max())
    print(f"{label}: attn worst err / bound {ratio:.4f} (worst |err| {float(err.max()):.3e}), text mass {float((merr / bound.sum(-1)).max()):.4f}")
    assert bool((err <= bound).all()) and bool((merr <= bound.sum(-1)).all())
    return ratio


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fp32_engine_align_matches_oracle(name):
    u = sc.utterance(sc.config(**CONFIGS[name]))
    m = _model(u["cfg"], u["sd"], "fp32")
    al = _align(m, u)
    T, S = u["codes"].shape[0] - u["P"], u["text"].shape[0]
    assert tuple(al.attn.shape) == (T, S) and tuple(al.text_mass.shape) == (T,) and al.attn.dtype == torch.float32
    _check_engine(u, al, sc.FP32_AR_TOL, label=f"fp32 {name}")
    if u["cfg"].is_vallf:
        assert float((al.text_mass.cpu() - 1.0).abs().max()) <= 1e-5
    else:
        assert float(al.text_mass.max()) < 1.0
    assert torch.equal(al.token_mass, al.attn.sum(0))


# --------------------------------------------------------------------------------------------------- case 4: bf16
def test_bf16_engine_align_matches_oracle_and_the_bound_is_not_vacuous():
    """bf16: delta_lh(t) = BF16_REL_TOL x the fp64 largest |score| of that head and row.  For these inputs exp(2 delta) - 1 is at
    most 0.13 - 0.20, so the bound could hide a wrong layer unless maps of different layers differ by more: the engine's layer-0
    map is held against the fp64 map of layer 1 and must violate the bound on at least half of the entries.
    Measured on the MI355X: worst error / bound 0.036 for the map, 0.011 for the text mass."""
    u = sc.utterance(sc.config())
    P64, smax = _ref(u)
    m = _model(u["cfg"], u["sd"], "bf16")
    delta = sc.BF16_REL_TOL * smax
    print(f"bf16: exp(2 delta) - 1 at most {float(torch.expm1(2 * delta).max()):.3f}")
    _check_engine(u, _align(m, u), delta, label="bf16 default")
    L, H = P64.shape[:2]
    w1 = torch.zeros(L, H, dtype=torch.float64)
    w1[1] = 1.0 / H
    want1, bound1 = _want_bound(P64, delta, w1)
    a0 = _align(m, u, heads=[(0, h) for h in range(H)]).attn.cpu().double()
    outside = float(((a0 - want1).abs() > bound1).float().mean())
    print(f"bf16 guard: the layer-0 map violates layer 1's bound on {outside:.3f} of the entries")
    assert outside >= 0.5
    w0 = torch.zeros(L, H, dtype=torch.float64)
    w0[0] = 1.0 / H
    want0, bound0 = _want_bound(P64, delta, w0)
    assert bool(((a0 - want0).abs() <= bound0).all())


def test_fp8nar_engine_aligns_like_bf16():
    """fp8nar touches the NAR stages only: its AR stack, and so its alignment, is the bf16 engine's bit for bit."""
    u = sc.utterance(sc.config())
    a = _align(_model(u["cfg"], u["sd"], "bf16"), u)
    b = _align(_model(u["cfg"], u["sd"], "fp8nar"), u)
    assert torch.equal(a.attn, b.attn) and torch.equal(a.path, b.path)


# ------------------------------------------------------------------------------------------ case 5: head selection
@pytest.mark.parametrize("name", ["default", "vallf"])
def test_head_selection(name):
    u = sc.utterance(sc.config(**CONFIGS[name]))
    m = _model(u["cfg"], u["sd"], "fp32")
    full = _align(m, u, per_head=True)
    L, H = u["cfg"].num_decoder_layers, u["cfg"].nhead
    T, S = full.attn.shape
    assert tuple(full.per_head.shape) == (L, H, T, S)
    P64, _ = _ref(u)
    assert float((full.per_head.cpu().double() - P64).abs().max()) <= float(np.expm1(2 * sc.FP32_AR_TOL)) + 1e-7
    one = _align(m, u, heads=[(1, 2)])
    assert torch.equal(one.attn.view(torch.int32), full.per_head[1, 2].view(torch.int32))
    assert float((full.attn - full.per_head.mean((0, 1))).abs().max()) <= 1e-6
    wt = torch.tensor([[1.0, 0.0, 2.0, 0.0], [0.0, 0.0, 0.0, 5.0]])
    a = _align(m, u, heads=wt)
    b = _align(m, u, heads=wt * 7.0)  # normalised: the scale of the tensor does not matter (7 x is exact in the ratio's rounding)
    want = (wt[:, :, None, None].cuda() / 8.0 * full.per_head).sum((0, 1))
    assert float((a.attn - want).abs().max()) <= 1e-6 and float((a.attn - b.attn).abs().max()) <= 1e-6
    again = _align(m, u, heads=wt)
    assert torch.equal(a.attn.view(torch.int32), again.attn.view(torch.int32)) and torch.equal(a.text_mass.view(torch.int32), again.text_mass.view(torch.int32))
    full2 = _align(m, u, per_head=True)
    assert torch.equal(full.attn.view(torch.int32), full2.attn.view(torch.int32)) and torch.equal(full.per_head.view(torch.int32), full2.per_head.view(torch.int32))
    assert torch.equal(full.path, full2.path) and full.path_score == full2.path_score


# ------------------------------------------------------------------------------------- case 6: the engine's path
@pytest.mark.parametrize("name", ["default", "vallf"])
def test_engine_path_and_spans(name):
    u = sc.utterance(sc.config(**CONFIGS[name]))
    al = _align(_model(u["cfg"], u["sd"], "fp32"), u)
    a = al.attn.cpu().numpy()
    T, S = a.shape
    _check_path(a, al.path.cpu().numpy().astype(np.int64), al.path_score)
    sp = al.spans.cpu()
    assert sp.dtype == torch.int32 and tuple(sp.shape) == (S, 2)
    assert int(sp[0, 0]) == 0 and int(sp[-1, 1]) == T and torch.equal(sp[1:, 0], sp[:-1, 1]) and bool((sp[:, 1] > sp[:, 0]).all())
    for j in range(S):
        assert bool((al.path[int(sp[j, 0]) : int(sp[j, 1])] == j).all())
    assert torch.allclose(al.seconds.cpu(), sp.float() / 75.0)


def test_engine_window_after_a_transcribed_prompt_and_no_path():
    """enroll_x_lens = 3 of S = 7: columns [3, 7) of the full map, bit for bit (the softmax still runs over every key).  With
    more window tokens than frames there is no path, which is a result, not an error."""
    u = sc.utterance(sc.config())
    m = _model(u["cfg"], u["sd"], "fp32")
    full = _align(m, u)
    win = _align(m, u, enroll_x_lens=torch.tensor([3]))
    assert tuple(win.attn.shape) == (full.attn.shape[0], 4)
    assert torch.equal(win.attn.view(torch.int32), full.attn[:, 3:].contiguous().view(torch.int32))
    assert torch.equal(win.text_mass.view(torch.int32), full.text_mass.view(torch.int32))
    A = u["codes"].shape[0]
    short = m.align(u["x"].cuda(), u["x_lens"].cuda(), u["y"].cuda(), A - 4)  # T = 4 frames for 7 tokens
    assert short.path is None and short.spans is None and short.path_score == float("-inf")
    assert torch.equal(short.attn.view(torch.int32), full.attn[-4:].contiguous().view(torch.int32))  # the same rows of the same pass


# -------------------------------------------------------------------------------------- case 7: nothing else moves
def test_align_leaves_inference_and_score_alone():
    u = sc.utterance(sc.config())
    m = _model(u["cfg"], u["sd"], "bf16")
    x, xl, y = u["x"].cuda(), u["x_lens"].cuda(), u["y"][:, :8].cuda()

    def gen(**kw):
        torch.manual_seed(5)
        return m.inference(x, xl, y, None, top_k=10, max_new_tokens=24, **kw)

    c0 = gen()
    s0 = m.score(x, xl, u["y"].cuda(), prompt_frames=u["P"])
    al = _align(m, u)
    c1 = gen()
    s1 = m.score(x, xl, u["y"].cuda(), prompt_frames=u["P"])
    assert torch.equal(c0, c1) and c0.shape[1] == 24
    assert torch.equal(s0.ar_nll, s1.ar_nll) and torch.equal(s0.ar_rank, s1.ar_rank) and torch.equal(s0.nar_nll, s1.nar_nll)
    codes, al2 = gen(return_alignment=True)
    assert torch.equal(codes, c0)
    want = m.align(x, xl, torch.cat([y, codes], 1), 8)
    assert torch.equal(al2.attn.view(torch.int32), want.attn.view(torch.int32)) and torch.equal(al2.path, want.path)
    assert tuple(al2.attn.shape) == (24, u["text"].shape[0])
    al3 = _align(m, u)  # and alignment does not depend on what ran before it
    assert torch.equal(al.attn.view(torch.int32), al3.attn.view(torch.int32))


def test_align_on_a_batched_engine():
    u = sc.utterance(sc.config())
    a = _align(_model(u["cfg"], u["sd"], "bf16"), u)
    b = _align(_model(u["cfg"], u["sd"], "bf16", max_batch=4), u)
    assert torch.equal(a.attn.view(torch.int32), b.attn.view(torch.int32)) and torch.equal(a.text_mass, b.text_mass) and torch.equal(a.path, b.path)


# ---------------------------------------------------------------------------------------- case 8: errors at the C ABI
def test_align_errors_at_the_c_abi():
    u = sc.utterance(sc.config())
    m = _model(u["cfg"], u["sd"], "fp32")
    e = m.engine()
    text, codes = u["text"], u["codes"].contiguous()
    out = torch.empty(70 * 7, dtype=torch.float32, device="cuda")
    L, H = u["cfg"].num_decoder_layers, u["cfg"].nhead

    def call(S=7, A=70, P=5, c0=0, c1=7, hw=None):
        return e.lib.vx_align(e.h, text.data_ptr(), S, codes.data_ptr(), A, P, c0, c1, None if hw is None else hw.data_ptr(),
                              out.data_ptr(), None, None, None, None, None)

    neg = torch.full((L, H), 0.1)
    neg[1, 1] = -0.1
    nan = torch.full((L, H), 0.1)
    nan[0, 3] = float("nan")
    for kw, code, match in [(dict(c0=3, c1=3), 1, "window"), (dict(c1=8), 1, "window"), (dict(c0=-1), 1, "window"),
                            (dict(hw=torch.zeros(L, H)), 1, "all zero"), (dict(hw=neg), 1, "head_w[5]"), (dict(hw=nan), 1, "head_w[3]"),
                            (dict(A=192), 4, "capacity"), (dict(P=0), 1, "prepend_bos"), (dict(P=70), 1, "P=70")]:
        assert call(**kw) == code and match.encode() in e.lib.vx_last_error(), (kw, e.lib.vx_last_error())
        assert call() == 0  # each error leaves the engine usable
    torch.cuda.synchronize()
    al = _align(m, u)
    assert torch.equal(out[: 65 * 7].view(65, 7).view(torch.int32), al.attn.view(torch.int32))
