"""GPU: batched alignment (vx_op_attn_text_segs, vx_op_mono_path_segs, vx_align_batch, VALLE.align_batch, alignment from
inference_batch / inference_stream, best-of-N ranked by alignment) against the fp64 restatement align_ref.py.  The bounds are those
of test_gpu_align.py, whose helpers are imported."""
import numpy as np
import pytest
import torch

import align_ref as ar
import score_cases as sc
from test_gpu_align import _check_engine, _check_path, _model, _ref, _want_bound

pytestmark = pytest.mark.gpu

CAP = dict(max_text=48, max_audio=192)
I32 = torch.int32


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(I32), b.contiguous().view(I32))


# ------------------------------------------------------------------------------------ case 1: the tap kernel
H, HD = 3, 64
D = H * HD
W = torch.tensor([0.25, 0.0, 0.75])


def _segments(shapes, seed):
    """Packed (M, 3 d) bf16 rows of the segments `shapes` = [(text_len, row0, rows)], each starting at a multiple of 64 rows; the
    tapped rows of a segment are its last `rows`.  V columns and the pad rows between (and after) the segments are NaN.  Returns
    (qkv, [dict(start, text_len, qfirst, rows, row0, c0, c1, q64 (H, rows, hd), k64 (H, keys, hd))])."""
    g = torch.Generator().manual_seed(seed)
    segs, start = [], 0
    for text_len, row0, rows in shapes:
        keys = text_len + row0 + rows
        c0, c1 = (1, text_len - 1) if text_len >= 3 else (0, text_len)  # strictly inside the text where it has room
        segs.append(dict(start=start, text_len=text_len, qfirst=text_len + row0, rows=rows, row0=row0, c0=c0, c1=c1, keys=keys))
        start += (keys + 63) // 64 * 64
    qkv = torch.full((start, 3 * D), float("nan")).to(torch.bfloat16)
    for s in segs:
        blk = torch.randn(s["keys"], 2 * D, generator=g).to(torch.bfloat16)
        qkv[s["start"] : s["start"] + s["keys"], : 2 * D] = blk
        s["blk"] = blk
        s["q64"] = blk[s["qfirst"] :, :D].double().reshape(s["rows"], H, HD).transpose(0, 1)
        s["k64"] = blk[:, D:].double().reshape(s["keys"], H, HD).transpose(0, 1)
    return qkv, segs


def _launch(qkv, segs, first=True, prior=None):
    """One launch into NaN-poisoned outputs with a guard row before, between and after the segments' cells and rows; returns
    ([attn (rows, Sw)], [mass (rows,)]) on the host after checking that nothing but the cells was written."""
    from valle_amd.engine import op_attn_text_segs

    desc, cell, row = [], 0, 0
    for s in segs:
        Sw = s["c1"] - s["c0"]
        cell += Sw  # guard row
        row += 1
        desc.append((s["start"], s["text_len"], s["qfirst"], s["rows"], s["row0"], s["c0"], s["c1"], cell, row))
        cell += s["rows"] * Sw
        row += s["rows"]
    cell += segs[-1]["c1"] - segs[-1]["c0"]
    row += 1
    attn = torch.full((cell,), float("nan"), device="cuda")
    mass = torch.full((row,), float("nan"), device="cuda")
    live_a, live_m = torch.zeros(cell, dtype=torch.bool), torch.zeros(row, dtype=torch.bool)
    for z, (s, d) in enumerate(zip(segs, desc)):
        n = s["rows"] * (s["c1"] - s["c0"])
        live_a[d[7] : d[7] + n] = True
        live_m[d[8] : d[8] + s["rows"]] = True
        if prior is not None:
            attn[d[7] : d[7] + n] = prior[z][0].flatten().cuda()
            mass[d[8] : d[8] + s["rows"]] = prior[z][1].cuda()
    op_attn_text_segs(qkv.cuda(), H, desc, W.cuda(), attn, mass, first=first)
    torch.cuda.synchronize()
    attn, mass = attn.cpu(), mass.cpu()
    assert torch.equal(torch.isnan(attn), ~live_a) and torch.equal(torch.isnan(mass), ~live_m)  # guards intact, every cell written
    return ([attn[d[7] : d[7] + s["rows"] * (s["c1"] - s["c0"])].view(s["rows"], -1) for s, d in zip(segs, desc)],
            [mass[d[8] : d[8] + s["rows"]] for s, d in zip(segs, desc)])


def _alone(s):
    """The segment by itself: its own rows at start 0, nothing after them."""
    qkv = torch.full((s["keys"], 3 * D), float("nan")).to(torch.bfloat16)
    qkv[:, : 2 * D] = s["blk"]
    return qkv, [dict(s, start=0)]


def test_attn_text_seg_kernel_against_fp64():
    """Floor rule of test_attn_text_rows_kernel_against_fp64: the worst error against fp64 is at most 4 x that of the same formula
    in torch fp32 on the host on the same bf16 values.  3 heads, one of weight zero (its scratch stays NaN: it must not be read).
    Launch 1: three segments, 1 / 33 / 70 tapped rows (one row; one over a wave; two workgroups).  Launch 2: 32 and 129 rows (a
    full wave; two full workgroups and one row, whose last row sees 202 keys, more than three 64-key tiles).  V, the pad rows and
    the guards around the outputs are NaN.  Each segment alone gives the bits it gives in the batch, a repeated launch too, and
    first = 0 adds one fp32 addition per cell.
    Measured on the MI355X: worst |err| 3.3e-8 against 5.5e-8 for torch fp32, ratio 0.61; text mass within 7.1e-8."""
    import __graft_entry__ as ge

    ge.build()
    worst_k = worst_t = worst_m = 0.0
    for shapes, seed in (([(1, 2, 1), (7, 2, 33), (33, 2, 70)], 11), ([(7, 2, 32), (33, 40, 129)], 12)):
        qkv, segs = _segments(shapes, seed)
        attn, mass = _launch(qkv, segs)
        for s, a, m in zip(segs, attn, mass):
            c0, c1 = s["c0"], s["c1"]
            p64 = ar.head_map(s["q64"], s["k64"], s["text_len"], True, s["row0"])                  # (H, rows, text_len)
            p32 = ar.head_map(s["q64"].float(), s["k64"].float(), s["text_len"], True, s["row0"])  # torch fp32, same values
            want = (W.double()[:, None, None] * p64).sum(0)
            floor = (W[:, None, None] * p32).sum(0)
            worst_k = max(worst_k, float((a.double() - want[:, c0:c1]).abs().max()))
            worst_t = max(worst_t, float((floor.double() - want)[:, c0:c1].abs().max()))
            worst_m = max(worst_m, float((m.double() - want.sum(-1)).abs().max()))
            a1, m1 = _launch(*_alone(s))
            assert _bits(a1[0], a) and _bits(m1[0], m), s["rows"]
        again = _launch(qkv, segs)
        assert all(_bits(x, y) for x, y in zip(again[0], attn)) and all(_bits(x, y) for x, y in zip(again[1], mass))
        g = torch.Generator().manual_seed(seed + 100)
        prior = [(torch.randn(a.shape, generator=g), torch.randn(m.shape, generator=g)) for a, m in zip(attn, mass)]
        a3, m3 = _launch(qkv, segs, first=False, prior=prior)
        for z in range(len(segs)):
            assert _bits(a3[z], prior[z][0] + attn[z]) and _bits(m3[z], prior[z][1] + mass[z])
    print(f"attn_text_segs bf16 hd=64: kernel worst |err| {worst_k:.3e}, torch fp32 {worst_t:.3e}, "
          f"ratio {worst_k / max(worst_t, 1e-300):.3f}; text mass worst |err| {worst_m:.3e}")
    assert worst_k <= 4 * worst_t
    # the mass is a sum of at most 33 probabilities, each within a few ulp, of total at most 1: (a few + log2 33) x 2^-24 < 2e-6
    assert worst_m <= 2e-6


# ------------------------------------------------------------------------------------------- case 2: the path kernel
def test_mono_path_seg_kernel():
    from valle_amd.engine import op_mono_path, op_mono_path_segs

    import __graft_entry__ as ge

    ge.build()
    shapes = [(1, 1), (6, 5), (70, 7), (300, 65), (4, 9)]
    rng = np.random.default_rng(7)
    maps, desc, off = [], [], 3  # a gap before, between and after the maps
    for T, Sw in shapes:
        a = rng.random((T, Sw)).astype(np.float32)
        a[rng.random((T, Sw)) < 0.1] = 0.0  # clamped at FLT_MIN
        maps.append(a)
        desc.append((T, Sw, off))
        off += T * Sw + 5
    flat = torch.full((off,), float("nan"))
    for a, (T, Sw, o) in zip(maps, desc):
        flat[o : o + T * Sw] = torch.from_numpy(a).flatten()
    paths, scores = op_mono_path_segs(flat.cuda(), desc)
    torch.cuda.synchronize()
    for z, (a, (T, Sw, _)) in enumerate(zip(maps, desc)):
        p1, s1 = op_mono_path(torch.from_numpy(a).cuda())
        torch.cuda.synchronize()
        assert torch.equal(paths[z], p1) and float(scores[z]) == float(s1[0]), (T, Sw)  # what the map gives alone
        if T < Sw:
            assert paths[z].tolist() == [-1] * T and float(scores[z]) == float("-inf")
        else:
            _check_path(a, paths[z].cpu().numpy().astype(np.int64), float(scores[z]))


# ------------------------------------------------------------------------------------------------- case 3: the engine
SHAPES = [(7, 70, 5), (1, 34, 1), (33, 140, 40)]


def _utts():
    cfg = sc.config()
    return cfg, [sc.utterance(cfg, S, A, P) for S, A, P in SHAPES]


def _args(us):
    return [(u["x"].cuda(), u["x_lens"].cuda(), u["y"].cuda()) for u in us], [u["P"] for u in us]


def test_bf16_engine_align_batch_matches_oracle_and_the_bound_is_not_vacuous():
    """Three utterances in one vx_align_batch (segments of 77, 35 and 173 rows; 65, 33 and 100 tapped rows): each map and text mass
    under the bf16 bound of test_gpu_align.py (delta = BF16_REL_TOL x the fp64 largest |score| of the head and row), the guard of
    that test repeated (the layer-0 map violates layer 1's bound on at least half of the entries), each path the host programme's
    on the engine's own map.  Measured on the MI355X: worst error / bound 0.036 / 0.030 / 0.036 for the three maps, 0.030 at most for
    the text mass; the guard 0.84."""
    cfg, us = _utts()
    m = _model(cfg, us[0]["sd"], "bf16", **CAP)
    utts, Ps = _args(us)
    als = m.align_batch(utts, Ps)
    assert len(als) == 3
    for i, (u, al) in enumerate(zip(us, als)):
        S, A, P = SHAPES[i]
        assert tuple(al.attn.shape) == (A - P, S) and tuple(al.text_mass.shape) == (A - P,) and al.attn.dtype == torch.float32
        _, smax = _ref(u)
        _check_engine(u, al, sc.BF16_REL_TOL * smax, label=f"bf16 align_batch {SHAPES[i]}")
        _check_path(al.attn.cpu().numpy(), al.path.cpu().numpy().astype(np.int64), al.path_score)
        assert torch.equal(al.token_mass, al.attn.sum(0)) and tuple(al.spans.shape) == (S, 2)
    # the same bits when the call is repeated, and for an utterance by itself
    again = m.align_batch(utts, Ps)
    assert all(_bits(a.attn, b.attn) and _bits(a.text_mass, b.text_mass) and torch.equal(a.path, b.path) for a, b in zip(als, again))
    solo = m.align_batch(utts[2:], Ps[2:])[0]
    assert _bits(solo.attn, als[2].attn) and _bits(solo.text_mass, als[2].text_mass) and solo.path_score == als[2].path_score
    # the guard
    u = us[0]
    P64, smax = _ref(u)
    delta = sc.BF16_REL_TOL * smax
    L, Hn = P64.shape[:2]
    a0 = m.align_batch(utts[:1], Ps[:1], heads=[(0, h) for h in range(Hn)])[0].attn.cpu().double()
    for layer, inside in ((1, False), (0, True)):
        w = torch.zeros(L, Hn, dtype=torch.float64)
        w[layer] = 1.0 / Hn
        want, bound = _want_bound(P64, delta, w)
        if inside:
            assert bool(((a0 - want).abs() <= bound).all())
        else:
            outside = float(((a0 - want).abs() > bound).float().mean())
            print(f"bf16 guard: the layer-0 map violates layer 1's bound on {outside:.3f} of the entries")
            assert outside >= 0.5


def test_align_batch_head_selection_fp8nar_and_a_batched_engine():
    cfg, us = _utts()
    m = _model(cfg, us[0]["sd"], "bf16", **CAP)
    utts, Ps = _args(us)
    als = m.align_batch(utts, Ps)
    one = m.align_batch(utts, Ps, heads=[(1, 2)])
    for u, al, full in zip(us, one, als):
        P64, smax = _ref(u)
        w = torch.zeros(P64.shape[:2], dtype=torch.float64)
        w[1, 2] = 1.0
        _check_engine(u, al, sc.BF16_REL_TOL * smax, w=w, label="bf16 align_batch head (1, 2)")
        assert not torch.equal(al.attn, full.attn)
    # fp8nar touches the NAR stages only; an engine with 4 slots serves the call as the batch-1 engine does (vx_align_batch itself,
    # not the fallback: the engine call raises where it is refused)
    for kw in (dict(precision="fp8nar"), dict(precision="bf16", max_batch=4)):
        m2 = _model(cfg, us[0]["sd"], kw.pop("precision"), **CAP, **kw)
        e2 = m2.engine()
        parts = e2.align_batch([u["text"] for u in us], [u["codes"] for u in us], Ps)
        for (attn, mass, path, score), al in zip(parts, als):
            assert _bits(attn, al.attn) and _bits(mass, al.text_mass) and torch.equal(path, al.path) and float(score) == al.path_score
        assert e2.align_ms() > 0


def test_align_batch_leaves_decode_state_alone():
    cfg, us = _utts()
    m = _model(cfg, us[0]["sd"], "bf16", max_batch=2, **CAP)
    e = m.engine()
    utts, Ps = _args(us)
    x, xl, y = utts[0][0], utts[0][1], utts[0][2][:, :8]

    def gen():
        torch.manual_seed(5)
        return m.inference(x, xl, y, None, top_k=10, max_new_tokens=24)

    c0 = gen()
    s0 = m.score(x, xl, utts[0][2], prompt_frames=Ps[0])
    als = m.align_batch(utts, Ps)
    c1 = gen()
    s1 = m.score(x, xl, utts[0][2], prompt_frames=Ps[0])
    assert torch.equal(c0, c1) and c0.shape[1] == 24
    assert torch.equal(s0.ar_nll, s1.ar_nll) and torch.equal(s0.ar_rank, s1.ar_rank) and torch.equal(s0.nar_nll, s1.nar_nll)

    def session(with_align):
        e.batch_open()
        # slot 0 stops after 5 steps: batch_run(1) returns there, slot 1 mid-utterance (the S = 33 one: 24 is under its length stop)
        for slot, i, new in ((0, 0, 5), (1, 2, 24)):
            e.batch_admit([slot], [us[i]["text"]], [us[i]["codes"][:8, 0].contiguous()], top_k=5, seeds=[11 + slot], max_new_tokens=new)
        assert e.batch_run(1) == [0]
        a, _ = e.batch_result(0)
        al = m.align_batch(utts, Ps) if with_align else None
        assert e.batch_run(1) == [1]
        b, _ = e.batch_result(1)
        return a, b, al

    a0, b0, _ = session(False)
    a1, b1, inside = session(True)
    assert a0.numel() == 5 and b0.numel() == 24 and torch.equal(a0, a1) and torch.equal(b0, b1)
    assert all(_bits(p.attn, q.attn) and torch.equal(p.path, q.path) for p, q in zip(inside, als))  # nor does it depend on the session


# ------------------------------------------------------------------------------------------------- case 4: fallback
def test_align_batch_falls_back_to_align_where_the_engine_refuses():
    """fp32 and VALL-F: align_batch is the loop of align, bit for bit, and vx_align_batch itself answers VX_ERR_UNSUPPORTED."""
    from valle_amd.engine import VxError

    cfg, us = _utts()
    utts, Ps = _args(us)
    m = _model(cfg, us[0]["sd"], "fp32", **CAP)
    cfg_f = sc.config(model_name="VALL-F", prepend_bos=True)
    uf = [sc.utterance(cfg_f, S, A, P) for S, A, P in SHAPES[:2]]
    mf = _model(cfg_f, uf[0]["sd"], "fp32", **CAP)
    for model, ul in ((m, us), (mf, uf)):
        ut, ps = _args(ul)
        got = model.align_batch(ut, ps)
        for (x, xl, y), p, al in zip(ut, ps, got):
            want = model.align(x, xl, y, p)
            assert _bits(al.attn, want.attn) and _bits(al.text_mass, want.text_mass) and torch.equal(al.path, want.path)
            assert al.path_score == want.path_score
        with pytest.raises(VxError) as ei:
            model.engine().align_batch([u["text"] for u in ul], [u["codes"] for u in ul], ps)
        assert ei.value.code == 5 and "vx_align_batch" in str(ei.value)


def test_align_batch_errors_at_the_c_abi():
    import ctypes as C

    cfg, us = _utts()
    m = _model(cfg, us[0]["sd"], "bf16", **CAP)
    e = m.engine()
    texts = [u["text"].contiguous() for u in us]
    long_text = torch.zeros(49, dtype=torch.int64)
    codes = [u["codes"].contiguous() for u in us]
    outs = [torch.empty((A - P) * S, dtype=torch.float32, device="cuda") for S, A, P in SHAPES]

    def call(n=3, S=None, P=None, c0=None, c1=None, text=None):
        S = list(S or [s[0] for s in SHAPES])
        n_ = max(n, 3)
        rep = lambda v: (list(v) * ((n_ + 2) // 3))[:n_]
        ptrs = lambda ts: (C.c_void_p * n_)(*[t.data_ptr() for t in rep(ts)])
        ints = lambda vs: (C.c_int32 * n_)(*rep(vs))
        return e.lib.vx_align_batch(e.h, n, ptrs(text or texts), ints(S), ptrs(codes), ints([s[1] for s in SHAPES]),
                                    ints(P or [s[2] for s in SHAPES]), ints(c0 or [0, 0, 0]), ints(c1 or S), None, ptrs(outs), None, None,
                                    None, None)

    for kw, code, match in [(dict(c0=[0, 0, 5], c1=[7, 1, 5]), 1, "window"), (dict(c1=[7, 2, 33]), 1, "(utterance 1)"),
                            (dict(c0=[0, 0, -1]), 1, "(utterance 2)"), (dict(P=[5, 0, 40]), 1, "prepend_bos"),
                            (dict(P=[5, 0, 40]), 1, "(utterance 1)"), (dict(n=65), 1, "1..64"), (dict(n=0), 1, "1..64"),
                            (dict(S=[7, 1, 49], text=[texts[0], texts[1], long_text]), 4, "(utterance 2)")]:
        assert call(**kw) == code and match.encode() in e.lib.vx_last_error(), (kw, e.lib.vx_last_error())
        assert call() == 0  # each error leaves the engine usable
    torch.cuda.synchronize()
    for out, al, (S, A, P) in zip(outs, m.align_batch(*_args(us)), SHAPES):
        assert _bits(out.view(A - P, S), al.attn)


# ------------------------------------------------------------------------------------------------- case 5: generation
def _gen_model(**kw):
    from valle_amd.weights import synthetic_inputs

    cfg = sc.config()
    m = _model(cfg, sc.utterance(cfg)["sd"], "bf16", max_batch=4, logprobs=True, **CAP, **kw)
    us = []
    for i, (S, P) in enumerate([(3, 6), (5, 9), (4, 12)]):  # 49, 81 and 65 generated frames (16 S + 1)
        x, xl, y = synthetic_inputs(S, P, cfg.num_quantizers, seed=20 + i)
        us.append((x.cuda(), xl.cuda(), y.cuda()))
    return m, us


def _same_alignment(a, b):
    return _bits(a.attn, b.attn) and _bits(a.text_mass, b.text_mass) and torch.equal(a.path, b.path) and a.path_score == b.path_score


def test_inference_batch_and_stream_return_alignment():
    m, us = _gen_model()
    seeds = [5, 6, 7]
    plain = m.inference_batch(us, top_k=20, seeds=seeds)
    got = m.inference_batch(us, top_k=20, seeds=seeds, return_alignment=True)
    both = m.inference_batch(us, top_k=20, seeds=seeds, return_alignment=True, return_logprobs=True)
    full = [(x, xl, torch.cat([y, c], 1)) for (x, xl, y), c in zip(us, plain)]
    want = m.align_batch(full, [u[2].shape[1] for u in us])
    for i in range(3):
        codes, al = got[i]
        assert torch.equal(codes, plain[i]) and codes.shape[1] == 16 * us[i][0].shape[1] + 1
        assert tuple(al.attn.shape) == (codes.shape[1], us[i][0].shape[1]) and _same_alignment(al, want[i])
        assert len(both[i]) == 3 and torch.equal(both[i][0], plain[i]) and both[i][1].n_tokens == codes.shape[1]
        assert _same_alignment(both[i][2], want[i])
    # the stream: its NAR groups differ from the static batch's, so it is held against its own run without the flag
    kw = dict(top_k=20, seeds=seeds, nar_group=2)
    plain_s = dict(m.inference_stream(us, **kw))
    got_s = dict(m.inference_stream(us, return_alignment=True, **kw))
    assert sorted(got_s) == [0, 1, 2]
    for i in range(3):
        codes, al = got_s[i]
        assert torch.equal(codes, plain_s[i])
        w = m.align_batch([(us[i][0], us[i][1], torch.cat([us[i][2], codes], 1))], us[i][2].shape[1])[0]
        assert _same_alignment(al, w)


def test_best_of_n_ranked_by_alignment():
    from valle_amd.models import alignment_rank_key, best_of_rank

    m, us = _gen_model()
    x, xl, y = us[1]
    n, seeds = 4, [101, 108, 115, 122]
    kw = dict(top_k=50, temperature=0.9, seeds=seeds)
    codes_lp, best_lp = m.inference_best_of(x, xl, y, None, n, **kw)
    again, best_lp2 = m.inference_best_of(x, xl, y, None, n, rank_by="logprob", **kw)
    assert torch.equal(codes_lp, again) and best_lp.index == best_lp2.index and best_lp.ar_mean == best_lp2.ar_mean
    assert best_lp.alignments is None and best_lp.rank_key == best_lp.ar_mean

    codes, best = m.inference_best_of(x, xl, y, None, n, rank_by="alignment", **kw)
    ref = m.inference_batch([(x, xl, y)] * n, **kw)
    assert best.seeds == seeds and best.ar_mean == best_lp.ar_mean and len(best.alignments) == n
    Q = y.shape[2]
    cand = []
    for tk in best.tokens:
        rows = torch.zeros((1, tk.numel(), Q), dtype=torch.int64, device="cuda")
        rows[0, :, 0] = tk.cuda()
        cand.append((x, xl, torch.cat([y, rows], 1)))
    want = m.align_batch(cand, y.shape[1])
    keys = []
    for k in range(n):
        assert torch.equal(best.tokens[k], ref[k][0, :, 0].cpu()) and _same_alignment(best.alignments[k], want[k])
        keys.append(want[k].path_score / want[k].attn.shape[0])
        assert best.rank_key[k] == keys[k] == alignment_rank_key(want[k])
    assert len(set(keys)) > 1  # the candidates differ: the choice means something
    assert best.index == max(range(n), key=lambda k: (keys[k], best.ar_mean[k], -k)) == best_of_rank(keys, best.ar_mean)
    assert torch.equal(codes, ref[best.index])
    # a callable: the candidate the log-probability likes least
    codes_c, best_c = m.inference_best_of(x, xl, y, None, n, rank_by=lambda al, g: -g.ar_mean, **kw)
    worst = min(range(n), key=lambda k: (best.ar_mean[k], k))
    assert best_c.index == worst and torch.equal(codes_c, ref[worst]) and best_c.rank_key == [-v for v in best.ar_mean]
    m._drop_engine()
