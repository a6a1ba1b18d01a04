"""GPU: the VALL-F row passes over concatenated utterances (VX_FLAG_VALLF_ROWS, ``VALLF(..., batched_rows=True)``): the segmented
cross-attention kernel (cross_attn_seg_kernel, through vx_op_cross_attention_segs) against plain fp64 torch in both of its
addressings, the batched NAR on a reference fixture, the batched prefill against the fp32 oracle, batched admission next to live
slots, the public interface, and one pass at the full geometry.

Kernel errors are measured in the unit of test_gpu_attention.py's segmented self-attention, u = 2^-9 (|ref| + vbar) with vbar =
sum_j p_j |v_j|: the kernel has the same arithmetic form (bf16 q / k / v, bf16 probabilities into the MFMA, fp32 accumulation, bf16
output) over key runs no longer than that test's, so its bound SEG_BOUND = 6.5 applies unchanged."""
import pytest
import torch

from conftest import Golden

BMAX = 64
pytestmark = pytest.mark.gpu

SEG_BOUND = 6.5     # tests/test_gpu_attention.py
WRONG_MARGIN = 4.0  # a wrong answer (one key more or fewer, the neighbour's memory) must be this many bounds away


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    engine.load_library()
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return engine


# ---- 1. the kernel against fp64 ---------------------------------------------------------------------------------------------------
SEG_LENS = [300, 1, 31, 64, 65, 127]      # query tiles of 128: three tiles, one row, a partial wave, one / one + 1 / two - 1 waves' tiles
SEG_GAPS = (1, 4)                         # an empty 64-row tile after these segments
KLENS = [1, 15, 16, 17, 63, 64, 65, 128]  # around the 16-key MFMA groups and the 64-key tile, and two full tiles
SLOT_PERM = [3, 0, 5, 1, 4, 2]

# name -> (H, segment lengths, gaps, key counts, max_text, slot map)
X_LAYOUTS = {}
for _H in (4, 16):
    for _off in (0, 4):  # the two windows of the cycled key counts cover all eight
        X_LAYOUTS[f"H{_H}_k{_off}"] = (_H, SEG_LENS, SEG_GAPS, [KLENS[(_off + z) % 8] for z in range(6)], 128, SLOT_PERM)
X_LAYOUTS["H4_k200"] = (4, [200], (), [200], 256, [1])  # four key tiles, the last one partial: the multi-tile loop


def _layout(lens, gaps):
    starts, r = [], 0
    for z, n in enumerate(lens):
        starts.append(r)
        r = -(-(r + n) // 64) * 64 + (64 if z in gaps else 0)
    return starts, r + 64


def _x_data(H, starts, lens, klens, max_text, rows, ldq, seed):
    """q (rows, ldq) bf16 and the logical memories K / V (n, H, max_text + 1, 64) (bf16 values, fp32).  Every query of segment z has a
    common component along a unit vector u[z, h]; keys klens[z] - 1 and klens[z] are multiples of it that score at least 9 above
    every other (query, key) pair of the segment and carry their own V rows: one key more or fewer moves every output row."""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    n = len(lens)
    q = torch.randn(rows, ldq, generator=g, device=dev)
    K = torch.randn(n, H, max_text + 1, 64, generator=g, device=dev).bfloat16().float()
    V = torch.randn(n, H, max_text + 1, 64, generator=g, device=dev).bfloat16().float()
    for z, (s, m, kl) in enumerate(zip(starts, lens, klens)):
        u = torch.randn(H, 64, generator=g, device=dev)
        u = u / u.norm(dim=-1, keepdim=True)
        qz = q[s : s + m, : 64 * H].reshape(m, H, 64).clone()
        qz += (8.0 - torch.einsum("mhc,hc->mh", qz, u))[..., None].clamp(min=0.0) * u  # q . u >= 8 for every query
        q[s : s + m, : 64 * H] = qz.reshape(m, 64 * H)
    q = q.bfloat16()
    for z, (s, m, kl) in enumerate(zip(starts, lens, klens)):
        qz = q[s : s + m, : 64 * H].float().reshape(m, H, 64).double()
        u = qz.mean(0)
        u = u / u.norm(dim=-1, keepdim=True)  # (H, 64): every query has a positive component along it
        along = torch.einsum("mhc,hc->mh", qz, u)
        assert float(along.min()) > 4.0
        top = (torch.einsum("mhc,hjc->mhj", qz, K[z, :, : kl - 1].double()) / 8).amax((0, 2)) if kl > 1 else torch.zeros(H, dtype=torch.float64, device=dev)
        beta = 8 * (top + 9) / along.amin(0)  # the weakest query still scores top + 9
        for j in (kl - 1, kl):
            K[z, :, j] = (beta[:, None] * u).float().bfloat16().float()
            V[z, :, j] = (3 * torch.randn(H, 64, generator=g, device=dev)).bfloat16().float()
    return q, K, V


def _x_mem(addressing, K, V, klens, max_text, slot_map, fill):
    """The physical memory in one addressing, every element that is not a visible key holding the int16 pattern `fill`:
    slots  [slot][K|V][head][max_text][64], segment z in slot slot_map[z] of 6 (the engine's slot memory, one layer);
    packed [K|V][head][total rows][64], segment z at text row trow[z] with one spare row behind it (the batched NAR's buffer)."""
    n, H = K.shape[0], K.shape[1]
    dev = K.device
    if addressing == "slots":
        nslot = max(slot_map) + 1 if len(slot_map) == 1 else 6
        mem = torch.empty((nslot, 2, H, max_text, 64), dtype=torch.bfloat16, device=dev)
        mem.view(torch.int16).fill_(fill)
        for z, kl in enumerate(klens):
            mem[slot_map[z], 0, :, :kl] = K[z, :, :kl].bfloat16()
            mem[slot_map[z], 1, :, :kl] = V[z, :, :kl].bfloat16()
        return mem, [sl * 2 * H * max_text * 64 for sl in slot_map], max_text * 64, H * max_text * 64
    trow, total = [], 0
    for kl in klens:
        trow.append(total)
        total += kl + 1
    total = -(-total // 8) * 8
    mem = torch.empty((2, H, total, 64), dtype=torch.bfloat16, device=dev)
    mem.view(torch.int16).fill_(fill)
    for z, kl in enumerate(klens):
        mem[0, :, trow[z] : trow[z] + kl] = K[z, :, :kl].bfloat16()
        mem[1, :, trow[z] : trow[z] + kl] = V[z, :, :kl].bfloat16()
    return mem, [t * 64 for t in trow], total * 64, H * total * 64


def _x_ref(q, H, s, m, Kz, Vz, nk):
    """fp64 attention of the m query rows at row s over the first nk keys of (Kz, Vz) (H, >= nk, 64) -> (out, vbar) (m, H, 64)"""
    qh = q[s : s + m, : 64 * H].double().reshape(m, H, 64).transpose(0, 1)
    p = torch.softmax(qh @ Kz[:, :nk].double().transpose(1, 2) / 8, dim=-1)
    v = Vz[:, :nk].double()
    return (p @ v).transpose(0, 1), (p @ v.abs()).transpose(0, 1)


@pytest.mark.parametrize("addressing", ["packed", "slots"])
@pytest.mark.parametrize("layout", sorted(X_LAYOUTS))
def test_cross_attention_segs_matches_fp64(eng, layout, addressing):
    """Every segment against fp64 over exactly its own klen keys.  Memory rows at and past klen and all unused memory are NaN, then
    0x7F7F: the output does not change by a bit.  One key more or fewer and the neighbouring segment's memory are far outside the
    bound.  Gap rows of `out` keep their sentinel; two runs are bitwise equal."""
    H, lens, gaps, klens, max_text, slot_map = X_LAYOUTS[layout]
    starts, rows = _layout(lens, gaps)
    d = 64 * H
    ldq = d + 64 if H == 4 else d  # a q buffer wider than the heads (the engine's is exactly d)
    q, K, V = _x_data(H, starts, lens, klens, max_text, rows, ldq, seed=17 * H + len(lens) + klens[0])
    inseg = torch.zeros(rows, dtype=torch.bool, device="cuda")
    for s, m in zip(starts, lens):
        inseg[s : s + m] = True
    q[~inseg] = float("nan")  # query rows outside the segments are not read into anything that is stored
    sentinel = torch.full((rows, d), 0x3C5A, dtype=torch.int16, device="cuda")

    def run(fill):
        mem, off, hs, vo = _x_mem(addressing, K, V, klens, max_text, slot_map, fill)
        return eng.op_cross_attention_segs(q, mem, off, hs, vo, klens, H, starts, lens, out=sentinel.clone().view(torch.bfloat16))

    out = run(-1)  # 0xFFFF: NaN
    assert torch.equal(out.view(torch.int16)[~inseg], sentinel[~inseg]), "a row outside the segments was written"
    assert torch.isfinite(out.float()[inseg]).all(), "a memory row at or past klen, or another segment's memory, reached the output"
    assert torch.equal(run(-1).view(torch.int16), out.view(torch.int16)), "not deterministic"
    assert torch.equal(run(0x7F7F).view(torch.int16), out.view(torch.int16)), "unused memory changed the output"

    o = out.double().reshape(rows, H, 64)
    worst, nearest_wrong = 0.0, float("inf")
    n = len(lens)
    for z, (s, m, kl) in enumerate(zip(starts, lens, klens)):
        ref, vbar = _x_ref(q, H, s, m, K[z], V[z], kl)
        unit = 2.0 ** -9 * (ref.abs() + vbar)
        err = ((o[s : s + m] - ref).abs() / unit).max().item()
        print(f"cross_attention_segs {layout} {addressing}: segment {z} (len {m}, klen {kl}) error {err:.3f} units")
        worst = max(worst, err)
        assert err <= SEG_BOUND, f"segment {z} (start {s}, len {m}, klen {kl}): error {err:.3f} units"
        wrongs = [_x_ref(q, H, s, m, K[z], V[z], alt)[0] for alt in (kl - 1, kl + 1) if alt >= 1]
        if n > 1:
            nb = (z + 1) % n
            wrongs.append(_x_ref(q, H, s, m, K[nb], V[nb], klens[nb])[0])
        for w in wrongs:  # every (query, head) of the segment is far from every wrong answer
            dist = ((o[s : s + m] - w).abs() / unit).amax(-1).min().item()
            nearest_wrong = min(nearest_wrong, dist)
            assert dist > WRONG_MARGIN * SEG_BOUND, f"segment {z}: a wrong answer is only {dist:.2f} units away"
    print(f"cross_attention_segs {layout} {addressing}: worst {worst:.3f} units (bound {SEG_BOUND}), nearest wrong answer {nearest_wrong:.1f} units")


# ---- engines -------------------------------------------------------------------------------------------------------------------------
def _setup_rows(max_batch=4, d=256, nhead=4, L=4, max_text=64, max_audio=700, **kw):
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.config import ModelConfig
    from valle_amd.models import VALLF
    from valle_amd.weights import synthetic_state_dict

    cfg = ModelConfig(model_name="VALL-F", decoder_dim=d, nhead=nhead, num_decoder_layers=L, prefix_mode=1)
    sd = synthetic_state_dict(cfg, 0)
    m = VALLF(d, nhead, L, prefix_mode=1, precision="bf16", max_text=max_text, max_audio=max_audio, print_eos=False, max_batch=max_batch,
              batched_rows=True, **kw)
    m.load_state_dict(sd)
    return cfg, sd, m.to("cuda:0").eval()


def _utts(shapes, seed0=10):
    from valle_amd.weights import synthetic_inputs

    return [synthetic_inputs(S, P, 8, seed=seed0 + i) for i, (S, P) in enumerate(shapes)]


class _few_threads:
    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(4)

    def __exit__(self, *a):
        torch.set_num_threads(self.n)


# ---- 2. batched NAR on a reference fixture -------------------------------------------------------------------------------------------
def test_vallf_batched_nar_on_a_reference_fixture():
    """vallf_cfg0_topk10 as segments 0 and 2 of a four-segment batched NAR pass (1 and 3: synthetic utterances of other sizes on the
    same weights), every stage fed the given earlier codes: the two copies bitwise equal, per-stage agreement with the fixture's
    codes >= 0.90 (the per-utterance test's floor), the others' codes in range.  Prints the per-utterance path's agreement too.
    Measured on the MI355X: see DESIGN.md 4.3."""
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.models import get_model

    g = Golden("vallf_cfg0_topk10")
    c = g.cfg
    m = get_model(dict(model_name="VALL-F", decoder_dim=c.decoder_dim, nhead=c.nhead, num_decoder_layers=c.num_decoder_layers,
                       scale_factor=c.scale_factor, norm_first=c.norm_first, add_prenet=c.add_prenet, prefix_mode=c.prefix_mode,
                       share_embedding=c.share_embedding, prepend_bos=c.prepend_bos, num_quantizers=c.num_quantizers,
                       precision="bf16", max_text=128, max_audio=1280, max_batch=4, batched_rows=True))
    m.print_eos = False
    m.load_state_dict(g.state_dict())
    eng = m.to("cuda:0").eval().engine()
    Q = c.num_quantizers
    text, prompts = g.x[0], g.y[0, :, :Q].contiguous()
    fcodes = g.codes[0].contiguous()
    gen = torch.Generator().manual_seed(5)
    texts, proms, toks, forced = [], [], [], []
    for spec in [None, (3, 8, 40), None, (11, 30, 150)]:
        S, P, T = spec or (None, None, None)
        if spec is None:
            texts.append(text); proms.append(prompts); toks.append(fcodes[:, 0].contiguous()); forced.append(fcodes)
        else:
            fc = torch.randint(0, 1024, (T, Q), generator=gen)
            texts.append(torch.randint(1, 500, (S,), generator=gen)); proms.append(torch.randint(0, 1024, (P, Q), generator=gen))
            toks.append(fc[:, 0].contiguous()); forced.append(fc)
    res = [r.cpu() for r in eng.nar_batch(texts, proms, toks, forced_codes=forced)]
    assert torch.equal(res[0], res[2]), "two copies of one utterance in one batched pass differ"
    for z in (1, 3):
        assert res[z].shape == (toks[z].numel(), Q) and int(res[z].min()) >= 0 and int(res[z].max()) < 1024
        assert torch.equal(res[z][:, 0], toks[z])
    batched = (res[0][:, 1:] == g.codes[0, :, 1:]).float().mean(0)
    single = (eng.nar(text, prompts, fcodes[:, 0].contiguous(), forced_codes=fcodes).cpu()[:, 1:] == g.codes[0, :, 1:]).float().mean(0)
    print("vallf_cfg0_topk10 NAR agreement per stage: batched", [round(float(v), 4) for v in batched],
          "per utterance", [round(float(v), 4) for v in single])
    assert float(batched.min()) >= 0.90, batched


# ---- 3. batched prefill against the fp32 oracle -----------------------------------------------------------------------------------------
def test_vallf_batched_prefill_teacher_forced_against_fp32_oracle():
    """test_vallf_slots_teacher_forced_against_fp32_oracle with one batch_prefill_all in place of the three per-slot prefills:
    per-pass argmax agreement >= 0.97, the logits after 25 forced tokens and the prefill's own logits (trace row 0) within 3 % of
    the row's scale."""
    from oracle import valle_oracle as vo

    cfg, sd, m = _setup_rows(max_batch=4, trace_logits=True)
    eng = m.engine()
    utts = _utts([(5, 30), (9, 12), (3, 55)])
    om = vo.OracleModelF(sd, cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers, prefix_mode=cfg.prefix_mode, num_quantizers=1)
    refs = []
    for x, xl, y in utts:
        tr = {}
        with _few_threads():
            codes = vo.inference_f(om, x, xl, y, None, 1, 1.0, None, trace=tr)  # greedy reference tokens
        refs.append((codes[0, :, 0].contiguous(), torch.stack(tr["ar_logits"])))
    eng.batch_prefill_all([x[0] for x, _, _ in utts], [y[0, :, 0].contiguous() for _, _, y in utts])
    eng.batch_decode(3, top_k=1, forced=[r[0].cuda() for r in refs])
    stride = eng.max_audio + 2
    arg = eng.read("batch_argmax", (BMAX, stride), dtype=torch.int32)
    K = 25
    for b, (toks, ref_logits) in enumerate(refs):
        got, reason = eng.batch_result(b)
        assert torch.equal(got, toks) and reason == 4
        n = toks.numel()
        assert n > K
        agree = (arg[b, :n].long() == ref_logits[:n].argmax(1)).float().mean().item()
        errs = []
        for k in (0, K):
            row = eng.read("batch_trace", (1025,), offset_bytes=(b * stride + k) * 1025 * 4)
            errs.append(float((row - ref_logits[k]).abs().max()) / float(ref_logits[k].abs().max()))
        print(f"batched prefill slot {b}: argmax agreement {agree:.4f}, relative logits error row 0 {errs[0]:.4f}, row {K} {errs[1]:.4f}")
        assert agree >= 0.97, (b, agree)
        assert errs[1] <= 0.03, (b, errs)
        assert errs[0] <= 0.03, (b, errs)


# ---- 4. batched admission leaves live slots alone --------------------------------------------------------------------------------------
def test_vallf_batched_admission_leaves_live_slots_alone():
    """Slot 2 is admitted per slot next to a pacer (slot 0, six tokens).  When the pacer has stopped, slots 3 and 1 are admitted in
    one batched pass; slot 2, live throughout, must produce bitwise the tokens of the same session without that admission."""
    cfg, sd, m = _setup_rows(max_batch=4)
    eng = m.engine()
    pacer, main, a, b = _utts([(4, 10), (6, 30), (3, 8), (2, 21)], seed0=60)
    cb0 = lambda u: u[2][0, :, 0].contiguous()

    def session(second):
        eng.batch_open()
        eng.batch_admit([0], [pacer[0][0]], [cb0(pacer)], top_k=5, seeds=[7], max_new_tokens=6, batched=False)
        eng.batch_admit([2], [main[0][0]], [cb0(main)], top_k=5, seeds=[8], batched=False)
        assert eng.batch_run(1, poll_steps=2) == [0]
        out = {0: eng.batch_result(0)}
        if second:
            eng.batch_admit([3, 1], [a[0][0], b[0][0]], [cb0(a), cb0(b)], top_k=5, seeds=[9, 10], batched=True)
        left = {1, 2, 3} if second else {2}
        while left:
            for sl in eng.batch_run(1, poll_steps=4):
                out[sl] = eng.batch_result(sl)
                left.discard(sl)
        return out

    with_adm, without, again = session(True), session(False), session(True)
    assert with_adm[0][0].numel() == 6
    assert torch.equal(with_adm[2][0], without[2][0]) and with_adm[2][1] == without[2][1], "a batched admission changed a live slot"
    assert with_adm[2][0].numel() == 16 * 6 + 1
    assert with_adm[3][0].numel() == 16 * 3 + 1 and with_adm[1][0].numel() == 16 * 2 + 1  # each by its own length rule
    for sl in (0, 1, 2, 3):
        assert torch.equal(with_adm[sl][0], again[sl][0]) and with_adm[sl][1] == again[sl][1], sl
        assert int(with_adm[sl][0].min()) >= 0 and int(with_adm[sl][0].max()) < 1024


# ---- 5. the public interface ---------------------------------------------------------------------------------------------------------
INDEP_SHAPES = [(6, 30), (9, 12), (4, 55), (3, 8)]


def test_vallf_batched_rows_public_interface():
    cfg, sd, m = _setup_rows(max_batch=4)
    u = _utts(INDEP_SHAPES)
    seeds = [11, 22, 33, 44]
    a = m.inference_batch(u, top_k=5, seeds=seeds)  # defaults: batched prefill and batched NAR
    b = m.inference_batch(u, top_k=5, seeds=seeds)
    for codes, again, (x, _, _) in zip(a, b, u):
        assert codes.shape == (1, 16 * x.shape[1] + 1, 8)
        assert int(codes.min()) >= 0 and int(codes.max()) < 1024
        assert torch.equal(codes, again)
    # a queue no longer than the slot count: the stream admits the same group in one batched pass
    got = dict(m.inference_stream(u, top_k=5, seeds=seeds, batched_admit=True, batched_nar=True))
    assert sorted(got) == [0, 1, 2, 3]
    for i in range(4):
        assert torch.equal(got[i][0, :, 0], a[i][0, :, 0]), i
    # per-slot / per-utterance on the same model: same lengths, codes in range
    c = m.inference_batch(u, top_k=5, seeds=seeds, batched_prefill=False, batched_nar=False)
    for codes, ref in zip(c, a):
        assert codes.shape == ref.shape and int(codes.min()) >= 0 and int(codes.max()) < 1024


def test_vallf_batched_rows_do_not_depend_on_uninitialised_memory():
    """VX_POISON=1 fills every fresh device allocation (the packed text memory and the regrown row buffers included) with NaN
    bytes: the codes of the batched paths must not change."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = (
        "import sys, json, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from test_gpu_vallf_rows import _setup_rows, _utts, INDEP_SHAPES\n"
        "cfg, sd, m = _setup_rows(max_batch=4)\n"
        "a = m.inference_batch(_utts(INDEP_SHAPES), top_k=5, seeds=[11, 22, 33, 44])\n"
        "print(json.dumps([t.flatten().tolist() for t in a]))\n" % (root, os.path.join(root, "tests")))
    outs = []
    for poison in ("0", "1"):
        env = dict(os.environ, VX_POISON=poison)
        r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]
    assert all(0 <= v < 1024 for seq in outs[1] for v in seq)


# ---- 6. the full geometry, once ----------------------------------------------------------------------------------------------------
def test_vallf_batched_nar_full_geometry_32_segments():
    """d = 1024, 16 heads, 12 layers, 32 segments alternating two utterances (the text / prompt mix of
    test_vallf_full_geometry_32_slots), 64 forced tokens each: 4096 concatenated rows, i.e. the 256^2 GEMM dispatch and a
    (1, 16, 32) grid of the cross-attention kernel.  Codes in range, all copies of an utterance bitwise equal - not a parity claim."""
    B, T = 32, 64
    cfg, sd, m = _setup_rows(max_batch=B, d=1024, nhead=16, L=12, max_text=128, max_audio=320)
    eng = m.engine()
    two = _utts([(47, 60), (23, 41)], seed0=70)
    fc = [torch.randint(0, 1024, (T, 8), generator=torch.Generator().manual_seed(90 + i)) for i in range(2)]
    kind = [b % 2 for b in range(B)]
    res = eng.nar_batch([two[k][0][0] for k in kind], [two[k][2][0].contiguous() for k in kind], [fc[k][:, 0].contiguous() for k in kind],
                        forced_codes=[fc[k] for k in kind])
    for b in range(B):
        r = res[b].cpu()
        assert r.shape == (T, 8) and int(r.min()) >= 0 and int(r.max()) < 1024
        assert torch.equal(r, res[kind[b]].cpu()), b
