"""GPU: the nucleus (top-p) filter of the AR sampler (sample4_body, the one sampling body of every decode step form).

* op level: vx_op_sample_topp on the reference's own masks (tests/golden/topp) with fixed Exp(1) noise;
* in situ: teacher-forced decodes with traced logits and given noise; every pass's sample is recomputed from the engine's own
  logits with tests/topp_ref.py - the sharded step and the five-launch step (VX_AR_TP=0) at d = 1024 / 16 heads, a VALL-F
  batch-1 engine, the batched step at B = 17 and 32 with slots mixing top-p off / top-k 10 + top-p 0.9 / top-p 0.8 alone, and
  a stream session that admits a top-p request into a refilled slot;
* end to end: fp32 engine with sampling="torch_cpu" against the oracle with the top-p sampler;
* off means off: top_p = 1.0 and a zero-filled struct give the same codes as a call without the keyword.
A pass is decided when the kept set lies more than 1e-6 (probability mass) from changing and its two best p / q differ by
more than 1e-5 relative; every decided pass must match exactly."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import topp_ref
from conftest import GOLDEN, Golden

pytestmark = pytest.mark.gpu

BMAX = 64
V = 1025
MARGIN = 1e-6
MIXED = [(10, 1.0), (10, 0.9), (-100, 0.8)]  # (top_k, top_p) of slot b: MIXED[b % 3]


def _build():
    import __graft_entry__ as ge

    ge.build()


def _noise(rows, seed):
    return torch.empty(rows, V).exponential_(1, generator=torch.Generator().manual_seed(seed))


def _pq_decided(logits, top_k, temp, top_p, q):
    x = logits.float().clone()
    if temp != 1.0:
        x = x / temp
    x = topp_ref.top_p_filter_(topp_ref.top_k_filter_(x, top_k), top_p)
    r = torch.softmax(x, -1) / q
    t2 = r.topk(2)[0]
    return float(t2[0] - t2[1]) > 1e-5 * float(t2[0])


def _check_passes(logits, sampled, noise, top_k, temp, top_p, what, min_decided=0.8):
    """Every decided pass: the engine's sample == the restated sampler on the engine's own logits.  Returns (decided, n)."""
    n = logits.shape[0]
    dec = 0
    for i in range(n):
        q = noise[min(i, noise.shape[0] - 1)]
        if topp_ref.boundary_margin(logits[i], top_k, temp, top_p) <= MARGIN or not _pq_decided(logits[i], top_k, temp, top_p, q):
            continue
        dec += 1
        want = topp_ref.expected_sample(logits[i], top_k, temp, top_p, q)
        assert int(sampled[i]) == want, (what, i, int(sampled[i]), want)
    print(what, f"decided {dec}/{n}")
    assert dec >= min_decided * n, (what, dec, n)
    return dec, n


# ---- op level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["t100", "t070"])
def test_op_sample_topp_matches_reference_masks(tag):
    _build()
    from valle_amd.engine import op_sample_topp

    rows = np.load(os.path.join(GOLDEN, "topp", "rows.npz"))
    z = np.load(os.path.join(GOLDEN, "topp", f"cases_{tag}.npz"))
    logits = torch.from_numpy(rows["logits"])
    masks = torch.from_numpy(np.unpackbits(z["masks"], axis=-1)[..., :V].astype(bool))
    temp = float(z["temperature"])
    R = logits.shape[0]
    noise = _noise(R, 77)
    dl, dq = logits.cuda(), noise.cuda()
    decided = total = 0
    for r in range(R):
        x = logits[r] / temp if temp != 1.0 else logits[r]
        raw_argmax = int(torch.argmax(logits[r]))
        for c, (tp, tk) in enumerate(zip(z["top_p"], z["top_k"])):
            got, am = op_sample_topp(dl[r], int(tk), temp, float(tp), dq[r])
            assert am == raw_argmax, (r, c)
            total += 1
            if float(z["margin"][r, c]) <= MARGIN:
                continue
            p = torch.softmax(torch.where(masks[r, c], x, torch.tensor(-float("inf"))), -1) / noise[r]
            t2 = p.topk(2)[0]
            if float(t2[0] - t2[1]) <= 1e-5 * float(t2[0]):
                continue
            decided += 1
            assert got == int(torch.argmax(p)), (tag, r, float(tp), int(tk), got, int(torch.argmax(p)))
    frac = decided / total
    print(f"{tag}: decided {decided}/{total} = {frac:.4f}")
    assert frac >= 0.95


def test_op_sample_topp_off_and_limits():
    _build()
    from valle_amd.engine import VxError, op_sample, op_sample_topp

    g = torch.Generator().manual_seed(5)
    for top_k, temp in [(10, 1.0), (-100, 0.7), (64, 1.3)]:
        x = (torch.randn(V, generator=g) * 2).cuda()
        q = _noise(1, 9)[0].cuda()
        assert op_sample_topp(x, top_k, temp, 1.0, q) == op_sample(x, top_k, temp, q)
        assert op_sample_topp(x, top_k, temp, 3.0, q) == op_sample(x, top_k, temp, q)  # >= 1: off
    big = torch.randn(1500).cuda()
    with pytest.raises(VxError) as ei:
        op_sample_topp(big, -100, 1.0, 0.9, None)
    assert ei.value.code == 5  # VX_ERR_UNSUPPORTED: the single-wave kernel has no nucleus stage
    assert op_sample_topp(big, -100, 1.0, 1.0, None)[1] == int(torch.argmax(big.cpu()))
    with pytest.raises(VxError) as ei:
        op_sample_topp(x, 10, 1.0, float("nan"), None)
    assert ei.value.code == 1


# ---- in situ: batch-1 step forms --------------------------------------------------------------------------------------------
def _batch1_passes(m, x, y, forced, cases):
    e = m.engine()
    for top_k, temp, top_p, seed in cases:
        noise = _noise(forced.numel() + 1, seed)
        e.ar_prefill(x[0], y[0, :, 0].contiguous())
        e.ar_decode(top_k=top_k, temperature=temp, top_p=top_p, exp_noise=noise, forced=forced)
        toks, reason, n_pass = e.ar_result()
        assert torch.equal(toks, forced) and n_pass == forced.numel() + 1
        lg = e.read("ar_logits", (n_pass, V)).clone()
        smp = e.read("ar_sampled", (n_pass,), dtype=torch.int32).clone()
        _check_passes(lg, smp, noise, top_k, temp, top_p, f"{type(m).__name__} k{top_k} t{temp} p{top_p}")


BATCH1_CASES = [(10, 1.0, 0.9, 1), (-100, 1.0, 0.8, 2), (-100, 0.7, 0.95, 3), (64, 1.0, 0.5, 4)]


@pytest.mark.parametrize("tp", ["1", "0"])
def test_sharded_and_plain_step_sample_with_top_p(tp, monkeypatch):
    """d = 1024 / 16 heads (BASELINE configs[1]'s geometry, two layers): VX_AR_TP=1 runs the sharded step, 0 the five-launch one."""
    _build()
    from valle_amd.config import ModelConfig
    from valle_amd.models import VALLE
    from valle_amd.weights import synthetic_inputs, synthetic_state_dict

    monkeypatch.setenv("VX_AR_TP", tp)
    cfg = ModelConfig(decoder_dim=1024, nhead=16, num_decoder_layers=2, prefix_mode=1)
    m = VALLE(1024, 16, 2, prefix_mode=1, precision="bf16", max_text=64, max_audio=512, print_eos=False, trace_logits=True)
    m.load_state_dict(synthetic_state_dict(cfg, 3))
    m.to("cuda:0").eval()
    x, xl, y = synthetic_inputs(40, 100, 8, seed=9)
    forced = torch.randint(0, 1024, (120,), generator=torch.Generator().manual_seed(4))
    _batch1_passes(m, x, y, forced, BATCH1_CASES)


def test_vallf_batch1_samples_with_top_p():
    _build()
    from valle_amd.config import ModelConfig
    from valle_amd.models import VALLF
    from valle_amd.weights import synthetic_inputs, synthetic_state_dict

    cfg = ModelConfig(model_name="VALL-F", decoder_dim=256, nhead=4, num_decoder_layers=4, prefix_mode=1)
    m = VALLF(256, 4, 4, prefix_mode=1, precision="bf16", max_text=64, max_audio=512, print_eos=False, trace_logits=True)
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    m.to("cuda:0").eval()
    x, xl, y = synthetic_inputs(12, 30, 8, seed=5)
    forced = torch.randint(0, 1024, (80,), generator=torch.Generator().manual_seed(6))
    _batch1_passes(m, x, y, forced, BATCH1_CASES)


# ---- in situ: batched step and session --------------------------------------------------------------------------------------
def _batch_model(B, vallf=False):
    _build()
    from valle_amd.config import ModelConfig
    from valle_amd.models import VALLE, VALLF

    cls, name = (VALLF, "VALL-F") if vallf else (VALLE, "VALL-E")
    from valle_amd.weights import synthetic_state_dict

    cfg = ModelConfig(model_name=name, decoder_dim=256, nhead=4, num_decoder_layers=4, prefix_mode=1)
    m = cls(256, 4, 4, prefix_mode=1, precision="bf16", max_text=64, max_audio=400, print_eos=False, max_batch=B, trace_logits=True)
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    return m.to("cuda:0").eval()


def _slot_check(eng, b, n_pass, noise, top_k, top_p, what):
    stride = eng.max_audio + 2
    lg = eng.read("batch_trace", (n_pass, V), offset_bytes=b * stride * V * 4).clone()
    smp = eng.read("batch_sampled", (BMAX, stride), dtype=torch.int32)[b, :n_pass].clone()
    return _check_passes(lg, smp, noise, top_k, 1.0, top_p, what)


@pytest.mark.parametrize("B,max_batch", [(17, 32), (32, 32)])
def test_batched_step_mixes_top_p_slots(B, max_batch):
    from valle_amd.weights import synthetic_inputs

    m = _batch_model(max_batch)
    eng = m.engine()
    utts = [synthetic_inputs(3 + b % 4, 6 + (b * 5) % 17, 8, seed=20 + b) for b in range(B)]
    eng.batch_prefill_all([u[0][0] for u in utts], [u[2][0, :, 0].contiguous() for u in utts])
    g = torch.Generator().manual_seed(11)
    forced = [torch.randint(0, 1024, (20 + (b * 7) % 31,), generator=g) for b in range(B)]
    noise = [_noise(f.numel() + 1, 100 + b) for b, f in enumerate(forced)]
    ks = [MIXED[b % 3][0] for b in range(B)]
    ps = [MIXED[b % 3][1] for b in range(B)]
    eng.batch_decode(B, top_k=ks, top_p=ps, exp_noise=[q.cuda() for q in noise], forced=[f.cuda() for f in forced])
    for b in range(B):
        toks, reason = eng.batch_result(b)
        assert torch.equal(toks, forced[b]) and reason == 4
        _slot_check(eng, b, forced[b].numel() + 1, noise[b], ks[b], ps[b], f"B{B} slot {b} k{ks[b]} p{ps[b]}")


def test_stream_session_admits_top_p_request_into_refilled_slot():
    from valle_amd.weights import synthetic_inputs

    m = _batch_model(4)
    eng = m.engine()
    utts = [synthetic_inputs(4 + i, 8 + 3 * i, 8, seed=40 + i) for i in range(3)]
    t = lambda i: [utts[i][0][0]]
    p = lambda i: [utts[i][2][0, :, 0].contiguous()]
    g = torch.Generator().manual_seed(12)
    long_f, pacer_f, late_f = (torch.randint(0, 1024, (n,), generator=g) for n in (60, 6, 30))
    long_q, late_q = _noise(61, 1), _noise(31, 2)
    eng.batch_open()
    # top-p requests go through the batched admission: its prefill also writes the pass-0 trace row
    eng.batch_admit([1], t(0), p(0), top_k=10, top_p=0.9, exp_noise=[long_q.cuda()], forced=[long_f.cuda()], batched=True)
    eng.batch_admit([0], t(1), p(1), top_k=1, forced=[pacer_f.cuda()], batched=False)
    assert eng.batch_run(1, 4) == [0]  # the pacer stops first
    toks, _ = eng.batch_result(0)
    assert torch.equal(toks, pacer_f)
    # slot 0 refilled mid-decode with a top-p-only request
    eng.batch_admit([0], t(2), p(2), top_k=-100, top_p=0.8, exp_noise=[late_q.cuda()], forced=[late_f.cuda()], batched=True)
    done = []
    while len(done) < 2:
        done += eng.batch_run(1, 4)
    assert sorted(done) == [0, 1]
    _slot_check(eng, 0, late_f.numel() + 1, late_q, -100, 0.8, "session slot 0 (refilled)")
    _slot_check(eng, 1, long_f.numel() + 1, long_q, 10, 0.9, "session slot 1")
    assert torch.equal(eng.batch_result(0)[0], late_f) and torch.equal(eng.batch_result(1)[0], long_f)


def test_engine_refuses_bad_top_p_before_decoding():
    from valle_amd.engine import VxError
    from valle_amd.weights import synthetic_inputs

    m = _batch_model(4)
    eng = m.engine()
    u = synthetic_inputs(4, 8, 8, seed=1)
    eng.batch_prefill(0, u[0][0], u[2][0, :, 0].contiguous())
    for bad in (float("nan"), -0.25):
        with pytest.raises(VxError) as ei:
            eng.batch_decode(1, top_p=bad)
        assert ei.value.code == 1
    eng.batch_open()
    with pytest.raises(VxError) as ei:
        eng.batch_admit([0], [u[0][0]], [u[2][0, :, 0].contiguous()], top_p=float("nan"))
    assert ei.value.code == 1


# ---- end to end, fp32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg0_topk10", "tiny_mode0"])
def test_fp32_torch_cpu_sampling_with_top_p_matches_oracle(name, monkeypatch):
    from oracle import valle_oracle as vo
    from valle_amd.models import VALLE

    _build()
    top_p, top_k, seed = 0.8, -100, 1234
    g = Golden(name)
    c = g.cfg
    m = VALLE(c.decoder_dim, c.nhead, c.num_decoder_layers, norm_first=c.norm_first, add_prenet=c.add_prenet, prefix_mode=c.prefix_mode,
              share_embedding=c.share_embedding, nar_scale_factor=c.scale_factor, prepend_bos=c.prepend_bos,
              num_quantizers=c.num_quantizers, precision="fp32", max_text=128, max_audio=1280, print_eos=False, sampling="torch_cpu")
    m.load_state_dict(g.state_dict())
    m.to("cuda:0").eval()
    torch.manual_seed(seed)
    codes = m.inference(g.x.cuda(), g.x_lens.cuda(), g.y.cuda(), g.enroll_x_lens, top_k=top_k, top_p=top_p).cpu()
    nxt = torch.empty(1, V).exponential_(1)

    # the reference with the nucleus filter on, fed the same Exp(1) stream (one row per pass from the global generator)
    S, bos = g.x.shape[1], int(c.prepend_bos)
    torch.manual_seed(seed)
    noise = torch.stack([torch.empty(1, V).exponential_(1)[0] for _ in range(max(1, 16 * S + 2 - bos))])
    monkeypatch.setattr(vo, "topk_sampling", lambda lg, k, t, q=None: topp_ref.topk_sampling(lg, k, t, q, top_p))
    tr = {}
    want = vo.inference_cached(g.oracle(), g.x, g.x_lens, g.y, g.enroll_x_lens, top_k, 1.0, noise, trace=tr)
    n_pass = len(tr["ar_logits"])
    undecided = [i for i, lg in enumerate(tr["ar_logits"])
                 if topp_ref.boundary_margin(lg, top_k, 1.0, top_p) <= MARGIN or not _pq_decided(lg, top_k, 1.0, top_p, noise[i])]
    print(name, "passes", n_pass, "undecided", undecided)
    if not undecided:
        assert torch.equal(codes, want)
    else:  # the AR tokens agree up to the first pass the margin rule leaves open
        k = undecided[0]
        assert torch.equal(codes[0, :k, 0], want[0, :k, 0])
    # the global generator is left where the reference leaves it: one draw per executed pass, the pass that trips the stop rule
    # included (T + 1; the oracle skips computing that pass when the length rule is certain to fire, so its trace can be shorter)
    torch.manual_seed(seed)
    for _ in range(want.shape[1] + 1):
        torch.empty(1, V).exponential_(1)
    assert torch.equal(nxt, torch.empty(1, V).exponential_(1))


# ---- off means off ----------------------------------------------------------------------------------------------------------
def test_top_p_off_is_bitwise_the_default_path():
    _build()
    from valle_amd.config import ModelConfig
    from valle_amd.engine import VxDecodeParams, _check
    from valle_amd.weights import synthetic_inputs

    g = Golden("cfg0_topk10")
    c = g.cfg
    from valle_amd.models import VALLE

    m = VALLE(c.decoder_dim, c.nhead, c.num_decoder_layers, prefix_mode=c.prefix_mode, share_embedding=c.share_embedding,
              nar_scale_factor=c.scale_factor, prepend_bos=c.prepend_bos, num_quantizers=c.num_quantizers, precision="bf16",
              max_text=128, max_audio=1280, print_eos=False)
    m.load_state_dict(g.state_dict())
    m.to("cuda:0").eval()
    args = (g.x.cuda(), g.x_lens.cuda(), g.y.cuda(), g.enroll_x_lens)
    torch.manual_seed(5)
    a = m.inference(*args, top_k=10).cpu()
    torch.manual_seed(5)
    b = m.inference(*args, top_k=10, top_p=1.0).cpu()
    assert torch.equal(a, b)
    # a zero-filled struct through the C ABI directly (top_p = 0)
    e = m.engine()
    res = []
    for raw in (False, True):
        e.ar_prefill(g.x[0], g.y[0, :, 0].contiguous())
        if raw:
            p = VxDecodeParams()
            C.memset(C.byref(p), 0, C.sizeof(p))
            p.struct_size, p.top_k, p.temperature, p.max_new_tokens, p.seed = C.sizeof(p), 10, 1.0, -1, 99
            _check(e.lib.vx_ar_decode(e.h, C.byref(p), None))
        else:
            e.ar_decode(top_k=10, seed=99)
        res.append(e.ar_result()[0])
    assert torch.equal(res[0], res[1])

    # batched: no keyword, top_p = 1.0 per slot, a zero-filled struct array
    mb = _batch_model(8)
    eb = mb.engine()
    utts = [synthetic_inputs(3 + i % 3, 7 + 2 * i, 8, seed=60 + i) for i in range(5)]
    outs = []
    for mode in ("none", "one", "raw"):
        eb.batch_prefill_all([u[0][0] for u in utts], [u[2][0, :, 0].contiguous() for u in utts])
        seeds = [7 + i for i in range(5)]
        if mode == "none":
            eb.batch_decode(5, top_k=10, seeds=seeds, max_new_tokens=40)
        elif mode == "one":
            eb.batch_decode(5, top_k=10, seeds=seeds, max_new_tokens=40, top_p=[1.0] * 5)
        else:
            arr = (VxDecodeParams * 5)()
            C.memset(arr, 0, C.sizeof(arr))
            for i in range(5):
                arr[i].struct_size, arr[i].top_k, arr[i].temperature, arr[i].max_new_tokens, arr[i].seed = C.sizeof(VxDecodeParams), 10, 1.0, 40, seeds[i]
            _check(eb.lib.vx_batch_decode(eb.h, 5, arr, None))
        outs.append([eb.batch_result(i)[0] for i in range(5)])
    for o in outs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(outs[0], o))
