"""GPU: the whole hot path through the C ABI against (a) the committed reference vectors and
(b) the CPU oracle on the same seeded inputs.

fp32 engine  -> free-running codes must equal the reference's bit for bit; logits within 2e-4.
bf16 engine  -> teacher-forced (the reference's own tokens are fed back) so that rounding cannot
                compound through sampling; logits within the bf16 tolerance stated below, and
                argmax / sampled index equal wherever the reference's decision margin exceeds it.
"""
import os

import pytest
import torch

from conftest import Golden, golden_names

pytestmark = pytest.mark.gpu

SMALL = [n for n in golden_names() if not n.startswith(("cfg1", "cfg4"))]  # the full-size fixtures have tests of their own


_BIG = {}  # d >= 1024 engines, shared across the tests of this module: the full-size fixtures use ONE model (weight seed 0)


def _model(g, precision, **kw):
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.models import VALLE

    c = g.cfg
    big = c.decoder_dim >= 1024
    if big:  # one engine per (model, precision, options); logits tracing always on (7 MB)
        kw.setdefault("trace_logits", True)
        key = (repr(c), g.weight_seed, precision, tuple(sorted(kw.items())))
        if key in _BIG:
            return _BIG[key]
    m = VALLE(c.decoder_dim, c.nhead, c.num_decoder_layers, norm_first=c.norm_first, add_prenet=c.add_prenet, prefix_mode=c.prefix_mode,
              share_embedding=c.share_embedding,
              nar_scale_factor=c.scale_factor, prepend_bos=c.prepend_bos, num_quantizers=c.num_quantizers, precision=precision, max_text=128,
              max_audio=1792 if big else 1280, print_eos=False, **kw)
    m.load_state_dict(g.state_dict())
    m = m.to("cuda:0").eval()
    if big:
        _BIG[key] = m
    return m


def _run(m, g, **kw):
    return m.inference(g.x.cuda(), g.x_lens.cuda(), g.y.cuda(), g.enroll_x_lens, top_k=g.top_k,
                       temperature=g.temperature, exp_noise=g.exp_noise, **kw).cpu()


@pytest.mark.parametrize("name", SMALL)
def test_fp32_engine_reproduces_reference_codes(name):
    g = Golden(name)
    m = _model(g, "fp32", trace_logits=True)
    codes = _run(m, g)
    assert codes.shape == g.codes.shape
    assert torch.equal(codes, g.codes)  # (1,T,Q) int64: bit-exact
    e = m.engine()
    for step, ref in zip(g.ar_probe_steps, g.ar_probe_logits):
        got = e.read("ar_logits", (1025,), offset_bytes=step * 1025 * 4)
        assert (got - ref).abs().max() <= 2e-4, step
    if g.nar_probe_logits is not None:
        got = e.read("nar_logits", (8, 1024))  # last stage, first 8 frames
        assert (got - g.nar_probe_logits[-1]).abs().max() <= 2e-3


@pytest.mark.parametrize("name,T", [("cfg1_topk10", 753), ("cfg4_s94_topk10", 1505)])
def test_fp32_engine_full_length(name, T):
    """BASELINE.json configs[1] geometry: d=1024 L=12, S=47, P=225 -> 753 frames x 8 codebooks, top-k 10; and configs[4]'s
    utterance on the same model: S=94 -> 1505 frames (20 s), context 319 -> 1824 rows."""
    g = Golden(name)
    m = _model(g, "fp32", trace_logits=True)
    codes = _run(m, g)
    assert codes.shape == (1, T, 8)
    e = m.engine()
    for step, ref in zip(g.ar_probe_steps, g.ar_probe_logits):
        got = e.read("ar_logits", (1025,), offset_bytes=step * 1025 * 4)
        assert (got - ref).abs().max() <= 5e-4, step
    assert torch.equal(codes[..., 0], g.codes[..., 0])  # AR tokens: bit-exact over all 753 steps
    agree = (codes == g.codes).float().mean().item()
    assert agree == 1.0, f"NAR codes agreement {agree}"


def test_sharded_step_matches_plain_step_beyond_one_key_pass(monkeypatch):
    """The XCD-sharded decode step (ar_tp.hpp) keeps 16 x 128 cached keys per head in registers; a longer context takes further
    passes with plain loads.  d=1024 / 16 heads / 2 layers in fp32, S=60, P=900, 1300 forced tokens: context 961 -> 2260 rows.
    The sharded step and the plain five-launch step (VX_AR_TP=0, itself pinned by every fixture) must give the
    same logits at every traced pass up to summation order, and the same argmax wherever the margin exceeds that."""
    from valle_amd.config import ModelConfig
    from valle_amd.models import VALLE
    from valle_amd.weights import synthetic_inputs, synthetic_state_dict

    import __graft_entry__ as ge

    ge.build()
    cfg = ModelConfig(decoder_dim=1024, nhead=16, num_decoder_layers=2, prefix_mode=1)
    sd = synthetic_state_dict(cfg, 3)
    x, xl, y = synthetic_inputs(60, 900, 8, seed=9)
    forced = torch.randint(0, 1024, (1300,), generator=torch.Generator().manual_seed(4))
    rows = []
    for tp in ("1", "0"):
        monkeypatch.setenv("VX_AR_TP", tp)
        m = VALLE(1024, 16, 2, prefix_mode=1, precision="fp32", max_text=64, max_audio=2304, print_eos=False, trace_logits=True)
        m.load_state_dict(sd)
        m.to("cuda:0").eval()
        e = m.engine()
        e.ar_prefill(x[0], y[0, :, 0].contiguous())
        e.ar_decode(top_k=1, forced=forced)
        toks, reason, n_pass = e.ar_result()
        assert torch.equal(toks, forced) and n_pass == 1301
        rows.append(e.read("ar_logits", (n_pass, 1025)).clone())
        del e, m
    a, b = rows
    scale = b.abs().amax(1)
    err = (a - b).abs().amax(1)
    assert bool((err <= 2e-5 * scale + 1e-6).all()), float((err / scale).max())
    top2 = b.topk(2, dim=1)[0]
    decided = (top2[:, 0] - top2[:, 1]) > 4e-5 * scale
    assert bool((a.argmax(1) == b.argmax(1))[decided].all())


def test_sharded_step_does_not_depend_on_uninitialised_memory():
    """VX_POISON=1 fills every fresh device allocation (including the slices of the small-block arena) with 0xFF bytes before the
    engine initialises it: the XCD-sharded decode step's granule scratch, accumulators and re-laid-out weights must all be written
    before they are read - same codes with and without the poison (d = 1024 / 16 heads / 2 layers, bf16, graph replay)."""
    import json
    import subprocess
    import sys

    from conftest import ROOT

    script = (
        "import sys, json, torch; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as ge; ge.build()\n"
        "from valle_amd.config import ModelConfig\n"
        "from valle_amd.models import VALLE\n"
        "from valle_amd.weights import synthetic_inputs, synthetic_state_dict\n"
        "cfg = ModelConfig(decoder_dim=1024, nhead=16, num_decoder_layers=2, prefix_mode=1)\n"
        "m = VALLE(1024, 16, 2, prefix_mode=1, precision='bf16', max_text=32, max_audio=256, print_eos=False)\n"
        "m.load_state_dict(synthetic_state_dict(cfg, 3)); m.to('cuda:0').eval()\n"
        "x, xl, y = synthetic_inputs(5, 40, 8, seed=2)\n"
        "out = []\n"
        "for seed in (1, 2):\n"
        "    torch.manual_seed(seed); out.append(m.inference(x.cuda(), xl.cuda(), y.cuda(), None, top_k=5).flatten().tolist())\n"
        "print(json.dumps(out))\n" % ROOT)
    outs = []
    for poison in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, VX_POISON=poison), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]
    assert all(len(seq) == 81 * 8 and all(0 <= v < 1024 for v in seq) for seq in outs[0])


def test_graph_and_eager_steps_agree():
    g = Golden("cfg0_topk10")
    a = _run(_model(g, "fp32"), g)
    b = _run(_model(g, "fp32", no_graph=True), g)
    assert torch.equal(a, b) and torch.equal(a, g.codes)


def test_device_rng_is_deterministic_per_seed():
    g = Golden("cfg0_greedy")
    m = _model(g, "bf16")
    outs = []
    for seed in (7, 7, 8):
        torch.manual_seed(seed)
        outs.append(m.inference(g.x.cuda(), g.x_lens.cuda(), g.y.cuda(), None, top_k=20, temperature=1.0).cpu())
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], outs[2])
    assert outs[0].shape == g.codes.shape and int(outs[0].max()) < 1024 and int(outs[0].min()) >= 0


def test_torch_cpu_sampling_mode_follows_global_generator():
    g = Golden("cfg0_topk10")
    m = _model(g, "fp32", sampling="torch_cpu")
    torch.manual_seed(g.sample_seed)
    codes = m.inference(g.x.cuda(), g.x_lens.cuda(), g.y.cuda(), None, top_k=g.top_k, temperature=g.temperature).cpu()
    assert torch.equal(codes, g.codes)
    # generator left where the reference leaves it: n_pass draws consumed
    nxt = torch.empty(1, 1025).exponential_(1)
    torch.manual_seed(g.sample_seed)
    for _ in range(g.n_pass):
        torch.empty(1, 1025).exponential_(1)
    assert torch.equal(nxt, torch.empty(1, 1025).exponential_(1))


@pytest.mark.parametrize("name,simple", [("cfg0_topk10", False), ("cfg0_topk10", True), ("tiny_mode0", False),
                                         ("tiny_mode2_q6", False), ("cfg0_postnorm", False), ("cfg0_postnorm", True),
                                         ("cfg1_topk10", False), ("cfg4_s94_topk10", False), ("reftest_mode0", False),
                                         ("reftest_mode1_scale05_bos_q7", False)])
def test_bf16_engine_teacher_forced(name, simple):
    from oracle import valle_oracle as vo

    g = Golden(name)
    m = _model(g, "bf16", trace_logits=True, simple_rows=simple)
    e = m.engine()
    bos = int(g.cfg.prepend_bos)
    text, prompts = g.x[0], g.y[0, :, : g.cfg.num_quantizers].contiguous()
    forced = g.codes[0, :, 0].contiguous()
    e.ar_prefill(text, prompts[:, 0].contiguous())
    e.ar_decode(top_k=g.top_k, temperature=g.temperature, exp_noise=g.exp_noise, forced=forced)
    toks, reason, n_pass = e.ar_result()
    assert torch.equal(toks, forced) and n_pass == forced.numel() + 1
    # fp32 oracle, teacher-forced with the same tokens
    tr = {}
    big = g.cfg.decoder_dim >= 1024
    steps = g.ar_probe_steps if big else list(range(0, n_pass, 7))
    if big:
        ref_logits = {s: r for s, r in zip(g.ar_probe_steps, g.ar_probe_logits)}
    else:
        vo.inference_cached(g.oracle(), g.x, g.x_lens, g.y, g.enroll_x_lens, g.top_k, g.temperature, g.exp_noise, trace=tr,
                            forced=forced, skip_nar=True)
        ref_logits = {s: tr["ar_logits"][s] for s in steps}
    got_all = e.read("ar_logits", (n_pass, 1025))
    # tolerance: bf16 weights/KV (2^-9 relative per element) through L layers; stated as a fraction of the
    # logits' own scale
    worst = 0.0
    for s in steps:
        ref = ref_logits[s]
        tol = 0.03 * float(ref.abs().max())
        err = float((got_all[s] - ref).abs().max())
        worst = max(worst, err / float(ref.abs().max()))
        assert err <= tol, (s, err, tol)
        # index selection is exact wherever the reference's margin exceeds the tolerance
        top2 = ref.topk(2)[0]
        if float(top2[0] - top2[1]) > 2 * tol:
            assert int(got_all[s].argmax()) == int(ref.argmax())
    # NAR: every stage is fed the reference's codes of the earlier stages (forced_codes), so each stage sees exactly the
    # reference's input and rounding cannot compound; per-stage argmax agreement against the reference codes (the margin
    # rule proper is test_nar_stages_teacher_forced_margin_rule)
    text_nar = text if g.cfg.prefix_mode not in (2, 4) else torch.cat([text[:1], text[int(g.enroll_x_lens.max()) - 1:]])
    codes = e.nar(text_nar, prompts, forced, forced_codes=g.codes[0]).cpu()
    if g.cfg.num_quantizers > 1:
        per_stage = (codes[:, 1:] == g.codes[0, :, 1:]).float().mean(0)
        print(name, "simple" if simple else "mfma", "AR worst rel err %.4f" % worst, "NAR agreement per stage", [round(float(v), 4) for v in per_stage])
        assert float(per_stage.min()) >= 0.93, per_stage


NAR_REL_TOL = 0.03  # bf16 operands through L layers, as a fraction of a logits row's largest magnitude (same as the AR side)


@pytest.mark.parametrize("name,precision", [("tiny_mode0", "fp32"), ("tiny_mode0", "bf16"), ("cfg0_topk10", "bf16"),
                                            ("cfg1_topk10", "bf16"), ("cfg4_s94_topk10", "bf16")])
def test_nar_stages_teacher_forced_margin_rule(name, precision):
    """North-star rule on the NAR side, for the precision the benchmark runs: every stage is fed the reference's own codes of
    the earlier stages (vx_nar_ex forced_codes: exactly the input the reference gave that stage, valle.py:1133-1134), so
    rounding cannot compound across stages.  Per stage and row: the engine's argmax must equal the reference's wherever the
    reference's top-2 margin exceeds 2 x tolerance; the logits of the recorded rows must lie within the tolerance; overall
    agreement is bounded from below by what is measured (not by the margin rule alone)."""
    from conftest import NarStats

    g = Golden(name)
    ns = NarStats(name)
    m = _model(g, precision)
    e = m.engine()
    Q = g.cfg.num_quantizers
    text, prompts = g.x[0], g.y[0, :, :Q].contiguous()
    ref = g.codes[0]
    codes, lg = e.nar(text, prompts, ref[:, 0].contiguous(), forced_codes=ref, stage_logits=True)
    codes = codes.cpu()
    assert torch.equal(codes[:, 0], ref[:, 0])
    rel = 1e-5 if precision == "fp32" else NAR_REL_TOL
    # (a) logits of the recorded rows within the tolerance
    worst = 0.0
    for i in range(Q - 1):
        err = (lg[i, ns.rows] - ns.row_logits[i]).abs().amax(1)
        scale = ns.absmax[i, ns.rows]
        worst = max(worst, float((err / scale).max()))
        assert bool((err <= rel * scale + 1e-6).all()), (i, float((err / scale).max()))
    # (b) index selection exact wherever the reference's margin exceeds 2 x tolerance
    eq = (codes[:, 1:] == ref[:, 1:]).t()  # (Q-1, T)
    decided = ns.decided(rel)
    assert bool(eq[decided].all()), f"{int((~eq[decided]).sum())} decided rows flipped"
    # (c) plain agreement, per stage
    per_stage = eq.float().mean(1)
    print(name, precision, "worst rel err %.4f" % worst, "decided %.3f" % float(decided.float().mean()),
          "agreement per stage", [round(float(v), 4) for v in per_stage])
    if precision == "fp32":
        assert bool(eq.all())
    else:
        assert float(per_stage.min()) >= 0.95, per_stage


FP8_AGREE_MIN = 0.88  # per-stage agreement with the reference's codes: measured 0.91-0.97 (d=1024), 0.90+ (d=256)
FP8_REL_TOL = 0.08  # MXFP8 (e4m3, 3 mantissa bits, one power-of-two scale per 32 k) operands in the QKV / FFN GEMMs of 12 layers


@pytest.mark.parametrize("name", ["cfg0_topk10", "cfg1_topk10", "cfg4_s94_topk10"])
def test_fp8_nar_stages_teacher_forced(name, monkeypatch):
    """VX_PREC_FP8_NAR (BASELINE configs[4]): the NAR stages' QKV / FFN1 / FFN2 GEMMs on MXFP8, everything else bf16.  Same
    protocol as the bf16 margin-rule test: every stage on the reference's inputs, logits of the recorded rows within the fp8
    tolerance, argmax exact wherever the reference's margin exceeds twice that tolerance, and the measured agreement reported.
    VX_MX_MIN_ROWS=1 sends one utterance's rows through the MXFP8 kernels (the product uses them from 4096 rows on)."""
    from conftest import NarStats

    monkeypatch.setenv("VX_MX_MIN_ROWS", "1")
    g = Golden(name)
    ns = NarStats(name)
    m = _model(g, "fp8nar")
    e = m.engine()
    Q = g.cfg.num_quantizers
    text, prompts = g.x[0], g.y[0, :, :Q].contiguous()
    ref = g.codes[0]
    codes, lg = e.nar(text, prompts, ref[:, 0].contiguous(), forced_codes=ref, stage_logits=True)
    codes = codes.cpu()
    worst = 0.0
    for i in range(Q - 1):
        err = (lg[i, ns.rows] - ns.row_logits[i]).abs().amax(1)
        scale = ns.absmax[i, ns.rows]
        worst = max(worst, float((err / scale).max()))
    eq = (codes[:, 1:] == ref[:, 1:]).t()
    decided = ns.decided(FP8_REL_TOL)
    per_stage = eq.float().mean(1)
    print(name, "fp8nar worst rel err %.4f" % worst, "decided %.3f" % float(decided.float().mean()),
          "flipped decided rows %d" % int((~eq[decided]).sum()), "agreement per stage", [round(float(v), 4) for v in per_stage])
    assert worst <= FP8_REL_TOL
    assert bool(eq[decided].all()), f"{int((~eq[decided]).sum())} decided rows flipped"
    assert float(per_stage.min()) >= FP8_AGREE_MIN, per_stage
    # the same utterance four times through the batched NAR (4352 concatenated rows: the product's MXFP8 path without the knob)
    monkeypatch.delenv("VX_MX_MIN_ROWS")
    if g.cfg.decoder_dim >= 1024:
        outs = e.nar_batch([text] * 4, [prompts] * 4, [ref[:, 0].contiguous()] * 4, forced_codes=[ref] * 4)
        for o in outs:
            eqb = (o.cpu()[:, 1:] == ref[:, 1:]).t()
            assert bool(eqb[decided].all()) and float(eqb.float().mean(1).min()) >= FP8_AGREE_MIN


@pytest.mark.parametrize("name", golden_names("continual"))
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_continual_matches_reference(name, precision):
    """VALLE.continual (valle.py:1139-1238; bin/infer.py:224-230): NAR stages only."""
    g = Golden(name)
    m = _model(g, precision)
    codes = m.continual(g.x.cuda(), g.x_lens.cuda(), g.y.cuda()).cpu()
    assert codes.shape == g.codes.shape
    assert torch.equal(codes[..., 0], g.codes[..., 0])
    if precision == "fp32":
        assert torch.equal(codes, g.codes)  # bit-exact
    else:  # bf16: stage by stage on the reference's inputs (vx_nar_ex, continual = 1)
        prefix_len = min(int(g.y.shape[1] * 0.5), 3 * 75)
        forced = g.codes[0]
        c2 = m.engine().nar(g.x[0], g.y[0, :prefix_len, :8].contiguous(), g.y[0, prefix_len:, 0].contiguous(), continual=True,
                            forced_codes=forced).cpu()
        per_stage = (c2[:, 1:] == forced[:, 1:]).float().mean(0)
        print(name, "continual bf16 agreement per stage", [round(float(v), 4) for v in per_stage])
        assert float(per_stage.min()) >= 0.93, per_stage


# ---- stop rule, exceptions and ragged sizes (valle.py:1044-1057) against the oracle ---------------------
def _tiny(precision="fp32", **kw):
    from valle_amd.config import ModelConfig
    from valle_amd.models import VALLE
    from valle_amd.weights import synthetic_state_dict

    import __graft_entry__ as ge

    ge.build()
    cfg = ModelConfig(decoder_dim=128, nhead=2, num_decoder_layers=2, prefix_mode=1)
    sd = synthetic_state_dict(cfg, 5)
    m = VALLE(128, 2, 2, prefix_mode=1, precision=precision, max_text=32, max_audio=600, print_eos=False, **kw)
    return cfg, sd, m


def _oracle(cfg, sd):
    from oracle import valle_oracle as vo

    return vo, vo.OracleModel(sd, cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers, cfg.prefix_mode, cfg.prepend_bos,
                              cfg.num_quantizers)


def test_eos_by_sample_stops_mid_sequence_like_the_oracle():
    from valle_amd.weights import synthetic_inputs

    cfg, sd, m = _tiny()
    sd["ar_predict_layer.weight"].zero_()  # all logits equal: the noise alone decides the sample
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    x, xl, y = synthetic_inputs(6, 9)
    noise = torch.ones(100, 1025)
    noise[:, 3] = 0.5      # token 3 wins every pass ...
    noise[7, 1024] = 1e-3  # ... until EOS wins pass 7 (valle.py:1046)
    vo, om = _oracle(cfg, sd)
    want = vo.inference_cached(om, x, xl, y, None, -100, 1.0, noise)
    got = m.inference(x.cuda(), xl.cuda(), y.cuda(), None, top_k=-100, exp_noise=noise).cpu()
    assert want.shape == (1, 7, 8) and torch.equal(got, want)
    assert m.engine().ar_result()[1] == 2  # VX_STOP_EOS_SAMPLE


def test_eos_at_first_pass_raises_syntax_error_like_the_reference():
    from valle_amd.weights import synthetic_inputs

    cfg, sd, m = _tiny()
    sd["ar_predict_layer.weight"].zero_()
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    x, xl, y = synthetic_inputs(6, 9)
    noise = torch.ones(4, 1025)
    noise[0, 1024] = 1e-3
    vo, om = _oracle(cfg, sd)
    with pytest.raises(SyntaxError):
        vo.inference_cached(om, x, xl, y, None, -100, 1.0, noise)
    with pytest.raises(SyntaxError, match="well trained model"):  # valle.py:1049-1052
        m.inference(x.cuda(), xl.cuda(), y.cuda(), None, top_k=-100, exp_noise=noise)


def test_eos_by_argmax():
    """valle.py:1045: the loop stops when argmax(logits) == EOS, whatever the sample is.  The EOS row of the predict layer is
    crafted from the oracle's own final hidden states: alpha x (the part of h_k orthogonal to h_0 .. h_{k-1}), so the EOS logit is
    ~0 at every earlier pass and top + 1 at pass k, while the noise makes the multinomial draw a chosen non-EOS token at every
    pass: only the argmax branch can stop the decode.  Engine == oracle, stop reason VX_STOP_EOS_ARGMAX."""
    from valle_amd.weights import synthetic_inputs

    cfg, sd, m = _tiny()
    x, xl, y = synthetic_inputs(5, 8)
    noise = torch.ones(16 * 5 + 2, 1025)
    toks = [(37 * p + 11) % 1000 for p in range(noise.shape[0])]
    for p, t in enumerate(toks):
        noise[p, t] = 1e-9  # p[t] / q[t] dwarfs every other ratio: token t is what pass p samples
    vo, om = _oracle(cfg, sd)
    tr = {}
    full = vo.inference_cached(om, x, xl, y, None, -100, 1.0, noise, trace=tr, skip_nar=True)
    assert full[0, :, 0].tolist() == toks[:81]
    H = torch.stack(tr["ar_hidden"])                        # (passes, d): independent of the predict layer
    top = torch.stack(tr["ar_logits"])[:, :1024].max(1)[0]  # best non-EOS logit of every pass
    k = 6
    B = H[:k]
    v = H[k] - B.t() @ torch.linalg.lstsq(B.t(), H[k].unsqueeze(1)).solution[:, 0]
    alpha = float(top[k] + 1.0) / float(v @ H[k])
    eos = alpha * (H[: k + 1] @ v)
    assert bool((eos[:k] < top[:k] - 0.5).all()) and float(eos[k]) > float(top[k]) + 0.5
    sd["ar_predict_layer.weight"][1024] = alpha * v
    vo, om = _oracle(cfg, sd)
    want = vo.inference_cached(om, x, xl, y, None, -100, 1.0, noise)
    assert want.shape == (1, k, 8)  # passes 0..k-1 appended a token, pass k stopped by argmax
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    got = m.inference(x.cuda(), xl.cuda(), y.cuda(), None, top_k=-100, exp_noise=noise).cpu()
    assert torch.equal(got, want)
    e = m.engine()
    assert e.ar_result()[1] == 1  # VX_STOP_EOS_ARGMAX
    n_pass = k + 1
    assert int(e.read("ar_argmax", (n_pass,), dtype=torch.int32)[k]) == 1024
    assert int(e.read("ar_sampled", (n_pass,), dtype=torch.int32)[k]) == toks[k]  # the sample was NOT EOS


def test_long_text_is_not_refused_by_the_worst_case_bound():
    """The stop rule's worst case (16 S + 1 tokens, valle.py:1047) may exceed max_audio as long as the decode really stops
    earlier (a trained model stops at EOS): S = 31, P = 200 needs 200 + 497 rows in the worst case, the cache has 600, EOS is
    sampled at pass 9.  Only a decode that fills the cache is a capacity error (test_capacity_and_index_errors_are_loud)."""
    from valle_amd.weights import synthetic_inputs

    cfg, sd, m = _tiny()
    sd["ar_predict_layer.weight"].zero_()
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    x, xl, y = synthetic_inputs(31, 200)
    noise = torch.ones(100, 1025)
    noise[:, 5] = 0.5
    noise[9, 1024] = 1e-3
    vo, om = _oracle(cfg, sd)
    want = vo.inference_cached(om, x, xl, y, None, -100, 1.0, noise)
    got = m.inference(x.cuda(), xl.cuda(), y.cuda(), None, top_k=-100, exp_noise=noise).cpu()
    assert want.shape == (1, 9, 8) and torch.equal(got, want)


@pytest.mark.parametrize("S,P", [(1, 1), (2, 33), (31, 3)])
def test_ragged_sizes_match_oracle(S, P):
    from valle_amd.weights import synthetic_inputs

    cfg, sd, m = _tiny()
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    x, xl, y = synthetic_inputs(S, P, seed=S * 100 + P)
    if S == 1:
        x[0, 0] = 1
    vo, om = _oracle(cfg, sd)
    want = vo.inference_cached(om, x, xl, y, None, 1, 1.0, None)
    got = m.inference(x.cuda(), xl.cuda(), y.cuda(), None, top_k=1).cpu()
    assert want.shape == (1, 16 * S + 1, 8)
    assert torch.equal(got, want)


def test_capacity_and_index_errors_are_loud():
    from valle_amd.engine import VxError
    from valle_amd.weights import synthetic_inputs

    cfg, sd, m = _tiny()
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    x, xl, y = synthetic_inputs(40, 9)  # S > max_text = 32
    with pytest.raises(VxError, match="capacity"):
        m.inference(x.cuda(), xl.cuda(), y.cuda(), None, top_k=1)
    x, xl, y = synthetic_inputs(30, 200)  # 200 + 16*30+1 > max_audio = 600
    with pytest.raises(VxError, match="capacity"):
        m.inference(x.cuda(), xl.cuda(), y.cuda(), None, top_k=1)
    x, xl, y = synthetic_inputs(4, 9)
    x[0, 1] = 600
    with pytest.raises(IndexError):  # nn.Embedding's error in the reference
        m.inference(x.cuda(), xl.cuda(), y.cuda(), None, top_k=1)


def test_max_new_tokens_extension():
    from valle_amd.weights import synthetic_inputs

    cfg, sd, m = _tiny()
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    x, xl, y = synthetic_inputs(6, 9)
    full = m.inference(x.cuda(), xl.cuda(), y.cuda(), None, top_k=1).cpu()
    part = m.inference(x.cuda(), xl.cuda(), y.cuda(), None, top_k=1, max_new_tokens=11).cpu()
    assert part.shape == (1, 11, 8)
    assert torch.equal(part[..., 0], full[:, :11, 0])  # same AR prefix (NAR differs: it sees fewer frames)


@pytest.mark.parametrize("seed", list(range(42)))
def test_random_option_walk_matches_oracle(seed):
    """Randomised constructor options / sizes / sampling parameters on a tiny model: the fp32 engine must produce the
    oracle's codes exactly (the oracle is pinned to the reference on the committed fixtures; this widens the option
    space the fixtures sample; oracle/check_random_walk.py ran the same 42 configurations through the unmodified reference
    and asserted oracle == reference)."""
    import random

    from oracle import valle_oracle as vo
    from valle_amd.config import ModelConfig
    from valle_amd.models import VALLE
    from valle_amd.weights import synthetic_inputs, synthetic_state_dict
    import __graft_entry__ as ge

    ge.build()
    rnd = random.Random(1000 + seed)
    mode = rnd.choice([0, 1, 2, 4])
    bos = rnd.random() < 0.4
    Q = rnd.choice([1, 2, 3, 5, 8])
    kw = dict(decoder_dim=128, nhead=2, num_decoder_layers=rnd.choice([1, 2, 3]), prefix_mode=mode, prepend_bos=bos,
              num_quantizers=Q, share_embedding=rnd.random() < 0.7, norm_first=rnd.random() < 0.6, add_prenet=rnd.random() < 0.3)
    cfg = ModelConfig(**kw)
    S = rnd.randint(3, 12)
    P = rnd.choice([0, 1, 5, 17]) if bos else rnd.choice([1, 2, 9, 23])
    top_k = rnd.choice([-100, 1, 2, 7, 1025])
    temp = rnd.choice([1.0, 0.6, 1.7])
    enroll = torch.tensor([rnd.randint(2, S - 1)], dtype=torch.int32) if mode in (2, 4) else None
    if seed >= 30:  # seeds 30+: small head sizes (the reference's own test runs head_dim 4) and scaled NAR stacks
        dd, nh = rnd.choice([(64, 16), (64, 8), (64, 4), (64, 2), (128, 4), (32, 8)])
        kw.update(decoder_dim=dd, nhead=nh, num_decoder_layers=rnd.choice([2, 4]))
        if Q > 1 and rnd.random() < 0.5:
            kw.update(scale_factor=0.5)
        cfg = ModelConfig(**kw)
    sd = synthetic_state_dict(cfg, seed=seed)
    x, xl, y = synthetic_inputs(S, P, 8, seed=50 + seed)
    om = vo.OracleModel(sd, cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers, mode, bos, Q, cfg.scale_factor, cfg.norm_first, cfg.add_prenet)
    noise = None
    if top_k != 1:  # the draws torch.multinomial makes in the reference after torch.manual_seed(7 + seed): one (1,1025) per pass
        torch.manual_seed(7 + seed)
        noise = torch.stack([torch.empty(1, 1025).exponential_(1)[0] for _ in range(16 * S + 3)])
    want = vo.inference_cached(om, x, xl, y, enroll, top_k, temp, noise)
    m = VALLE(cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers, norm_first=cfg.norm_first, add_prenet=cfg.add_prenet, prefix_mode=mode,
              share_embedding=cfg.share_embedding, nar_scale_factor=cfg.scale_factor, prepend_bos=bos, num_quantizers=Q, precision="fp32", max_text=32, max_audio=400,
              print_eos=False)
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    got = m.inference(x.cuda(), xl.cuda(), y.cuda(), enroll, top_k=top_k, temperature=temp,
                      exp_noise=None if noise is None else noise.cuda()).cpu()
    assert got.shape == want.shape, (kw, S, P, top_k, temp)
    assert torch.equal(got, want), (kw, S, P, top_k, temp)


def test_valle_like_the_reference_test():
    """The reference's own `test_valle` (valle/tests/valle_test.py:90-135), inference half: decoder_dim 64 / nhead 16 (head_dim 4),
    4 layers, post-norm, prenets, numpy-random text (8) and prompt (16 x 8), prefix modes 0 / 1 / 2 with scale_factor 0.5 from
    the second iteration on, prepend_bos toggling and one quantizer fewer each time, default sampling (top_k=-100).  The
    reference only checks that it runs; here every iteration must also equal the oracle on the same weights and draws."""
    import numpy as np

    from oracle import valle_oracle as vo
    from valle_amd.models import get_model
    import __graft_entry__ as ge

    ge.build()
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.randint(0, 100, size=[4, 8]))
    x_lens = torch.from_numpy(rs.randint(4, 8, size=[4]))
    x_lens[-1] = 8
    enroll_x_lens = torch.from_numpy(rs.randint(1, 3, size=[4]))
    y = torch.from_numpy(rs.randint(0, 1000, size=[4, 16, 8]))

    params = dict(decoder_dim=64, nhead=16, num_decoder_layers=4, norm_first=False, add_prenet=True, model_name="VALL-E",
                  share_embedding=True, scale_factor=1.0, prepend_bos=False, num_quantizers=8, precision="fp32", sampling="torch_cpu",
                  max_text=32, max_audio=400)
    for it, mode in enumerate([0, 1, 2]):
        params["prefix_mode"] = mode
        torch.manual_seed(100 + it)  # the constructor draws its random-init seed from the global generator, like nn.Module
        model = get_model(params)
        model.print_eos = False
        model.to("cuda:0")
        model.eval()
        torch.manual_seed(7 + it)
        codes = model.inference(x[-1:].cuda(), x_lens[-1:].cuda(), y[-1:].cuda(), enroll_x_lens=enroll_x_lens)
        Q = params["num_quantizers"]
        assert codes.ndim == 3 and codes.shape[0] == 1 and codes.shape[2] == Q and codes.shape[1] >= 1
        assert int(codes.min()) >= 0 and int(codes.max()) < 1024

        cfg = model.cfg
        om = vo.OracleModel(model.state_dict(), 64, 16, 4, mode, cfg.prepend_bos, Q, cfg.scale_factor, False, True)
        torch.manual_seed(7 + it)
        noise = torch.stack([torch.empty(1, 1025).exponential_(1)[0] for _ in range(16 * 8 + 3)])
        want = vo.inference_cached(om, x[-1:], x_lens[-1:], y[-1:], enroll_x_lens, -100, 1.0, noise)
        assert torch.equal(codes.cpu(), want), (it, mode)

        params["scale_factor"] = 0.5
        params["prepend_bos"] = not params["prepend_bos"]
        params["num_quantizers"] -= 1


# ---- VALL-F (valle.py:566-710) --------------------------------------------------------------------
VALLF_NAMES = golden_names("vallf")


def _model_f(g, precision, **kw):
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.models import VALLF, get_model

    c = g.cfg
    m = get_model(dict(model_name="VALL-F", decoder_dim=c.decoder_dim, nhead=c.nhead, num_decoder_layers=c.num_decoder_layers,
                       scale_factor=c.scale_factor, norm_first=c.norm_first, add_prenet=c.add_prenet, prefix_mode=c.prefix_mode,
                       share_embedding=c.share_embedding, prepend_bos=c.prepend_bos, num_quantizers=c.num_quantizers,
                       precision=precision, max_text=128, max_audio=1280))
    assert isinstance(m, VALLF)
    m.print_eos = False
    for k, v in kw.items():
        m.engine_opts[k] = v
    m.load_state_dict(g.state_dict())
    return m.to("cuda:0").eval()


@pytest.mark.parametrize("name", VALLF_NAMES)
def test_vallf_fp32_engine_reproduces_reference_codes(name):
    """The fixtures are the reference's own VALLF layers run under the torch-1.13.1 decoder loop (oracle/ref_harness.py); the
    fp32 engine must reproduce their codes bit for bit: KV-cached causal self-attention over the audio rows, cross-attention
    over the text memory projected once, three norms per layer, pre- and post-norm, prenets, prefix modes 0/1/2/4."""
    g = Golden(name)
    m = _model_f(g, "fp32", trace_logits=True)
    codes = _run(m, g)
    assert codes.shape == g.codes.shape
    assert torch.equal(codes, g.codes)
    e = m.engine()
    c = g.cfg  # the step's shape: sampler, 8 launches per layer (the 5 of a VALL-E layer + the cross-attention block), head
    assert e.timings()["step_kernels"] == 8 * c.num_decoder_layers + 2 + (3 if c.add_prenet else 0)
    for step, ref in zip(g.ar_probe_steps, g.ar_probe_logits):
        got = e.read("ar_logits", (1025,), offset_bytes=step * 1025 * 4)
        assert (got - ref).abs().max() <= 2e-4, step
    if g.nar_probe_logits is not None:
        got = e.read("nar_logits", (8, 1024))
        assert (got - g.nar_probe_logits[-1]).abs().max() <= 2e-3


def test_vallf_graph_and_eager_steps_agree():
    g = Golden("vallf_mode1")
    a = _run(_model_f(g, "fp32"), g)
    b = _run(_model_f(g, "fp32", no_graph=True), g)
    assert torch.equal(a, b) and torch.equal(a, g.codes)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_vallf_one_model_serves_texts_of_different_lengths(precision):
    """valle/bin/infer.py loops over texts with ONE model; the decode step is captured once per engine.  The cross-attention
    length must follow the current utterance (it is read from the decode state, not frozen into the captured launch): the
    fixture's utterance (S = 7), then a longer text (S = 13), then a shorter one (S = 4), then the fixture again, each against
    the oracle on the same model (fp32: bit-exact codes; bf16: identical to a fresh engine's, i.e. no state leaks across calls)."""
    from oracle import valle_oracle as vo
    from valle_amd.weights import synthetic_inputs

    g = Golden("vallf_mode1")
    m = _model_f(g, precision)
    om = g.oracle()
    utts = [(g.x, g.x_lens, g.y), synthetic_inputs(13, 9, 8, seed=77), synthetic_inputs(4, 21, 8, seed=78), (g.x, g.x_lens, g.y)]
    for i, (x, xl, y) in enumerate(utts):
        got = m.inference(x.cuda(), xl.cuda(), y.cuda(), None, top_k=1).cpu()
        if precision == "fp32":
            want = vo.inference_f(om, x, xl, y, None, 1, 1.0, None)
        else:
            want = _model_f(g, precision).inference(x.cuda(), xl.cuda(), y.cuda(), None, top_k=1).cpu()
        assert torch.equal(got, want), i


@pytest.mark.parametrize("name,simple", [("vallf_cfg0_topk10", False), ("vallf_cfg0_topk10", True), ("vallf_postnorm_mode4_bos", False),
                                         ("vallf_reftest_mode2_bos_q3", False)])
def test_vallf_bf16_engine_teacher_forced(name, simple):
    """bf16 VALL-F engine, teacher-forced with the reference's tokens: AR logits within 3 % of a row's scale and argmax equal
    wherever the reference's margin exceeds twice that; NAR stages fed the reference's earlier codes, per-stage agreement."""
    from oracle import valle_oracle as vo

    g = Golden(name)
    m = _model_f(g, "bf16", trace_logits=True, simple_rows=simple)
    e = m.engine()
    Q = g.cfg.num_quantizers
    text, prompts = g.x[0], g.y[0, :, :Q].contiguous()
    forced = g.codes[0, :, 0].contiguous()
    e.ar_prefill(text, prompts[:, 0].contiguous())
    e.ar_decode(top_k=g.top_k, temperature=g.temperature, exp_noise=g.exp_noise, forced=forced)
    toks, reason, n_pass = e.ar_result()
    assert torch.equal(toks, forced) and n_pass == forced.numel() + 1
    tr = {}
    # fp32 oracle, teacher-forced with the same tokens (AR part only: a one-quantizer view of the same weights)
    c = g.cfg
    m1 = vo.OracleModelF(g.state_dict(), c.decoder_dim, c.nhead, c.num_decoder_layers, prefix_mode=c.prefix_mode, prepend_bos=c.prepend_bos,
                         num_quantizers=1, nar_scale_factor=c.scale_factor, norm_first=c.norm_first, add_prenet=c.add_prenet)
    vo.inference_f(m1, g.x, g.x_lens, g.y, g.enroll_x_lens, g.top_k, g.temperature, g.exp_noise, trace=tr, forced=forced)
    got_all = e.read("ar_logits", (n_pass, 1025))
    worst = 0.0
    for s in range(0, n_pass, 7):
        ref = tr["ar_logits"][s]
        tol = 0.03 * float(ref.abs().max())
        err = float((got_all[s] - ref).abs().max())
        worst = max(worst, err / float(ref.abs().max()))
        assert err <= tol, (s, err, tol)
        top2 = ref.topk(2)[0]
        if float(top2[0] - top2[1]) > 2 * tol:
            assert int(got_all[s].argmax()) == int(ref.argmax())
    if Q > 1:
        text_nar = text if c.prefix_mode not in (2, 4) else torch.cat([text[:1], text[int(g.enroll_x_lens.max()) - 1:]])
        codes = e.nar(text_nar, prompts, forced, forced_codes=g.codes[0]).cpu()
        per_stage = (codes[:, 1:] == g.codes[0, :, 1:]).float().mean(0)
        print(name, "simple" if simple else "mfma", "AR worst rel err %.4f" % worst, "NAR agreement per stage", [round(float(v), 4) for v in per_stage])
        assert float(per_stage.min()) >= 0.90, per_stage


def test_vallf_has_no_continual_and_no_batch():
    g = Golden("vallf_mode1")
    m = _model_f(g, "fp32")
    with pytest.raises(AttributeError):
        m.continual(g.x, g.x_lens, g.y)
    with pytest.raises(NotImplementedError):
        m.inference_batch([(g.x, g.x_lens, g.y)])


@pytest.mark.parametrize("seed", range(36))
def test_vallf_random_option_walk_matches_oracle(seed):
    """The randomised option walk of test_random_option_walk_matches_oracle with --model-name VALL-F: the fp32 engine must produce
    the oracle's codes exactly.  oracle/check_random_walk.py --vallf ran the same 36 configurations through the reference's layers
    (torch-1.13.1 decoder loop, oracle/ref_harness.py) and asserted oracle == reference."""
    from oracle import valle_oracle as vo
    from oracle.check_random_walk import walk
    from valle_amd.config import ModelConfig
    from valle_amd.models import VALLF
    from valle_amd.weights import synthetic_inputs, synthetic_state_dict
    import __graft_entry__ as ge

    ge.build()
    kw, S, P, top_k, temp, enroll = walk(seed)
    cfg = ModelConfig(model_name="VALL-F", **kw)
    sd = synthetic_state_dict(cfg, seed=seed)
    x, xl, y = synthetic_inputs(S, P, 8, seed=50 + seed)
    om = vo.OracleModelF(sd, cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers, prefix_mode=cfg.prefix_mode, prepend_bos=cfg.prepend_bos,
                         num_quantizers=cfg.num_quantizers, nar_scale_factor=cfg.scale_factor, norm_first=cfg.norm_first, add_prenet=cfg.add_prenet)
    noise = None
    if top_k != 1:
        torch.manual_seed(7 + seed)
        noise = torch.stack([torch.empty(1, 1025).exponential_(1)[0] for _ in range(16 * S + 3)])
    want = vo.inference_f(om, x, xl, y, enroll, top_k, temp, noise)
    m = VALLF(cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers, norm_first=cfg.norm_first, add_prenet=cfg.add_prenet, prefix_mode=cfg.prefix_mode,
              share_embedding=cfg.share_embedding, nar_scale_factor=cfg.scale_factor, prepend_bos=cfg.prepend_bos, num_quantizers=cfg.num_quantizers,
              precision="fp32", max_text=32, max_audio=400, print_eos=False)
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    got = m.inference(x.cuda(), xl.cuda(), y.cuda(), enroll, top_k=top_k, temperature=temp,
                      exp_noise=None if noise is None else noise.cuda()).cpu()
    assert got.shape == want.shape, (kw, S, P, top_k, temp)
    assert torch.equal(got, want), (kw, S, P, top_k, temp)
