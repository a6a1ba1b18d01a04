"""GPU: the two roles of the XCD-sharded attention launch (ar_tp.hpp tp_attn_kernel).  Of a head's 16 workgroups the eight key
splits project q alone, run the key loop, publish their partial and exit; the other eight project k and v, append them to the
cache, gather the partials and apply two 64-row slices of the out-projection each, head 0's also the carry and the bias of all
1024 rows.  One d = 1024 / 16-head / 2-layer model as in test_gpu_tp_attn_splits.py (layer 0 = the FIRST instantiation),
synthetic weights with the q rows sharpened, teacher-forced runs of at most 11 tokens.

(1) Determinism of the hand-overs: the same prefill and forced decode three times on one engine and once on a second one give
    bitwise equal traced logits and KV caches, bf16 and fp32, at cached-row counts 2..9 (splits without a key and with one; the
    q-only gather of splits 0..6) and 1023..1033 (the second key pass).
(2) Role coverage of k / v: every newly appended K and V row of every layer and head against the five-launch step's
    (VX_AR_TP=0) under the rules of test_gpu_tp_attn_splits.py applied to a row of 64 channels (fp32: 2e-5 of the row's largest
    value + 1e-6; bf16: 3 % of it - both steps round the row to bf16 on their own), and every one of the 64 channels differs
    from what the cache held before the decode: a channel that no role projects stays stale, one projected into another's
    slot leaves its own stale.
(3) Bias and carry once: out_proj.bias = 0.5 x row index on one layer (either), fp32 logits against the five-launch step
    within 2e-5 of a row's largest logit + 1e-6.  The bias reaches 511.5 in the residual stream, where a doubled or a missing
    lead (carry + bias) in any 64-row block moves the normalised row, and the logits, by far more than that.
(4) A decode that has finished keeps replaying the step until the host's next poll: with an EOS row that wins the first
    argmax the decode stops in its first launch and the rest of the chunk runs behind it; the cache must stay bit for bit what
    the prefill left and the traced logits what a forced decode of the same prefill traced."""
import pytest
import torch

pytestmark = pytest.mark.gpu

L = 2
Q_SHARPEN = 4.0
# (prepend_bos, prompt rows P, forced tokens): text S = 1, so the first decode pass has n = 1 + bos + P cached rows
RUNS = [(True, 0, 8), (False, 1022, 11)]
MAX_AUDIO = 1022 + 11 + 8


def _state_dict(bos, seed=5):
    from valle_amd.config import ModelConfig
    from valle_amd.weights import synthetic_state_dict

    cfg = ModelConfig(decoder_dim=1024, nhead=16, num_decoder_layers=L, prefix_mode=1, prepend_bos=bos, num_quantizers=1)
    sd = synthetic_state_dict(cfg, seed)
    for li in range(L):
        sd[f"ar_decoder.layers.{li}.self_attn.in_proj_weight"][:1024] *= Q_SHARPEN
    return cfg, sd


def _engine(monkeypatch, precision, bos, tp, sd=None):
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.engine import Engine

    if tp:
        monkeypatch.delenv("VX_AR_TP", raising=False)
    else:
        monkeypatch.setenv("VX_AR_TP", "0")
    cfg, sd0 = _state_dict(bos)
    e = Engine(cfg, precision, max_text=16, max_audio=MAX_AUDIO, trace_logits=True)
    e.load_state_dict(sd0 if sd is None else sd)
    return e


def _inputs(run):
    _, P, n = RUNS[run]
    g = torch.Generator().manual_seed(300 + run)
    return torch.randint(3, 100, (1,), generator=g), torch.randint(0, 1024, (P,), generator=g), torch.randint(0, 1024, (n,), generator=g)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _forced_decode(e, run, tp, pre=None):
    """Traced logits (n + 1, 1025) and the cache after a forced decode of RUNS[run]; `pre` (a list) receives the cache as the
    prefill left it."""
    text, prompt, forced = _inputs(run)
    e.ar_prefill(text, prompt)
    if pre is not None:
        pre.append(e.read_ar_kv())
    e.ar_decode(top_k=1, forced=forced)  # raises if the error word of the hand-overs is set
    toks, _, n_pass = e.ar_result()
    assert torch.equal(toks, forced) and n_pass == forced.numel() + 1
    want = 2 * L + 2 if tp else 5 * L + 2
    assert e.timings()["step_kernels"] == want, (tp, e.timings()["step_kernels"])
    return e.read("ar_logits", (n_pass, 1025)).clone(), e.read_ar_kv()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_hand_overs_are_deterministic(monkeypatch, precision):
    for run, (bos, P, n) in enumerate(RUNS):
        got = []
        for eng in range(2):
            e = _engine(monkeypatch, precision, bos, True)
            try:
                for rep in range(3 if eng == 0 else 1):
                    got.append(_forced_decode(e, run, True))
            finally:
                e.close()
        rows = 1 + int(bos) + P + n  # text, bos, prompt and the appended rows: what lies behind them is nobody's
        for k, (lg, kv) in enumerate(got[1:], 1):
            assert torch.equal(_bits(lg), _bits(got[0][0])), f"run {run}: logits of repeat {k} differ"
            assert torch.equal(_bits(kv[:, :, :, :rows]), _bits(got[0][1][:, :, :, :rows])), f"run {run}: cache of repeat {k} differs"


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_every_new_kv_channel_is_projected_once(monkeypatch, precision):
    fails = []
    for run, (bos, P, n) in enumerate(RUNS):
        res = {}
        for tp in (True, False):
            e = _engine(monkeypatch, precision, bos, tp)
            try:
                pre = []
                _, kv = _forced_decode(e, run, tp, pre)
                res[tp] = (pre[0], kv)
            finally:
                e.close()
        n0 = 1 + int(bos) + P
        new = slice(n0, n0 + n)
        pre, kv = res[True]
        stale = _bits(kv[:, :, :, new]) == _bits(pre[:, :, :, new])
        if bool(stale.any()):
            li, w, h, r, c = (int(v) for v in stale.nonzero()[0])
            fails.append(f"run {run}: {int(stale.sum())} stale elements, first layer {li} {'KV'[w]} head {h} row {n0 + r} channel {c}")
        a, ref = kv[:, :, :, new].double(), res[False][1][:, :, :, new].double()
        scale = ref.abs().amax(-1, keepdim=True)
        tol = 2e-5 * scale + 1e-6 if precision == "fp32" else 0.03 * scale
        err = (a - ref).abs()
        print(f"\n{precision} run {run}: worst new-row error / row scale {float((err / scale).max()):.3g}")
        bad = err > tol
        if bool(bad.any()):
            li, w, h, r, c = (int(v) for v in bad.nonzero()[0])
            fails.append(f"run {run}: {int(bad.sum())} elements off, first layer {li} {'KV'[w]} head {h} row {n0 + r} channel {c}: "
                         f"{float(a[li, w, h, r, c]):.6g} vs {float(ref[li, w, h, r, c]):.6g}")
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("layer", [0, 1])
def test_out_projection_bias_and_carry_are_added_once(monkeypatch, layer):
    run = 0
    bos = RUNS[run][0]
    _, sd = _state_dict(bos)
    sd[f"ar_decoder.layers.{layer}.self_attn.out_proj.bias"] = 0.5 * torch.arange(1024, dtype=torch.float32)
    logits = {}
    for tp in (True, False):
        e = _engine(monkeypatch, "fp32", bos, tp, sd)
        try:
            logits[tp], _ = _forced_decode(e, run, tp)
        finally:
            e.close()
    a, ref = logits[True].double(), logits[False].double()
    scale = ref.abs().amax(1)
    err = (a - ref).abs().amax(1)
    print(f"\nlayer {layer}: worst err / scale {float((err / scale).max()):.3g}")
    assert bool((err <= 2e-5 * scale + 1e-6).all()), f"layer {layer}: err / scale per pass {(err / scale).tolist()}"


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_finished_decode_leaves_cache_and_logits_alone(monkeypatch, precision):
    run = 0
    bos = RUNS[run][0]
    text, prompt, _ = _inputs(run)
    # an EOS row that wins the first argmax: channel 0 of the final norm's output is lifted by 1000 (the normalised value itself is
    # below sqrt(1024) = 32 times its gain), the EOS row reads that channel alone and no other row reads it
    _, sd = _state_dict(bos)
    sd["ar_decoder.norm.bias"][0] += 1000.0
    sd["ar_predict_layer.weight"][:, 0] = 0.0
    sd["ar_predict_layer.weight"][1024].zero_()
    sd["ar_predict_layer.weight"][1024, 0] = 1000.0
    e = _engine(monkeypatch, precision, bos, True, sd)
    try:
        want, _ = _forced_decode(e, run, True)  # teacher forcing does not look at the EOS logit
        e.ar_prefill(text, prompt)
        pre = e.read_ar_kv()
        e.ar_decode(top_k=1)
        toks, reason, n_pass = e.ar_result()
        assert toks.numel() == 0 and n_pass == 1 and reason == 1, (toks, reason, n_pass)
        assert e.timings()["launches"] > 1, "no step was replayed behind the one that stopped"
        assert torch.equal(_bits(e.read_ar_kv()), _bits(pre)), "a finished decode wrote to the cache"
        got = e.read("ar_logits", (1, 1025))
    finally:
        e.close()
    # the one traced row is the prefill's, the same in both decodes
    assert torch.equal(_bits(got), _bits(want[:1])), "a finished decode rewrote the traced logits"
