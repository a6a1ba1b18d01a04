"""GPU: the log-probabilities generation records on engines created with VX_FLAG_LOGPROBS, and best-of-N synthesis on top of them.

Every value is checked against the fp64 restatement of tests/logprob_ref.py on the engine's OWN logits row (the traced AR rows,
the NAR stage logits), at the token the pass is scored at.  Tolerance everywhere: the engine's worst error at most 4 x the floor,
the worst error of torch.log_softmax in fp32 on the host over the same rows (logprob_ref.check prints both and their ratio).
Sizes are the smallest at which the kernels can still go wrong: V = 1025 (not a multiple of 256: tail lanes), a dozen passes (the
prefill / step boundary and the stop rule), several slots with different lengths, a refilled slot."""
import pytest
import torch

import logprob_ref as lr

pytestmark = pytest.mark.gpu

BMAX = 64
VX_ERR_STATE, VX_ERR_UNSUPPORTED = 3, 5
_ENGINES = {}


def _engine(d=128, H=2, L=2, Q=1, vallf=False, wseed=0, zero_eos=True, precision="bf16", **kw):
    """(engine, cfg): one engine per configuration for the whole module (max_text 16, max_audio 64)."""
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.config import ModelConfig
    from valle_amd.engine import Engine
    from valle_amd.weights import synthetic_state_dict

    key = (d, H, L, Q, vallf, wseed, zero_eos, precision, tuple(sorted(kw.items())))
    if key not in _ENGINES:
        cfg = ModelConfig(model_name="VALL-F" if vallf else "VALL-E", decoder_dim=d, nhead=H, num_decoder_layers=L, prefix_mode=1,
                          num_quantizers=Q)
        e = Engine(cfg, precision, max_text=16, max_audio=64, **kw)
        e.load_state_dict(synthetic_state_dict(cfg, wseed, zero_eos=zero_eos))
        _ENGINES[key] = (e, cfg)
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e, _ in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _utt(i, S=None, P=None):
    from valle_amd.weights import synthetic_inputs

    S = 5 + i % 5 if S is None else S   # S in 5..9
    P = 3 + i % 4 if P is None else P   # P in 3..6
    x, xl, y = synthetic_inputs(S, P, 8, seed=20 + i)
    return x[0].contiguous(), y[0, :, 0].contiguous(), (x, xl, y)


# ---------------------------------------------------------------------------------------------- the kernel
def _kernel_rows():
    """64 rows of V = 1025 logits and their Exp(1) noise: random rows at three scales, and the special rows at 0..5."""
    g = torch.Generator().manual_seed(7)
    V = 1025
    lg = torch.randn(64, V, generator=g) * torch.tensor([0.5, 2.0, 8.0]).repeat(22)[:64, None]
    noise = torch.empty(64, V).exponential_(1, generator=g)
    ninf = float("-inf")
    lg[0, torch.randperm(V, generator=g)[:700]] = ninf       # -inf entries add 0
    lo = int(lg[1].argmin())
    noise[1, lo] = 1e-30                                     # the sampled token is the row's minimum (unfiltered settings)
    lg[2] = 1.25                                             # all equal: lp = -log(1025)
    lg[3] = torch.linspace(-100.0, 0.0, V)[torch.randperm(V, generator=g)]  # spread 100: a sum without the max underflows
    lg[4] += 80.0                                            # ... or overflows
    lg[5] -= 80.0
    return lg, noise


@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_sample_logprob_kernel(temperature):
    """vx_op_sample_logprob: token and argmax equal vx_op_sample_topp's on the same inputs (the LP instantiation samples as the
    plain one does), lp within the floor rule of the fp64 value on the raw row, under every filter setting."""
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.engine import op_sample_logprob, op_sample_topp

    lg, noise = _kernel_rows()
    dl, dn = lg.cuda(), noise.cuda()
    hit_min = False
    for top_k in (-100, 1, 10, 64):
        for top_p in (1.0, 0.9):
            toks, lps = [], []
            for r in range(lg.shape[0]):
                tok, am, lp = op_sample_logprob(dl[r], top_k, temperature, top_p, dn[r])
                assert (tok, am) == op_sample_topp(dl[r], top_k, temperature, top_p, dn[r]), (top_k, top_p, r)
                assert am == int(lg[r].argmax())
                toks.append(tok)
                lps.append(lp)
            toks = torch.tensor(toks)
            if top_k <= 0 and top_p == 1.0:
                hit_min = hit_min or toks[1] == int(lg[1].argmin())
            lr.check(torch.tensor(lps), lg, toks, f"kernel T={temperature} top_k={top_k} top_p={top_p}")
    assert hit_min  # the row built for it really scored its minimum


def test_sample_logprob_kernel_degenerate_rows():
    """A row of -inf only: the sampler's clamp picks a token inside the row and its log-probability is -inf, never NaN; a V below
    one pass of the block (V = 300) and the widest V (1088) index their tails correctly."""
    from valle_amd.engine import op_sample_logprob

    row = torch.full((1025,), float("-inf")).cuda()
    tok, am, lp = op_sample_logprob(row, -100, 1.0, 1.0, torch.ones(1025).cuda())
    assert 0 <= tok < 1025 and lp == float("-inf")
    g = torch.Generator().manual_seed(3)
    for V in (300, 1088):
        lg = torch.randn(8, V, generator=g) * 3.0
        nz = torch.empty(8, V).exponential_(1, generator=g)
        out = [op_sample_logprob(lg[r].cuda(), -100, 1.0, 1.0, nz[r].cuda()) for r in range(8)]
        lr.check(torch.tensor([o[2] for o in out]), lg, torch.tensor([o[0] for o in out]), f"kernel V={V}")


# ---------------------------------------------------------------------------------------------- decode paths, batch-1
def _decode_b1(e, i, **kw):
    text, prompt, _ = _utt(i)
    e.ar_prefill(text, prompt)
    e.ar_decode(max_new_tokens=kw.pop("max_new_tokens", 12), **kw)
    toks, reason, n_pass = e.ar_result()
    lp = e.ar_logprobs()
    rows = e.read("ar_logits", (n_pass, 1025))
    sampled = e.read("ar_sampled", (n_pass,), dtype=torch.int32)
    return toks, reason, n_pass, lp, rows, sampled


B1_CASES = {
    "bf16": dict(),
    "fp32": dict(precision="fp32"),
    "no_graph": dict(no_graph=True),
    "vallf": dict(vallf=True),
    "head_dim_4": dict(d=64, H=16),                  # the reference's own test geometry, plain kernels
    "sharded": dict(d=1024, H=16),                   # the XCD-sharded step (2 L + 2 launches per pass)
}
SAMPLING = [dict(seed=5), dict(seed=6, top_k=10, temperature=0.8), dict(seed=7, top_k=100, top_p=0.9)]


@pytest.mark.parametrize("name", list(B1_CASES))
def test_batch1_decode_paths(name):
    """lp[i] of every pass against fp64 on traced row i at the sampled token, unfiltered and under top-k / temperature / top-p
    (the value is the model's, on the raw row, whatever the filter)."""
    e, _ = _engine(trace_logits=True, logprobs=True, **B1_CASES[name])
    for j, kw in enumerate(SAMPLING):
        toks, reason, n_pass, lp, rows, sampled = _decode_b1(e, j, **kw)
        n = toks.numel()  # 12 and the token limit, unless an unfiltered draw hit EOS first (its logit is 0 in these weights)
        assert (reason == 4 and n == 12) or (reason in lr.EOS_STOPS and n < 12)
        assert n_pass == n + (reason in lr.EOS_STOPS) and lp.shape == (n_pass,) and n_pass > 4
        assert torch.equal(toks, sampled[:n].long())  # the appended token is the sampled one
        lr.check(lp, rows, lr.ar_targets(sampled, n, reason), f"{name} {kw}")
    if name == "sharded":
        assert e.timings()["step_kernels"] == 2 * 2 + 2


def test_forced_tokens_are_the_scored_tokens():
    e, _ = _engine(trace_logits=True, logprobs=True)
    forced = torch.tensor([3, 1000, 17, 512, 1023, 0, 77])
    toks, reason, n_pass, lp, rows, sampled = _decode_b1(e, 3, seed=9, forced=forced, max_new_tokens=-1)
    assert torch.equal(toks, forced) and reason == 4 and n_pass == 8 and lp.shape == (8,)
    assert not torch.equal(sampled[:7].long(), forced)  # the draw went elsewhere: scoring it would fail below
    t = lr.ar_targets(sampled, 7, reason, forced)
    assert torch.equal(t[:7], forced) and int(t[7]) == int(sampled[7])  # the closing pass has no forced token: the sample
    lr.check(lp, rows, t, "forced")


def test_eos_stop_scores_eos():
    """Weights with a live EOS row (seed 2) and an utterance whose greedy decode the fp32 CPU oracle ends on EOS after 8 tokens:
    the last pass is scored at 1024, len(lp) == n_tokens + 1, and the sum is -sum(nll_ar) of vx_score for the same codes."""
    from valle_amd.weights import synthetic_inputs

    e, _ = _engine(wseed=2, zero_eos=False, precision="fp32", trace_logits=True, logprobs=True)
    x, xl, y = synthetic_inputs(5, 5, 8, seed=10)
    text, prompt = x[0].contiguous(), y[0, :, 0].contiguous()
    e.ar_prefill(text, prompt)
    e.ar_decode(top_k=1, max_new_tokens=12)
    toks, reason, n_pass = e.ar_result()
    lp = e.ar_logprobs()
    assert reason in lr.EOS_STOPS and 0 < toks.numel() < 12
    assert lp.shape == (toks.numel() + 1,) and n_pass == toks.numel() + 1
    rows = e.read("ar_logits", (n_pass, 1025))
    sampled = e.read("ar_sampled", (n_pass,), dtype=torch.int32)
    t = lr.ar_targets(sampled, toks.numel(), reason)
    assert int(t[-1]) == 1024 and torch.equal(t[:-1], toks)
    lr.check(lp, rows, t, "eos")
    codes = torch.cat([prompt, toks]).reshape(-1, 1)
    nll = e.score(text, text, codes, prompt.numel(), nar=False)[0].cpu()
    # Not a floor bound: the two sides are two different fp32 passes over the same model (vx_score's row kernels, the decode step's
    # GEMVs), whose logits differ by summation order.  With logits within 1e-5 of each other (fp32 at |logit| < 4, d = 128) a row's
    # nll moves by at most 2e-5, the 9 rows' sum by 2e-4; 1e-3 leaves a factor 5 and is far below one mis-scored token (~7 nats).
    assert abs(float(lp.double().sum()) + float(nll.double().sum())) <= 1e-3


# ---------------------------------------------------------------------------------------------- slots
def _slot_check(e, slot, n_tokens, reason, lp, what, forced=None):
    stride = e.max_audio + 2
    n_pass = lp.numel()
    rows = e.read("batch_trace", (n_pass, 1025), offset_bytes=slot * stride * 1025 * 4)
    sampled = e.read("batch_sampled", (n_pass,), dtype=torch.int32, offset_bytes=slot * stride * 4)
    lr.check(lp, rows, lr.ar_targets(sampled, n_tokens, reason, forced), what)


def test_three_slots_of_different_lengths():
    """max_batch = 3, three utterances of different lengths prefilled in one pass; slot 1 is teacher-forced with 5 tokens and
    stops six passes before the others.  Driven on the Engine (batch_prefill_all / batch_decode / batch_logprobs), which is all
    VALLE.inference_batch does between its argument checks and the NAR stages, because only there can the slot's traced rows be
    read; test_python_surface_returns_logprobs ties inference_batch and inference_stream to this path bit for bit."""
    e, _ = _engine(trace_logits=True, logprobs=True, max_batch=3)
    utts = [_utt(i) for i in (0, 2, 4)]
    forced = torch.tensor([9, 8, 7, 1001, 5])
    e.batch_prefill_all([u[0] for u in utts], [u[1] for u in utts])
    e.batch_decode(3, seeds=[11, 12, 13], top_k=[-100, -100, 20], forced=[None, forced.cuda(), None], max_new_tokens=12)
    lens = []
    for b in range(3):
        lp = e.batch_logprobs(b)
        toks, reason = e.batch_result(b)
        lens.append(lp.numel())
        # a pass per token, and one more that closes the decode without appending: the EOS pass, or the pass behind the last forced token
        assert lp.numel() == toks.numel() + (reason in lr.EOS_STOPS or b == 1)
        assert torch.equal(e.batch_logprobs(b), lp)  # after vx_batch_decode a slot answers until it is prefilled again
        _slot_check(e, b, toks.numel(), reason, lp, f"3 slots, slot {b}", forced if b == 1 else None)
    assert lens[1] == 6 and lens[0] > 6 and lens[2] > 6  # 12 each unless an unfiltered draw hit EOS


def test_session_with_a_refilled_slot():
    """5 utterances through 3 slots (vx_batch_open / _admit / _run) with different token limits, so slots stop at different steps
    and two are refilled while the others decode.  A slot's values are read while it is STOPPED; after the vx_batch_result that
    vacates it the call is a state error.  This is VALLE.inference_stream's loop written out on the Engine: a slot's traced rows are
    overwritten when it is refilled, so they have to be read between the stop and the refill, which the generator does not expose;
    test_python_surface_returns_logprobs checks that inference_stream returns these values."""
    from valle_amd.engine import VxError

    e, _ = _engine(trace_logits=True, logprobs=True, max_batch=3)
    utts = [_utt(i) for i in range(5)]
    limit = [6, 12, 9, 4, 7]
    e.batch_open()
    live, nxt, seen = {}, 0, []
    for s in range(3):
        e.batch_admit([s], [utts[nxt][0]], [utts[nxt][1]], seeds=[30 + nxt], max_new_tokens=limit[nxt])
        live[s] = nxt
        nxt += 1
    while live:
        for s in e.batch_run(1):
            i = live.pop(s)
            lp = e.batch_logprobs(s)
            toks, reason = e.batch_result(s)  # vacates the slot; its trace and sample rows stay until it is admitted into again
            assert (reason == 4 and toks.numel() == limit[i]) or (reason in lr.EOS_STOPS and toks.numel() < limit[i])
            assert lp.numel() == toks.numel() + (reason in lr.EOS_STOPS)
            _slot_check(e, s, toks.numel(), reason, lp, f"session, utterance {i} in slot {s}")
            with pytest.raises(VxError) as err:
                e.batch_logprobs(s)
            assert err.value.code == VX_ERR_STATE
            seen.append((i, s))
            if nxt < 5:
                e.batch_admit([s], [utts[nxt][0]], [utts[nxt][1]], seeds=[30 + nxt], max_new_tokens=limit[nxt])
                live[s] = nxt
                nxt += 1
    assert sorted(i for i, _ in seen) == list(range(5))
    assert len({s for i, s in seen if i >= 3}) >= 1  # utterances 3 and 4 ran in refilled slots


def test_batch_invariance():
    """The same utterance and seed give bitwise the same values in slot 0 and in slot 2 of a 3-slot batch, and alone."""
    e, _ = _engine(trace_logits=True, logprobs=True, max_batch=3)
    u, other = _utt(1), [_utt(6), _utt(8)]

    def run(slots):  # slot -> utterance; per-slot prefill: the prefill of a slot does not depend on the others either
        for s, v in enumerate(slots):
            e.batch_prefill(s, v[0], v[1])
        e.batch_decode(len(slots), seeds=[77 if v is u else 80 + s for s, v in enumerate(slots)], max_new_tokens=12)
        k = [s for s, v in enumerate(slots) if v is u][0]
        lp = e.batch_logprobs(k)
        return lp, e.batch_result(k)[0]

    lp0, t0 = run([u, other[0], other[1]])
    lp2, t2 = run([other[1], other[0], u])
    lp1, t1 = run([u])
    assert torch.equal(t0, t2) and torch.equal(t0, t1)
    assert torch.equal(lp0.view(torch.int32), lp2.view(torch.int32)) and torch.equal(lp0.view(torch.int32), lp1.view(torch.int32))


# ---------------------------------------------------------------------------------------------- no behaviour change
@pytest.mark.parametrize("geom", [dict(), dict(d=1024, H=16)], ids=["five_launch", "sharded"])
def test_flag_off_is_unchanged_batch1(geom):
    """Same model, same seeds, flag on and off: the same tokens, stop reasons and launches per pass (5 L + 2 on the five-launch
    step, 2 L + 2 on the sharded one: 26 at the 12 layers of the README's figure); a flag-off engine answers UNSUPPORTED, a
    flag-on one STATE before its first decode."""
    from valle_amd.engine import VxError

    off, _ = _engine(**geom)
    on, _ = _engine(logprobs=True, **geom)
    text, prompt, _ = _utt(2)
    on.ar_prefill(text, prompt)
    with pytest.raises(VxError) as err:
        on.ar_logprobs()
    assert err.value.code == VX_ERR_STATE
    res = []
    for e in (off, on):
        out = []
        for kw in SAMPLING:
            e.ar_prefill(text, prompt)
            e.ar_decode(max_new_tokens=12, **kw)
            toks, reason, n_pass = e.ar_result()
            out.append((toks.tolist(), reason, n_pass))
        res.append((out, e.timings()["step_kernels"]))
    assert res[0] == res[1]
    assert res[0][1] == (2 * 2 + 2 if geom else 5 * 2 + 2)
    with pytest.raises(VxError) as err:
        off.ar_logprobs()
    assert err.value.code == VX_ERR_UNSUPPORTED
    assert on.ar_logprobs().shape == (res[1][0][-1][2],)


def test_flag_off_is_unchanged_three_slots():
    from valle_amd.engine import VxError

    off, _ = _engine(max_batch=3)
    on, _ = _engine(logprobs=True, max_batch=3)
    utts = [_utt(i) for i in (0, 2, 4)]
    res = []
    for e in (off, on):
        e.batch_prefill_all([u[0] for u in utts], [u[1] for u in utts])
        e.batch_decode(3, seeds=[11, 12, 13], top_k=[-100, 5, 20], top_p=[1.0, 1.0, 0.9], max_new_tokens=12)
        res.append([(t.tolist(), r) for t, r in (e.batch_result(b) for b in range(3))])
    assert res[0] == res[1]
    for fn in (lambda: off.batch_logprobs(0), lambda: off.nar_logprobs(0, 1)):
        with pytest.raises(VxError) as err:
            fn()
        assert err.value.code == VX_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- NAR
def _nar_inputs(i, T, Q=4):
    g = torch.Generator().manual_seed(50 + i)
    text = torch.randint(3, 100, (5 + i,), generator=g)
    prompts = torch.randint(0, 1024, (4 + i, Q), generator=g)
    toks = torch.randint(0, 1024, (T,), generator=g)
    return text, prompts, toks


def test_nar_logprobs():
    """Q = 4: every stage's value against fp64 on the stage's own logits rows at the code it reports; under forced_codes still
    the stage's own argmax; two utterances of different T in one batched call give bitwise what each gives alone."""
    from valle_amd.engine import VxError

    e, _ = _engine(Q=4, logprobs=True)
    with pytest.raises(VxError) as err:
        e.nar_logprobs(0, 13)
    assert err.value.code == VX_ERR_STATE  # no NAR call yet
    a, b = _nar_inputs(0, 13), _nar_inputs(1, 9)
    for forced in (None, torch.randint(0, 1024, (13, 4), generator=torch.Generator().manual_seed(1))):
        codes, lg = e.nar(*a, out_device="cpu", stage_logits=True, forced_codes=forced)
        lp = e.nar_logprobs(0, 13)
        assert lp.shape == (3, 13) and torch.equal(codes[:, 1:].t(), lg.argmax(2))
        lr.check(lp.reshape(-1), lg.reshape(-1, 1024), codes[:, 1:].t().reshape(-1), f"nar forced={forced is not None}")
    both = e.nar_batch([a[0], b[0]], [a[1], b[1]], [a[2], b[2]], out_device="cpu")
    lps = [e.nar_logprobs(0, 13), e.nar_logprobs(1, 9)]
    with pytest.raises(VxError) as err:
        e.nar_logprobs(2, 9)
    assert err.value.code == 1
    for z, u in enumerate((a, b)):
        alone = e.nar_batch([u[0]], [u[1]], [u[2]], out_device="cpu")[0]
        assert torch.equal(alone, both[z])
        assert torch.equal(e.nar_logprobs(0, u[2].numel()).view(torch.int32), lps[z].view(torch.int32)), z
    assert lps[0].shape == (3, 13) and lps[1].shape == (3, 9) and bool((lps[0] <= 0).all()) and bool((lps[1] <= 0).all())


# ---------------------------------------------------------------------------------------------- Python surface, best-of-N
def _model(max_batch, cls_name="VALLE", **kw):
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import models
    from valle_amd.config import ModelConfig
    from valle_amd.weights import synthetic_state_dict

    cfg = ModelConfig(model_name="VALL-F" if cls_name == "VALLF" else "VALL-E", decoder_dim=128, nhead=2, num_decoder_layers=2,
                      prefix_mode=1, num_quantizers=4)
    m = getattr(models, cls_name)(128, 2, 2, prefix_mode=1, num_quantizers=4, max_text=16, max_audio=192, print_eos=False,
                                  max_batch=max_batch, logprobs=True, **kw)
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    return m.to("cuda:0").eval()


def _cuda(u):
    return tuple(t.cuda() for t in u)


@pytest.mark.parametrize("n,max_batch", [(4, 4), (5, 2)])
def test_best_of_n(n, max_batch):
    """n candidates of one utterance (n = 5 on 2 slots: three groups): the winner is the argmax of ar_mean (lowest index on
    ties), its codes are inference_batch's for that seed bit for bit, and tokens[k] is the batch result for seed k."""
    from valle_amd.models import best_of_index

    m = _model(max_batch)
    x, xl, y = _cuda(_utt(0, S=5, P=4)[2])
    seeds = [101 + 7 * k for k in range(n)]
    codes, best = m.inference_best_of(x, xl, y, None, n, top_k=50, temperature=0.9, seeds=seeds)
    ref = m.inference_batch([(x, xl, y)] * n, top_k=50, temperature=0.9, seeds=seeds, return_logprobs=True)
    assert best.seeds == seeds and len(best.ar_mean) == n and len(best.tokens) == n
    assert best.index == best_of_index(best.ar_mean) == max(range(n), key=lambda k: (best.ar_mean[k], -k))
    assert len(set(best.ar_mean)) > 1  # the candidates differ: the choice means something
    for k in range(n):
        assert torch.equal(best.tokens[k], ref[k][0][0, :, 0].cpu())
        assert best.ar_mean[k] == ref[k][1].ar_mean
    assert torch.equal(codes, ref[best.index][0]) and codes.shape == (1, 81, 4)
    assert best.logprobs.nar.shape == (3, 81) and torch.equal(best.logprobs.nar, ref[best.index][1].nar)
    m._drop_engine()


def test_python_surface_returns_logprobs():
    """inference / inference_batch / inference_stream with return_logprobs=True: (codes, GenLogProbs) per utterance, the codes
    those of the same call without it; the stream's values are the static batch's (per-slot prefill on both sides)."""
    m = _model(3)
    us = [_cuda(_utt(i)[2]) for i in range(4)]
    seeds = [5, 6, 7, 8]
    torch.manual_seed(3)
    plain = m.inference(*us[0], None, top_k=20, max_new_tokens=9)
    torch.manual_seed(3)
    codes, g = m.inference(*us[0], None, top_k=20, max_new_tokens=9, return_logprobs=True)
    assert torch.equal(codes, plain) and g.ar.shape == (9,) and g.nar.shape == (3, 9) and (g.n_tokens, g.stop_reason) == (9, 4)
    assert g.ar_mean == pytest.approx(float(g.ar.double().mean())) and bool((g.nar <= 0).all()) and bool((g.ar < 0).all())
    plain = m.inference_batch(us, top_k=20, seeds=seeds, batched_prefill=False)
    batch = m.inference_batch(us, top_k=20, seeds=seeds, batched_prefill=False, return_logprobs=True)
    stream = dict(m.inference_stream(us, top_k=20, seeds=seeds, batched_admit=False, return_logprobs=True))
    assert sorted(stream) == [0, 1, 2, 3]
    for i, (c, g) in enumerate(batch):
        T = 16 * us[i][0].shape[1] + 1
        assert torch.equal(c, plain[i]) and c.shape == (1, T, 4)
        assert g.ar.shape == (T,) and g.nar.shape == (3, T) and (g.n_tokens, g.stop_reason) == (T, 3)
        sc, sg = stream[i]
        assert torch.equal(sc, c) and torch.equal(sg.ar.view(torch.int32), g.ar.view(torch.int32))
        assert (sg.n_tokens, sg.stop_reason) == (T, 3) and sg.nar.shape == (3, T)
    m._drop_engine()
