"""GPU: the Whisper recogniser (whisper_kernels.hpp and spk_kernels.hpp behind vx_wsp_recognize, valle_amd.whisper.WhisperRecognizer)
against the restatement of tests/whisper_ref.py, which test_whisper_cpu.py pins against transformers.

Yardstick: the restatement in fp64.  Floor: the same restatement in torch fp32 on the host.  Bound: engine max-abs error <=
4 x floor (whisper_cases.TOL_FACTOR, the project's rule), per tap and per utterance: log-mel, conv1, features, every encoder hidden
state, the encoder output and the teacher-forced logits; all three figures are printed before they are asserted and written to the
file VX_WSP_PARITY_OUT names (profiles/whisper_parity.json comes from there).  Greedy tokens, counts and stop reasons equal fp64's up
to the first undecided step (test_whisper_cpu.py asserts that the cases have none), and the reported log-probabilities equal the
restatement run on the engine's own logits within 2^-22 max(1, |v|).

1. parity per tap on every case of whisper_cases.CASES: audio of 1, 199, 200, 201, 319, 320, 321, chunk - 1 and chunk samples, prompts
   of 1, 2 and 4 tokens, a cache that passes 31 / 32 / 33 and 63 / 64 / 65 positions (geometry B), whisper-tiny's widths (C), two K
   chunks in fc2, 300 logits and 260 cross keys (D); on D also 260 teacher-forced tokens, which take the self cache across 256 keys;
2. greedy generation on the same cases;
3. a ragged batch (1, 3 and max_batch utterances, and 9 on a max_batch = 16 recogniser; shuffled lengths, different stop steps) is
   bitwise every utterance alone, a second run is bitwise the first, nothing is written outside the outputs;
4. 24 kHz input through the resampler, score_tokens, recognition_error end to end, the refusals."""
import json
import os

import pytest
import torch

import whisper_cases as WC
import whisper_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_BATCH = 8
_REC, _PARITY = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    yield
    for r in _REC.values():
        r.close()
    _REC.clear()
    out = os.environ.get("VX_WSP_PARITY_OUT")
    if out and _PARITY:
        with open(out, "w") as f:
            json.dump(_PARITY, f, indent=1, sort_keys=True)


def _rec(name, max_batch=MAX_BATCH):
    from valle_amd.whisper import WhisperRecognizer

    if (name, max_batch) not in _REC:
        _REC[(name, max_batch)] = WhisperRecognizer(WC.config(name), WC.vocab(name), WC.generation(name), max_batch=max_batch,
                                                    state_dict=WC.state_dict(name), keep_taps=True).to(DEV)
    return _REC[(name, max_batch)]


def _engine_taps(rec, name, utt, count):
    g = WC.GEOMETRIES[name]
    P, d = g["max_source_positions"], g["d_model"]
    taps = {"logmel": rec.read_tap("logmel", utt, 2 * P, g["num_mel_bins"]), "conv1": rec.read_tap("conv1", utt, 2 * P, d),
            "features": rec.read_tap("features", utt, P, d), "encoder": rec.read_tap("encoder", utt, P, d),
            "logits": rec.read_tap("logits", utt, count, g["vocab_size"])}
    for l in range(g["encoder_layers"] + 1):
        taps[f"enc{l}"] = rec.read_tap(f"enc{l}", utt, P, d)
    return taps


# ---- 1. parity per tap ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(WC.CASES))
def test_parity(cid):
    name = WC.CASES[cid][0]
    rec = _rec(name)
    want_gen = WC.generated(cid)
    wav = WC.case_wave(cid).to(DEV)
    sc = rec.score_tokens([wav], [want_gen["tokens"]], sr=16000, prompt_ids=WC.case_prompt(cid))
    got = _engine_taps(rec, name, 0, len(want_gen["tokens"]))
    want, floors = WC.named_taps(cid, torch.float64), WC.floors(cid)
    assert sorted(got) == sorted(want)
    bad = []
    for tap in sorted(want):
        assert got[tap].shape == want[tap].shape, (tap, got[tap].shape, want[tap].shape)
        assert bool(torch.isfinite(got[tap]).all()), tap
        err, floor = float((got[tap].double() - want[tap]).abs().max()), floors[tap]
        ratio = err / floor if floor else float("inf")
        print(f"{cid} {tap:10s}: engine {err:.3e}, floor {floor:.3e}, ratio {ratio:.2f}")
        _PARITY.setdefault(cid, {})[tap] = {"engine": err, "floor": floor, "ratio": ratio}
        if not err <= WC.TOL_FACTOR * floor:
            bad.append((tap, err, floor))
    # the forced log-probabilities: the restatement on the engine's own logits
    g = WC.generation(name)
    own = R.forced_logprobs(got["logits"], want_gen["tokens"], g["suppress_tokens"], g["begin_suppress_tokens"])
    for a, b in zip(sc.token_logprobs[0], own):
        assert abs(a - b) <= 2.0 ** -22 * max(1.0, abs(b)), (a, b)
    assert abs(sc.nll[0] + sum(sc.token_logprobs[0])) <= 1e-9
    assert not bad, f"{cid}: engine error above {WC.TOL_FACTOR} x floor: {bad}"


def test_teacher_forced_across_256_self_keys():
    """Geometry D, 260 forced tokens after a 4-token prompt: the self-attention cache passes 255 / 256 / 257 keys (a thread's second
    key, quarters of more than 64 keys), every step's cross-attention reads 260 keys, fc2 sums two K chunks, the head reads 300 logits."""
    name = WC.TF_CASE[0]
    rec = _rec(name)
    tokens = WC.tf_tokens()
    g = WC.generation(name)
    assert len(WC.tf_prompt()) + len(tokens) == WC.GEOMETRIES[name]["max_target_positions"] and len(tokens) == 260
    assert not set(tokens) & (set(g["suppress_tokens"]) | set(g["begin_suppress_tokens"]) | {WC.special(name)["eos"]})
    sc = rec.score_tokens([WC.tf_wave().to(DEV)], [tokens], sr=16000, prompt_ids=WC.tf_prompt())
    got = _engine_taps(rec, name, 0, len(tokens))
    want, floors = WC.tf_taps(torch.float64), WC.tf_floors()
    assert sorted(got) == sorted(want)
    bad = []
    for tap in sorted(want):
        assert got[tap].shape == want[tap].shape, (tap, got[tap].shape, want[tap].shape)
        assert bool(torch.isfinite(got[tap]).all()), tap
        err, floor = float((got[tap].double() - want[tap]).abs().max()), floors[tap]
        ratio = err / floor if floor else float("inf")
        print(f"D_tf260 {tap:10s}: engine {err:.3e}, floor {floor:.3e}, ratio {ratio:.2f}")
        _PARITY.setdefault("D_tf260", {})[tap] = {"engine": err, "floor": floor, "ratio": ratio}
        if not err <= WC.TOL_FACTOR * floor:
            bad.append((tap, err, floor))
    own = R.forced_logprobs(got["logits"], tokens, g["suppress_tokens"], g["begin_suppress_tokens"])
    assert len(sc.token_logprobs[0]) == len(own) == 260
    for a, b in zip(sc.token_logprobs[0], own):
        assert abs(a - b) <= 2.0 ** -22 * max(1.0, abs(b)), (a, b)
    assert not bad, f"engine error above {WC.TOL_FACTOR} x floor: {bad}"


# ---- 2. greedy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(WC.CASES))
def test_greedy_tokens_equal_fp64(cid):
    name, _, _, _, mn = WC.CASES[cid]
    rec = _rec(name)
    want = WC.generated(cid)
    hyp = rec.recognize([WC.case_wave(cid).to(DEV)], sr=16000, prompt_ids=WC.case_prompt(cid), max_new_tokens=mn)[0]
    dec = WC.decided(cid)
    upto = dec.index(False) if False in dec else len(dec)
    print(f"{cid}: {len(want['tokens'])} tokens, stop {want['stop']}, first undecided step {upto if upto < len(dec) else None}")
    assert hyp.tokens[:upto] == want["tokens"][:upto]
    if upto == len(dec):
        from valle_amd.whisper import STOP_REASONS

        assert hyp.tokens == want["tokens"] and hyp.stop_reason == STOP_REASONS[want["stop"]]
    g = WC.generation(name)
    raw = rec.read_tap("logits", 0, len(hyp.tokens), WC.GEOMETRIES[name]["vocab_size"])
    for step, (tok, lp) in enumerate(zip(hyp.tokens, hyp.token_logprobs)):
        t, v, _ = R.step_outputs(raw[step], step, g["suppress_tokens"], g["begin_suppress_tokens"])
        assert t == tok and abs(lp - v) <= 2.0 ** -22 * max(1.0, abs(v)), (step, tok, t, lp, v)
    assert abs(hyp.logprob - sum(hyp.token_logprobs)) <= 1e-9


# ---- 3. bitwise --------------------------------------------------------------------------------------------------------------------
def _raw_call(rec, wavs, prompts, max_new, stride):
    n = len(wavs)
    tok = torch.full((n * stride + 1,), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((n * stride + 1,), float("nan"), dtype=torch.float32, device=DEV)
    cnt = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    stop = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    rec._recognize_raw([w.data_ptr() for w in wavs], [w.numel() for w in wavs], prompts, max_new, None, stride, tok.data_ptr(), lp.data_ptr(),
                       cnt.data_ptr(), stop.data_ptr())
    torch.cuda.synchronize()
    assert int(tok[-1]) == -7 and bool(torch.isnan(lp[-1])) and int(cnt[-1]) == -7 and int(stop[-1]) == -7, "a write outside an output"
    return tok[:-1].reshape(n, stride).cpu(), lp[:-1].reshape(n, stride).cpu(), cnt[:-1].cpu(), stop[:-1].cpu()


@pytest.mark.parametrize("name,cids", (
    ("A", ("A_len16000",)),
    ("A", ("A_prompt1", "A_len1", "A_cap3")),
    ("A", ("A_len320", "A_prompt2", "A_len15999", "A_cap3", "A_len1", "A_prompt1", "A_len201", "A_len16000")),
    ("B", ("B_2", "B_0", "B_3", "B_1", "B_0", "B_1", "B_2", "B_3")),
    # nine utterances on a max_batch = 16 recogniser: a second, ragged row tile of the token loop's GEMM
    ("D", ("D_1", "D_0", "D_0", "D_1", "D_0", "D_1", "D_1", "D_0", "D_1")),
    ("B", ("B_2", "B_0", "B_3", "B_1", "B_0", "B_1", "B_2", "B_3", "B_0")),
))
def test_ragged_batch_is_bitwise_solo_and_repeatable(name, cids):
    rec = _rec(name, MAX_BATCH if len(cids) <= MAX_BATCH else 16)
    Tt, V = WC.GEOMETRIES[name]["max_target_positions"], WC.GEOMETRIES[name]["vocab_size"]
    wavs = [WC.case_wave(c).to(DEV) for c in cids]
    prompts = [WC.case_prompt(c) for c in cids]
    max_new = [min(WC.case_max_new(c), Tt) for c in cids]
    runs = [_raw_call(rec, wavs, prompts, max_new, Tt) for _ in range(2)]
    for a, b in zip(*runs):  # bits, so that the NaN sentinel compares equal to itself
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a second run differs"
    tok, lp, cnt, stop = runs[0]
    pick = len(cids) // 2
    mid = _engine_taps(rec, name, pick, int(cnt[pick]))
    assert len(set(int(c) for c in cnt)) > 1 or len(cids) == 1, "the utterances stop at different steps"
    for i in range(len(cids)):
        st, sl, sc, ss = _raw_call(rec, [wavs[i]], [prompts[i]], [max_new[i]], Tt)
        k = int(cnt[i])
        assert int(sc[0]) == k and int(ss[0]) == int(stop[i]), (i, int(sc[0]), k)
        assert torch.equal(st[0, :k], tok[i, :k]) and torch.equal(sl[0, :k].view(torch.int32), lp[i, :k].view(torch.int32)), f"utterance {i} differs from solo"
        assert bool((tok[i, k:] == -7).all()) and bool(torch.isnan(lp[i, k:]).all()), "the rest of an utterance's slots is left alone"
        if i == pick:
            alone = _engine_taps(rec, name, 0, k)
            for tap in alone:
                assert torch.equal(mid[tap], alone[tap]), tap


# ---- 4. behaviour ------------------------------------------------------------------------------------------------------------------
def test_24khz_input_goes_through_the_resampler():
    from valle_amd.codec import Resampler

    rec = _rec("A")
    g = torch.Generator().manual_seed(24)
    wav24 = (0.3 * torch.randn(21000, generator=g)).to(DEV)
    via = rec.recognize(wav24)[0]  # the default rate is 24 kHz, the default prefix is [start, en, transcribe, notimestamps]
    wav16 = Resampler(24000, 16000).to(DEV)(wav24).reshape(-1)
    assert wav16.numel() == 14000
    assert via == rec.recognize(wav16, sr=16000, prompt_ids=WC.prompt("A", 4))[0]


def test_score_tokens_reproduces_the_greedy_logprobs():
    rec = _rec("B")
    wavs = [WC.case_wave(c).to(DEV) for c in ("B_0", "B_1")]
    hyps = rec.recognize(wavs, sr=16000)
    sc = rec.score_tokens(wavs, [h.tokens for h in hyps], sr=16000)
    for h, lps, nll in zip(hyps, sc.token_logprobs, sc.nll):
        assert lps == h.token_logprobs and nll == -h.logprob
    assert sc.mean == sum(sc.nll) / sum(len(h.tokens) for h in hyps)


def test_recognition_error_end_to_end():
    from valle_amd.asr import recognition_error, word_error_rate

    rec = _rec("A")
    wavs = [WC.case_wave(c).to(DEV) for c in ("A_prompt1", "A_len16000")]
    hyps = rec.recognize(wavs, sr=16000)
    inv = {i: t for t, i in WC.vocab("A").items()}
    from valle_amd.whisper import decode_tokens

    for h in hyps:
        assert h.text == decode_tokens(h.tokens, inv, WC.special("A")["eos"]) and h.text != ""
    texts = ["the cat sat on the mat", "a dog"]
    got = recognition_error(texts, wavs, rec, sr=16000)
    want = word_error_rate(texts, [h.text for h in hyps], DEV)
    assert got == want and [p.ref_len for p in got.pairs] == [6, 2]


def test_refusals():
    from valle_amd.engine import VxError

    rec = _rec("A")
    ch = WC.chunk("A")
    with pytest.raises(VxError, match=f"n_samples = {ch + 1} > the chunk of {ch} samples") as ei:
        rec.recognize(torch.zeros(ch + 1, device=DEV), sr=16000)
    assert ei.value.code == 4
    with pytest.raises(ValueError, match="prompt_ids"):
        rec.recognize(torch.zeros(100, device=DEV), sr=16000, prompt_ids=[])
    with pytest.raises(ValueError, match="max_target_positions"):
        rec.recognize(torch.zeros(100, device=DEV), sr=16000, prompt_ids=[0] * 40)
    out = rec.recognize(torch.zeros(1, device=DEV), sr=16000, max_new_tokens=2)[0]  # silence: every power is 0, the log-mel is flat
    assert len(out.tokens) == 2 and all(map(lambda v: v == v and v > float("-inf"), out.token_logprobs))
