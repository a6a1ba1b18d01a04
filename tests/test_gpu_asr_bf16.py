"""GPU: the CTC recogniser in the bf16 encoder mode (`SpeechRecognizer(..., precision="bf16")`, VX_ASR_ENC_BF16) against the
restatements: yardstick asr_ref in fp64, unrounded; floor enc_bf16_ref (the definition's roundings) in torch fp32 on the host against
that fp64; bound engine max-abs error <= 4 x floor per tap and per utterance (enc_bf16_cases).  The figures are printed before they
are asserted and written to the file VX_ENC_BF16_PARITY_OUT names, under "ctc".

1. every tap - conv0, features, every hidden<l>, the logits - on hd64_layer x asr_cases.FRAMES and large2 x WIDE_FRAMES; the argmax
   equals fp64's on every decided frame; the transcript is the restatement's decode of the engine's own logits; the taps ahead of
   the first layer are bitwise the fp32 handle's;
2. a ragged batch is bitwise every utterance alone, and a second run is bitwise the first;
3. align and recognition_error run on a bf16 handle; timings() reports the mode's smaller workspace and weights."""
import json
import os

import pytest
import torch

import asr_cases as AC
import asr_ref as R
import enc_bf16_cases as EC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_REC, _PARITY = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    yield
    for r in _REC.values():
        r.close()
    _REC.clear()
    out = os.environ.get("VX_ENC_BF16_PARITY_OUT")
    if out and _PARITY:
        prev = {}
        if os.path.isfile(out):
            with open(out) as f:
                prev = json.load(f)
        prev["ctc"] = _PARITY
        with open(out, "w") as f:
            json.dump(prev, f, indent=1, sort_keys=True)


def _rec(name, precision="bf16"):
    from valle_amd.asr import SpeechRecognizer

    if (name, precision) not in _REC:
        wide = name in AC.WIDE
        _REC[(name, precision)] = SpeechRecognizer(AC.config(name), AC.vocab(name), max_batch=2 if wide else 8, max_seconds=1.1 if wide else 2.7,
                                                   state_dict=AC.state_dict(name), keep_taps=True, precision=precision).to(DEV)
    return _REC[(name, precision)]


def _engine_taps(rec, frames, utt=0, samples=None):
    c = rec.config
    d, L = int(c.hidden_size), int(c.num_hidden_layers)
    taps = {"features": rec.read_tap("features", utt, frames, int(c.conv_dim[-1])), "logits": rec.read_tap("logits", utt, frames, int(c.vocab_size))}
    if samples is not None:
        t0 = (samples - int(c.conv_kernel[0])) // int(c.conv_stride[0]) + 1
        taps["conv0"] = rec.read_tap("conv0", utt, t0, int(c.conv_dim[0]))
    for l in range(L + 1):
        taps[f"hidden{l}"] = rec.read_tap(f"hidden{l}", utt, frames, d)
    return taps


# ---- 1. parity per tap ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frames", EC.ASR_CASES)
def test_parity_and_decided_frames(name, frames):
    rec = _rec(name)
    wav = AC.wave(name, frames).to(DEV)
    hyp = rec.recognize(wav, sr=16000)[0]
    torch.cuda.synchronize()
    got = _engine_taps(rec, frames, samples=wav.numel())
    want = AC.named_taps(AC.reference(name, frames, torch.float64))
    floors = EC.asr_floors(name, frames)
    assert sorted(got) == sorted(want)
    case = f"{name}_T{frames}"
    bad = []
    for tap in sorted(want):
        assert got[tap].shape == want[tap].shape, (tap, got[tap].shape, want[tap].shape)
        assert bool(torch.isfinite(got[tap]).all()), tap
        err, floor = float((got[tap].double() - want[tap]).abs().max()), floors[tap]
        ratio = err / floor if floor else float("inf")
        print(f"{case} {tap:10s}: engine {err:.3e}, floor {floor:.3e}, ratio {ratio:.2f}")
        _PARITY.setdefault(case, {})[tap] = {"engine": err, "floor": floor, "ratio": ratio}
        if not err <= EC.TOL_FACTOR * floor:
            bad.append((tap, err, floor))
    ids64, decided = EC.asr_decided_frames(name, frames)
    assert bool(decided.any())
    own = R.ctc_greedy(got["logits"].numpy(), rec.blank_id)  # the head and the decode are the fp32 mode's
    assert hyp.tokens == own[0] and hyp.frames == own[1]
    assert abs(hyp.logprob - own[2]) <= 2.0 ** -22 * max(1.0, abs(own[2])), (hyp.logprob, own[2])
    assert torch.equal(got["logits"].argmax(1)[decided], ids64[decided]), f"{case}: an argmax differs from fp64's on a decided frame"
    assert not bad, f"{case}: engine error above {EC.TOL_FACTOR} x floor: {bad}"


@pytest.mark.parametrize("name,frames", (("hd64_layer", 65), ("large2", 49)))
def test_ahead_of_the_layers_it_is_the_fp32_handle(name, frames):
    wav = AC.wave(name, frames).to(DEV)
    taps = {}
    for prec in ("fp32", "bf16"):
        rec = _rec(name, prec)
        rec.recognize(wav, sr=16000)
        taps[prec] = _engine_taps(rec, frames, samples=wav.numel())
    for tap in ("conv0", "features", "hidden0"):
        assert torch.equal(taps["fp32"][tap], taps["bf16"][tap]), tap
    assert not torch.equal(taps["fp32"]["hidden1"], taps["bf16"]["hidden1"]), "the mode runs"
    want, floors = AC.named_taps(AC.reference(name, frames, torch.float64)), AC.floors(name, frames)
    for tap in want:  # the fp32 handle of this build is still inside the fp32 bound
        assert float((taps["fp32"][tap].double() - want[tap]).abs().max()) <= AC.TOL_FACTOR * floors[tap], tap


# ---- 2. bitwise -------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_is_bitwise_solo_and_repeatable():
    name = "hd64_layer"
    rec = _rec(name)
    order = (64, 1, 130, 33, 17, 65, 2)
    wavs = [AC.wave(name, f).to(DEV) for f in order]
    solo_logits = [rec.logits(w, sr=16000)[0].clone() for w in wavs]
    solo = [rec.recognize(w, sr=16000)[0] for w in wavs]
    n, V, total = len(wavs), int(rec.config.vocab_size), sum(order)
    runs = []
    for _ in range(2):
        tok = torch.full((total + 1,), -7, dtype=torch.int32, device=DEV)
        frm = torch.full((total + 1,), -7, dtype=torch.int32, device=DEV)
        cnt = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
        lp = torch.full((n + 1,), float("nan"), dtype=torch.float32, device=DEV)
        lg = torch.full((total * V + 1,), float("nan"), dtype=torch.float32, device=DEV)
        rec._recognize_raw([w.data_ptr() for w in wavs], [w.numel() for w in wavs], False, tok.data_ptr(), frm.data_ptr(), cnt.data_ptr(),
                           lp.data_ptr(), lg.data_ptr())
        torch.cuda.synchronize()
        assert int(tok[-1]) == -7 and int(frm[-1]) == -7 and int(cnt[-1]) == -7 and bool(torch.isnan(lp[-1])) and bool(torch.isnan(lg[-1])), \
            "a write outside an output"
        runs.append((tok.cpu(), frm.cpu(), cnt.cpu(), lp.cpu(), lg[:-1].reshape(total, V).cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a second run differs"
    tok, frm, cnt, lp, lg = runs[0]
    o = 0
    for i, T in enumerate(order):
        k = int(cnt[i])
        assert torch.equal(lg[o:o + T], solo_logits[i].cpu()), f"utterance {i} ({T} frames) differs from its solo logits"
        assert tok[o:o + k].tolist() == solo[i].tokens and frm[o:o + k].tolist() == solo[i].frames
        assert float(lp[i]) == solo[i].logprob
        o += T
    mids = {u: _engine_taps(rec, order[u], utt=u, samples=wavs[u].numel()) for u in (2, 3)}  # the taps of an utterance inside the batch
    for u, mid in mids.items():
        rec.recognize(wavs[u], sr=16000)
        alone = _engine_taps(rec, order[u], utt=0, samples=wavs[u].numel())
        for k in alone:
            assert torch.equal(mid[k], alone[k]), (u, k)


# ---- 3. behaviour -----------------------------------------------------------------------------------------------------------------
def test_align_recognition_error_and_timings_on_a_bf16_handle():
    from valle_amd.asr import recognition_error, word_error_rate

    name = "hd64_layer"
    rec = _rec(name)
    wavs = [AC.wave(name, f).to(DEV) for f in (130, 65)]
    hyps = rec.recognize(wavs, sr=16000)
    texts = ["the cat sat", "a dog"]
    got = recognition_error(texts, wavs, rec, sr=16000)
    assert got == word_error_rate(texts, [h.text for h in hyps], DEV) and [p.ref_len for p in got.pairs] == [3, 2]
    al = rec.align(wavs, texts, sr=16000)
    assert len(al) == 2 and all(a.feasible for a in al) and all(a.nll == a.nll and a.nll < float("inf") for a in al)
    a32 = _rec(name, "fp32").align(wavs, texts, sr=16000)
    for a, b in zip(al, a32):  # the same text on nearly the same logits: the likelihoods are close, not equal
        assert abs(a.nll - b.nll) <= 0.05 * abs(b.nll) + 1.0, (a.nll, b.nll)
    w16, w32 = rec.workspace_bytes(), _rec(name, "fp32").workspace_bytes()
    print(f"workspace {w32} -> {w16} bytes")
    assert w16 < w32
