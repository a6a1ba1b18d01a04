"""GPU: the CTC recogniser (asr_kernels.hpp and spk_kernels.hpp behind vx_asr_recognize, valle_amd.asr.SpeechRecognizer), the greedy
decode (vx_ctc_greedy) and the edit distance (vx_edit_distance) against the restatements of tests/asr_ref.py, which test_asr_cpu.py
pins against transformers' Wav2Vec2ForCTC / HubertForCTC, hand-worked cases and a full-matrix backtrace.

Yardstick: the restatement in fp64.  Floor: the same restatement in torch fp32 on the host.  Bound: engine max-abs error <=
4 x floor (asr_cases.TOL_FACTOR, the project's rule), per tap and per utterance: the output of conv layer 0, the features, every
hidden state, the logits; all three figures are printed before they are asserted and written to the file VX_ASR_PARITY_OUT names
(profiles/asr_parity.json comes from there).  The argmax equals fp64's on every frame whose fp64 top-two margin exceeds 2 x 4 x the
case's logits floor, at most 2 % of a case's frames are excused (test_asr_cpu.py asserts that of the inputs), and the token
sequence equals fp64's when no frame was.  That these inputs tell a wrong encoder order, a dropped norm, bias or affine and the tanh
GELU apart is checked without a GPU in test_asr_cpu.py.

1. both flavours at the tiny geometry (vocab 32 and 40: both tile paths of the head's GEMM; HuBERT's projection without its norm;
   head_dim 64) at 1 (the minimum), 2, 17, 33, 64, 65 and 130 frames; the base widths in the group flavour and the large widths in
   the layer flavour, two layers, at 16 and 49 frames;
2. vx_ctc_greedy on hand-made logits and vx_edit_distance on 64 seeded pairs, exactly;
3. a ragged batch (the lengths, shuffled) is bitwise every utterance alone, a second run is bitwise the first, nothing is written
   outside the outputs;
4. normalize=True; 24 kHz input through the resampler; the refusals; the error rates end to end; the codec round trip."""
import json
import os

import numpy as np
import pytest
import torch

import asr_cases as AC
import asr_ref as R

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
    out = os.environ.get("VX_ASR_PARITY_OUT")
    if out and _PARITY:
        with open(out, "w") as f:
            json.dump(_PARITY, f, indent=1, sort_keys=True)


def _rec(name):
    from valle_amd.asr import SpeechRecognizer

    if name not in _REC:
        wide = name in AC.WIDE
        _REC[name] = SpeechRecognizer(AC.config(name), AC.vocab(name), max_batch=2 if wide else 8, max_seconds=1.1 if wide else 2.7,
                                      state_dict=AC.state_dict(name), keep_taps=True).to(DEV)
    return _REC[name]


def _engine_taps(rec, frames, utt=0, samples=None):
    c = rec.config
    d, L = int(c.hidden_size), int(c.num_hidden_layers)
    taps = {"features": rec.read_tap("features", utt, frames, int(c.conv_dim[-1])),
            "logits": rec.read_tap("logits", utt, frames, int(c.vocab_size))}
    if samples is not None:
        t0 = (samples - int(c.conv_kernel[0])) // int(c.conv_stride[0]) + 1
        taps["conv0"] = rec.read_tap("conv0", utt, t0, int(c.conv_dim[0]))
    for l in range(L + 1):
        taps[f"hidden{l}"] = rec.read_tap(f"hidden{l}", utt, frames, d)
    return taps


def _check(name, frames, normalize=False):
    rec = _rec(name)
    wav = AC.wave(name, frames).to(DEV)
    hyp = rec.recognize(wav, sr=16000, normalize=normalize)[0]
    torch.cuda.synchronize()
    got = _engine_taps(rec, frames, samples=wav.numel())
    want = AC.named_taps(AC.reference(name, frames, torch.float64, normalize))
    floors = AC.floors(name, frames, normalize)
    assert sorted(got) == sorted(want)
    case = f"{name}_T{frames}" + ("_norm" if normalize else "")
    bad = []
    for tap in sorted(want):
        assert got[tap].shape == want[tap].shape, (tap, got[tap].shape, want[tap].shape)
        assert bool(torch.isfinite(got[tap]).all()), tap
        err, floor = float((got[tap].double() - want[tap]).abs().max()), floors[tap]
        ratio = err / floor if floor else float("inf")
        print(f"{case} {tap:10s}: engine {err:.3e}, floor {floor:.3e}, ratio {ratio:.2f}")
        _PARITY.setdefault(case, {})[tap] = {"engine": err, "floor": floor, "ratio": ratio}
        if not err <= AC.TOL_FACTOR * floor:
            bad.append((tap, err, floor))
    # the decode: the engine's own logits through the restatement are the engine's transcript; fp64's where the margins decide
    ids64, decided = AC.decided_frames(name, frames, normalize)
    excused = int((~decided).sum())
    print(f"{case}: {excused} of {frames} frames excused")
    _PARITY[case]["excused_share"] = excused / frames
    own = R.ctc_greedy(got["logits"].numpy(), rec.blank_id)
    assert hyp.tokens == own[0] and hyp.frames == own[1]
    lp_tol = 2.0 ** -22 * max(1.0, abs(own[2]))  # both start from the same fp32 logits and sum in fp64; the kernel rounds its mean to fp32 once
    assert abs(hyp.logprob - own[2]) <= lp_tol, (hyp.logprob, own[2])
    assert excused <= AC.EXCUSED_SHARE * frames
    assert torch.equal(got["logits"].argmax(1)[decided], ids64[decided]), f"{case}: an argmax differs from fp64's on a decided frame"
    if excused == 0:
        want_tok = R.ctc_greedy(want["logits"].numpy(), rec.blank_id)
        assert hyp.tokens == want_tok[0] and hyp.frames == want_tok[1]
    assert not bad, f"{case}: engine error above {AC.TOL_FACTOR} x floor: {bad}"


# ---- 1. parity per tap ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", AC.FRAMES)
@pytest.mark.parametrize("name", [n for n in AC.GEOMETRIES if n not in AC.WIDE])
def test_parity(name, frames):
    _check(name, frames)


@pytest.mark.parametrize("frames", AC.WIDE_FRAMES)
@pytest.mark.parametrize("name", AC.WIDE)
def test_parity_released_widths(name, frames):
    _check(name, frames)


@pytest.mark.parametrize("name", ("tiny_group", "tiny_layer"))
def test_parity_normalize(name):
    _check(name, 33, normalize=True)


# ---- 2. the decode and the distance on their own ---------------------------------------------------------------------------------
def _ctc_case():
    """Hand-made rows: (frames per utterance, logits (sum, V))."""
    g = np.random.default_rng(11)
    V = 7
    utts = []

    def rows(ids, hi=4.0):
        x = g.normal(0.0, 0.5, (len(ids), V))
        for t, i in enumerate(ids):
            x[t, i] += hi
        return x

    utts.append(rows([1, 1, 0, 1]))                    # A A _ A -> A A
    utts.append(rows([2, 2, 2, 3, 3, 0, 0, 3]))        # runs, a blank-separated repeat
    utts.append(rows([0, 0, 4, 5, 0, 0]))              # leading and trailing blanks
    utts.append(rows([0] * 9))                         # all blank
    utts.append(rows([6]))                             # one frame, a token
    utts.append(rows([0]))                             # one frame, blank
    ties = np.zeros((4, V))
    ties[0, [2, 5]] = 3.0                              # an exact tie -> 2
    ties[1, :] = 1.0                                   # every value equal -> 0 = blank
    ties[2, [1, 6]] = -2.0                             # the maximum 0 is shared by five columns -> 0
    ties[3, [6, 3]] = 7.5                              # -> 3
    utts.append(ties)
    for T in (1, 63, 64, 65, 1000):                    # straddle the wave, the workgroup and its chunk loop
        utts.append(rows(g.integers(0, 3, T).tolist(), hi=2.0))  # a small alphabet: long runs and many blanks
    utts.append(np.zeros((0, V)))                      # no frame at all
    return [len(u) for u in utts], np.concatenate(utts).astype(np.float32)


def test_ctc_greedy_equals_the_restatement():
    from valle_amd.asr import ctc_greedy

    frames, x = _ctc_case()
    ids, at, mean, flp = ctc_greedy(torch.from_numpy(x).to(DEV), frames, blank=0)
    x64 = torch.from_numpy(x).double()
    ref_lp = torch.log_softmax(x64, 1).max(1).values
    floor = float((torch.log_softmax(torch.from_numpy(x), 1).max(1).values.double() - ref_lp).abs().max())
    o = 0
    for u, T in enumerate(frames):
        w_ids, w_at, w_mean, w_lp = R.ctc_greedy(x[o:o + T], 0)
        assert ids[u] == w_ids and at[u] == w_at, u
        if T:
            err = float((flp[o:o + T].double() - torch.from_numpy(w_lp)).abs().max())
            print(f"utterance {u} ({T} frames): {len(w_ids)} tokens, log-probability error {err:.3e}, floor {floor:.3e}")
            assert err <= AC.TOL_FACTOR * floor and abs(float(mean[u]) - w_mean) <= AC.TOL_FACTOR * floor
        else:
            assert float(mean[u]) == 0.0
        o += T
    assert ids[0] == [1, 1] and at[0] == [0, 3] and ids[3] == [] and ids[6] == [2, 3] and at[6] == [0, 3]


def _edit_pairs():
    from valle_amd.asr import EDIT_MAX_LEN

    g = np.random.default_rng(7)
    lens = [(0, 0), (0, 5), (5, 0), (1, 1), (1, 0), (63, 64), (64, 64), (65, 63), (257, 255), (255, 257), (EDIT_MAX_LEN, EDIT_MAX_LEN),
            (EDIT_MAX_LEN, 1), (1, EDIT_MAX_LEN), (300, 0), (0, 300)]
    pairs = []
    for a, b in lens:
        k = int(g.integers(2, 4))
        pairs.append((g.integers(0, k, a).tolist(), g.integers(0, k, b).tolist()))
    same = g.integers(0, 3, 257).tolist()
    pairs.append((same, list(same)))                                   # identical
    pairs.append((g.integers(0, 3, 65).tolist(), g.integers(5, 8, 70).tolist()))  # disjoint alphabets
    pairs.append(([1] * 64, [1] * 65))
    while len(pairs) < 64:
        k = int(g.integers(1, 4))
        pairs.append((g.integers(0, k, int(g.integers(0, 90))).tolist(), g.integers(0, k, int(g.integers(0, 90))).tolist()))
    return pairs


def test_edit_distance_equals_the_restatement():
    from valle_amd.asr import EDIT_MAX_LEN, edit_distance
    from valle_amd.engine import VxError

    pairs = _edit_pairs()
    assert len(pairs) == 64
    got = edit_distance([p[0] for p in pairs], [p[1] for p in pairs], DEV).tolist()
    for (a, b), row in zip(pairs, got):
        assert tuple(row) == R.edit_distance_fast(a, b), (len(a), len(b), row)
    assert got[15] == [0, 0, 0, 0] and got[16] == [70, 65, 0, 5]
    with pytest.raises(VxError, match=f"up to {EDIT_MAX_LEN} tokens"):
        edit_distance([[0] * (EDIT_MAX_LEN + 1)], [[0]], DEV)


# ---- 3. bitwise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("tiny_group", "tiny_layer", "hd64_layer"))
def test_ragged_batch_is_bitwise_solo_and_repeatable(name):
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
    for a, b in zip(*runs):  # bits, so that the NaN sentinel compares equal to itself
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a second run differs"
    tok, frm, cnt, lp, lg = runs[0]
    o = 0
    for i, T in enumerate(order):
        k = int(cnt[i])
        assert torch.equal(lg[o:o + T], solo_logits[i].cpu()), f"utterance {i} ({T} frames) differs from its solo logits"
        assert tok[o:o + k].tolist() == solo[i].tokens and frm[o:o + k].tolist() == solo[i].frames
        assert float(lp[i]) == solo[i].logprob
        assert bool((tok[o + k:o + T] == -7).all()), "the rest of an utterance's token slots is left alone"
        o += T
    # the taps of an utterance inside the batch are its solo taps
    mid = _engine_taps(rec, order[3], utt=3, samples=wavs[3].numel())
    rec.recognize(wavs[3], sr=16000)
    alone = _engine_taps(rec, order[3], utt=0, samples=wavs[3].numel())
    for k in alone:
        assert torch.equal(mid[k], alone[k]), k


# ---- 4. behaviour -----------------------------------------------------------------------------------------------------------------
def test_24khz_input_goes_through_the_resampler():
    from valle_amd.codec import Resampler

    rec = _rec("tiny_layer")
    g = torch.Generator().manual_seed(24)
    wav24 = (0.3 * torch.randn(30000, generator=g)).to(DEV)
    via = rec.logits(wav24, sr=24000)[0]
    wav16 = Resampler(24000, 16000).to(DEV)(wav24).reshape(-1)
    assert wav16.numel() == 20000
    assert torch.equal(via, rec.logits(wav16, sr=16000)[0])
    both = rec.recognize([wav24, wav24[:27000]])  # the default rate is 24 kHz
    assert both[0] == rec.recognize(wav16, sr=16000)[0] and len(both) == 2


def test_refusals():
    from valle_amd.asr import RecognizerConfig, SpeechRecognizer
    from valle_amd.engine import VxError

    rec = _rec("tiny_layer")
    assert rec.min_samples == 400
    with pytest.raises(VxError, match="399 samples, the shortest served is 400"):
        rec.recognize(torch.zeros(399, device=DEV), sr=16000)
    out = rec.logits(torch.zeros(400, device=DEV), sr=16000)[0]  # a constant input: every variance is 0, eps keeps it finite
    assert out.shape == (1, 32) and bool(torch.isfinite(out).all())
    with pytest.raises(NotImplementedError, match="add_adapter"):
        SpeechRecognizer(RecognizerConfig(**dict(AC.GEOMETRIES["tiny_layer"], add_adapter=True)), AC.vocab("tiny_layer"))


def test_error_rates_end_to_end():
    from valle_amd.asr import char_error_rate, normalize_text, recognition_error, word_error_rate

    rec = _rec("tiny_group")
    wavs = [AC.wave("tiny_group", f).to(DEV) for f in (130, 65)]
    hyps = [t.text for t in rec.recognize(wavs, sr=16000)]
    texts = ["The cat sat, on the mat!", ""]
    got = recognition_error(texts, wavs, rec, sr=16000)
    rate, rows = R.error_rate([R.normalize_text(t).split() for t in texts], [R.normalize_text(h).split() for h in hyps])
    assert [(p.distance, p.substitutions, p.deletions, p.insertions, p.ref_len) for p in got.pairs] == rows
    assert got.rate == rate and np.isnan(got.pairs[1].rate) and got.pairs[0].rate == rows[0][0] / 6
    cer = recognition_error(texts[0], wavs[0], rec, sr=16000, unit="char")
    crate, crows = R.error_rate([list(R.normalize_text(texts[0]))], [list(R.normalize_text(hyps[0]))])
    assert cer.rate == crate and cer.pairs[0].distance == crows[0][0]
    # known texts: the numbers by hand
    w = word_error_rate(["the cat sat on the mat", "hello world", ""], ["the cat sit on mat", "hello, WORLD!", "uh"], DEV)
    assert [(p.substitutions, p.deletions, p.insertions, p.ref_len) for p in w.pairs] == [(1, 1, 0, 6), (0, 0, 0, 2), (0, 0, 1, 0)]
    assert w.rate == 3 / 8
    c = char_error_rate("abc", "abd", DEV)
    assert c.rate == 1 / 3 and normalize_text("abd") == "ABD"


def test_roundtrip_wer_is_the_hand_composed_chain():
    import encodec_enc_ref as E
    from valle_amd.asr import recognition_error
    from valle_amd.codec import CodecConfig, EncodecDecoder

    geo = E.FULL
    codec = EncodecDecoder(CodecConfig(hidden=geo.hidden, filters=geo.filters, codebook_size=geo.codebook_size,
                                       n_codebooks=geo.n_codebooks), max_frames=256, max_batch=2, encoder=True)
    codec.load_state_dict(E.make_enc_weights(geo, 3), strict=True)
    codec.to(DEV)
    rec = _rec("tiny_layer")
    wav = E.make_wave(24001, 8).to(DEV)  # 1 s at 24 kHz
    out = codec.decode(codec.encode(wav))
    want = recognition_error("a b c", out.reshape(-1), rec, sr=24000)
    got = codec.roundtrip_wer(wav, "a b c", rec)
    assert got == want and got.pairs[0].ref_len == 3
