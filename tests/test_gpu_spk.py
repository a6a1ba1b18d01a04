"""GPU: the speaker encoder (spk_kernels.hpp behind vx_spk_embed, valle_amd.spk.SpeakerEncoder) against the fp64 restatement of
tests/spk_ref.py, which test_spk_cpu.py pins against transformers' WavLMForXVector / Wav2Vec2ForXVector.

Yardstick: the restatement in fp64.  Floor: the same restatement in torch fp32 on the host.  Bound: engine max-abs error <=
4 x floor (spk_cases.TOL_FACTOR, the project's rule), per tap and per utterance: features, every hidden state, every gate, the layer
sum, the TDNN output, the pooled statistics, the embedding, the logits; all three figures are printed before they are asserted and
written to the file VX_SPK_PARITY_OUT names (profiles/spk_parity.json comes from there).  That these inputs tell a wrong gate, bias
direction, pooling, padding, weight norm, layer sum, GroupNorm, GELU or TDNN order apart is checked without a GPU in
test_spk_cpu.py::test_every_mutation_moves_the_output.

1. the tiny geometry in both attention modes and a head_dim-64 one at 16 (the minimum), 17, 31, 33, 63, 64, 65 and 130 frames: they
   straddle the GEMM's row tiles (64 and 128), the attention's query tile (128) and its key tile (32); the tiny geometry without the
   weighted layer sum at two lengths; the base widths (768 / 12 heads, conv 512, pos conv 128 / 16, buckets 320 / 800, two layers)
   at 16 and 49 frames;
2. a ragged batch (the lengths, shuffled) is bitwise every utterance alone, a second run is bitwise the first, nothing is written
   outside the outputs;
3. normalize=True; the similarity; 24 kHz input through the resampler; the refusal of a too short utterance; the codec round trip."""
import json
import os

import pytest
import torch

import spk_cases as SC
import spk_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_ENC, _PARITY = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    yield
    for e in _ENC.values():
        e.close()
    _ENC.clear()
    out = os.environ.get("VX_SPK_PARITY_OUT")
    if out and _PARITY:
        with open(out, "w") as f:
            json.dump(_PARITY, f, indent=1, sort_keys=True)


def _enc(name):
    from valle_amd.spk import SpeakerEncoder

    if name not in _ENC:
        base = name == "base2"
        _ENC[name] = SpeakerEncoder(SC.config(name), attention=SC.attention(name), max_batch=2 if base else 8,
                                    max_seconds=1.1 if base else 2.7, state_dict=SC.state_dict(name), keep_taps=True).to(DEV)
    return _ENC[name]


def _engine_taps(enc, name, frames, utt=0):
    """Every tap of utterance `utt` of the last call, under spk_cases.named_taps' names (embedding and logits excepted)."""
    c = enc.config
    d, H, L = int(c.hidden_size), int(c.num_attention_heads), int(c.num_hidden_layers)
    tp = frames - sum(int(dl) * (int(k) - 1) for k, dl in zip(c.tdnn_kernel, c.tdnn_dilation))
    taps = {"features": enc.read_tap("features", utt, frames, int(c.conv_dim[-1])),
            "layer_sum": enc.read_tap("layer_sum", utt, frames, d),
            "tdnn": enc.read_tap("tdnn", utt, tp, int(c.tdnn_dim[-1])),
            "pooled": enc.read_tap("pooled", utt, 1, 2 * int(c.tdnn_dim[-1])).reshape(-1)}
    for l in range(L + 1):
        taps[f"hidden{l}"] = enc.read_tap(f"hidden{l}", utt, frames, d)
    if SC.attention(name) == "wavlm":
        for l in range(L):
            taps[f"gate{l}"] = enc.read_tap(f"gate{l}", utt, frames, H)
    return taps


def _check(name, frames, normalize=False):
    enc = _enc(name)
    wav = SC.wave(name, frames).to(DEV)
    emb, logits = enc.embed(wav, sr=16000, normalize=normalize, return_logits=True)
    torch.cuda.synchronize()
    got = _engine_taps(enc, name, frames)
    got["embedding"], got["logits"] = emb[0].cpu(), logits[0].cpu()
    want = SC.named_taps(SC.reference(name, frames, torch.float64, normalize))
    floors = SC.floors(name, frames, normalize)
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
        if not err <= SC.TOL_FACTOR * floor:
            bad.append((tap, err, floor))
    assert not bad, f"{case}: engine error above {SC.TOL_FACTOR} x floor: {bad}"


# ---- 1. parity per tap ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", SC.FRAMES)
@pytest.mark.parametrize("name", ("tiny_wavlm", "tiny_plain", "hd64"))
def test_parity(name, frames):
    _check(name, frames)


@pytest.mark.parametrize("frames", (17, 65))
def test_parity_without_layer_sum(frames):
    _check("tiny_last", frames)


@pytest.mark.parametrize("frames", SC.BASE_FRAMES)
def test_parity_base_widths(frames):
    _check("base2", frames)


def test_parity_normalize():
    _check("tiny_wavlm", 33, normalize=True)


# ---- 2. bitwise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("tiny_wavlm", "hd64"))
def test_ragged_batch_is_bitwise_solo_and_repeatable(name):
    enc = _enc(name)
    order = (63, 16, 130, 33, 17, 65, 31, 64)
    wavs = [SC.wave(name, f).to(DEV) for f in order]
    solo = [enc.embed(w, sr=16000, return_logits=True) for w in wavs]
    n, xv = len(wavs), enc.embedding_dim
    runs = []
    for _ in range(2):
        emb = torch.full((n * xv + 1,), float("nan"), dtype=torch.float32, device=DEV)
        lg = torch.full((n * xv + 1,), float("nan"), dtype=torch.float32, device=DEV)
        enc._embed_raw([w.data_ptr() for w in wavs], [w.numel() for w in wavs], False, emb.data_ptr(), lg.data_ptr())
        torch.cuda.synchronize()
        assert bool(torch.isnan(emb[-1])) and bool(torch.isnan(lg[-1])), "a write outside an output"
        runs.append((emb[:-1].reshape(n, xv).clone(), lg[:-1].reshape(n, xv).clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "a second run differs"
    for i, (e, l) in enumerate(solo):
        assert torch.equal(runs[0][0][i], e[0]), f"utterance {i} ({order[i]} frames) differs from its solo embedding"
        assert torch.equal(runs[0][1][i], l[0]), f"utterance {i} ({order[i]} frames) differs from its solo logits"
    # the taps of an utterance inside the batch are its solo taps
    mid = _engine_taps(enc, name, order[3], utt=3)
    enc.embed(wavs[3], sr=16000)
    alone = _engine_taps(enc, name, order[3], utt=0)
    for k in alone:
        assert torch.equal(mid[k], alone[k]), k


# ---- 3. behaviour -----------------------------------------------------------------------------------------------------------------
def test_similarity():
    name = "tiny_wavlm"
    enc = _enc(name)
    fa, fb = 33, 64
    a, b = SC.wave(name, fa).to(DEV), SC.wave(name, fb).to(DEV)
    own = enc.similarity(a, a, sr=16000)
    assert own.shape == (1,) and abs(float(own[0]) - 1.0) <= 1e-6
    from valle_amd.spk import speaker_similarity

    got = float(speaker_similarity(a, b, encoder=enc, sr=16000))
    ea, eb = SC.reference(name, fa, torch.float64)["embedding"], SC.reference(name, fb, torch.float64)["embedding"]
    want = R.cosine(ea, eb)
    # |d cos| <= 2 (|da| / |a| + |db| / |b|) to first order, |d.|_2 <= sqrt(n) x the embeddings' bound; one fp32 rounding of the result
    n = ea.numel()
    tol = 2 * sum(SC.TOL_FACTOR * SC.floors(name, f)["embedding"] * n ** 0.5 / float(e.norm()) for f, e in ((fa, ea), (fb, eb))) + 2.0 ** -23
    print(f"similarity: engine {got:.8f}, restatement {want:.8f}, tolerance {tol:.2e}")
    assert abs(got - want) <= tol
    pair = enc.similarity([a, b], [b, a], sr=16000)
    assert torch.equal(pair[0], pair[1]) and float(pair[0]) == got


def test_24khz_input_goes_through_the_resampler():
    from valle_amd.codec import Resampler

    name = "tiny_wavlm"
    enc = _enc(name)
    g = torch.Generator().manual_seed(24)
    wav24 = (0.3 * torch.randn(30000, generator=g)).to(DEV)
    via = enc.embed(wav24, sr=24000)
    wav16 = Resampler(24000, 16000).to(DEV)(wav24).reshape(-1)
    assert wav16.numel() == 20000
    assert torch.equal(via, enc.embed(wav16, sr=16000))
    both = enc.embed([wav24, wav24[:27000]])  # the default rate is 24 kHz
    assert torch.equal(both[0], via[0])


def test_too_short_utterance_is_refused():
    from valle_amd.engine import VxError

    enc = _enc("tiny_wavlm")
    assert enc.min_samples == 5200
    with pytest.raises(VxError, match="5199 samples, the shortest served is 5200"):
        enc.embed(torch.zeros(5199, device=DEV), sr=16000)
    out = enc.embed(torch.zeros(5200, device=DEV), sr=16000)  # a constant input: GroupNorm's variance is 0, eps keeps it finite
    assert bool(torch.isfinite(out).all())


def test_roundtrip_speaker_similarity_is_the_hand_composed_chain():
    import encodec_enc_ref as E
    from valle_amd.codec import CodecConfig, EncodecDecoder

    geo = E.FULL
    codec = EncodecDecoder(CodecConfig(hidden=geo.hidden, filters=geo.filters, codebook_size=geo.codebook_size,
                                       n_codebooks=geo.n_codebooks), max_frames=256, max_batch=2, encoder=True)
    codec.load_state_dict(E.make_enc_weights(geo, 3), strict=True)
    codec.to(DEV)
    enc = _enc("tiny_wavlm")
    wav = E.make_wave(24001, 8).to(DEV)  # 1 s at 24 kHz: 16001 samples at 16 kHz
    rec = codec.decode(codec.encode(wav))
    want = enc.similarity(wav.reshape(-1), rec.reshape(-1), sr=24000)[0]
    got = codec.roundtrip_speaker_similarity(wav, enc)
    assert got.dim() == 0 and torch.equal(got, want) and bool(torch.isfinite(got)) and -1.0 - 1e-6 <= float(got) <= 1.0 + 1e-6
