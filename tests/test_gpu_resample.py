"""GPU: the sample-rate converter (codec_resample behind vx_resample, valle_amd.Resampler) against the fp64 definition of
tests/resample_ref.py.

* parity: orig in {8000 .. 48000} -> 24000 and 24000 -> {16000, 44100, 48000}, L in {1, 7, 4801, 3 s}, 1 and 2 channels, on
  unit-variance noise, outputs pre-filled with NaN.  Yardstick: the direct definition in fp64.  Floor: torchaudio's polyphase
  form run in torch fp32 on the host (mean, kernel rounded once, conv1d).  Bound: engine error <= 4 x floor
  (resample_ref.TOL_FACTOR, the rule of the codec's tests); every ratio is printed before it is asserted;
* orig == new returns the channel mean bit for bit;
* a ragged batch of mixed lengths and channel counts: every utterance bitwise its solo result, two calls bitwise equal;
* no dependence on memory the call does not own (NaN around the inputs, VX_POISON on the handle's own allocations), in fresh
  child processes;
* composition with the codec: encode(..., sr=), decode(..., sr=), tokenize_audio on a WAV file."""
import json
import os
import subprocess
import sys

import pytest
import torch

import encodec_enc_ref as E
import resample_ref as RR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAIRS = [(r, 24000) for r in RR.RATES_IN] + [(24000, r) for r in RR.RATES_OUT]


def _build():
    import __graft_entry__ as ge

    ge.build()


_RS = {}


def _resampler(orig, new, max_batch=8):
    _build()
    from valle_amd.codec import Resampler

    key = (orig, new, max_batch)
    if key not in _RS:
        _RS[key] = Resampler(orig, new, max_batch).to(DEV)
    return _RS[key]


def _run_nan_prefilled(rs, x):
    """One utterance through vx_resample into an output that holds NaN before the call."""
    x = x.reshape(-1, x.shape[-1]).to(DEV).contiguous()
    out = torch.full((rs.output_length(x.shape[1]),), float("nan"), device=DEV)
    rs._resample_raw([x.data_ptr()], [x.shape[0]], [x.shape[1]], [out.data_ptr()])
    return out


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_parity_with_fp64(pair):
    orig, new = pair
    rs = _resampler(orig, new)
    failures = []
    for L in (1, 7, 4801, 3 * orig):
        for ch in (1, 2):
            x = RR.make_noise(L, 7 * L + ch, channels=ch)
            ref64 = torch.from_numpy(RR.resample_direct(x, orig, new))
            ref32 = RR.resample_polyphase(x, orig, new, torch.float32)
            got = _run_nan_prefilled(rs, x)
            assert got.shape == ref64.shape == ref32.shape == (RR.out_length(orig, new, L),)
            assert not torch.isnan(got).any(), f"L={L} C={ch}: NaN sentinel left in the output"
            floor = float((ref32.double() - ref64).abs().max())
            err = float((got.double().cpu() - ref64).abs().max())
            print(f"resample {orig} -> {new} L={L} C={ch}: scale {float(ref64.abs().max()):.3g} floor {floor:.3e} engine {err:.3e} "
                  f"ratio {err / max(floor, 1e-300):.2f}")
            if err > RR.tolerance(floor):
                failures.append(f"L={L} C={ch}: engine {err:.3e} > {RR.TOL_FACTOR} x floor {floor:.3e}")
    assert not failures, failures


@pytest.mark.parametrize("pair", [(44101, 24000), (192000, 8000)], ids=lambda p: f"{p[0]}to{p[1]}")
def test_parity_of_the_large_table_and_the_short_tile(pair):
    """44101 -> 24000 has 24000 phases: the table (24000 x 23) is read from memory instead of LDS.  192000 -> 8000 has 291 taps
    per output: a workgroup owns fewer than 256 outputs so that their input span fits the staged window.  Same yardstick, floor
    and bound as above."""
    orig, new = pair
    rs = _resampler(orig, new)
    for L, ch in ((4801, 1), (4801, 2), (40000, 2)):
        x = RR.make_noise(L, 3 * L + ch, channels=ch)
        ref64 = torch.from_numpy(RR.resample_direct(x, orig, new))
        ref32 = RR.resample_polyphase(x, orig, new, torch.float32)
        got = _run_nan_prefilled(rs, x)
        assert got.shape == ref64.shape == (RR.out_length(orig, new, L),)
        assert not torch.isnan(got).any(), f"L={L} C={ch}: NaN sentinel left in the output"
        floor = float((ref32.double() - ref64).abs().max())
        err = float((got.double().cpu() - ref64).abs().max())
        print(f"resample {orig} -> {new} L={L} C={ch}: floor {floor:.3e} engine {err:.3e} ratio {err / max(floor, 1e-300):.2f}")
        assert err <= RR.tolerance(floor), f"L={L} C={ch}: engine {err:.3e} > {RR.TOL_FACTOR} x floor {floor:.3e}"
    batch = rs.resample_batch([x, x[:1, :777]])
    assert torch.equal(batch[0][0, 0], got) and torch.equal(batch[1], rs(x[:1, :777]))


def test_same_rate_is_the_mixed_down_input_bit_for_bit():
    rs = _resampler(24000, 24000)
    x = RR.make_noise(4801, 2, channels=2)
    assert torch.equal(_run_nan_prefilled(rs, x).cpu().view(torch.int32), x.mean(0).view(torch.int32))
    # the sign of a zero too: the mean as the header states it, (x0 + x1) / 2 in fp32 (torch.mean starts its sum at +0 and returns
    # +0 for two -0 samples), and a mono input unchanged
    x[0, 5], x[1, 5], x[0, 6], x[1, 6] = -0.0, -0.0, 0.0, -0.0
    assert torch.equal(_run_nan_prefilled(rs, x).cpu().view(torch.int32), ((x[0] + x[1]) / 2).view(torch.int32))
    assert torch.equal(_run_nan_prefilled(rs, x[0]).cpu().view(torch.int32), x[0].view(torch.int32))
    assert rs(x).shape == (1, 1, 4801)


@pytest.mark.parametrize("pair", [(44100, 24000), (48000, 24000), (11025, 24000), (24000, 44100)], ids=lambda p: f"{p[0]}to{p[1]}")
def test_ragged_batch_equals_alone_and_repeats_bitwise(pair):
    """Mixed lengths and channel counts in one call, among them one sample, a length below the filter's width and rows that start
    at every alignment of the 16-byte loads."""
    orig, new = pair
    rs = _resampler(orig, new)
    shapes = [(1, 1), (2, 7), (1, 4801), (2, 3 * orig + 1), (3, 1002), (2, 4803), (1, 255), (2, 1)]
    wavs = [RR.make_noise(L, 50 + i, channels=ch) for i, (ch, L) in enumerate(shapes)]
    together = [t.clone() for t in rs.resample_batch(wavs)]
    again = rs.resample_batch(wavs)
    for i, w in enumerate(wavs):
        alone = rs(w)
        assert together[i].shape == alone.shape == (1, 1, RR.out_length(orig, new, w.shape[1]))
        assert torch.equal(together[i], alone), f"utterance {i} {tuple(w.shape)} differs between the ragged batch and alone"
        assert torch.equal(together[i], again[i]), f"utterance {i}: two identical calls differ"
    ref = torch.from_numpy(RR.resample_direct(wavs[4], orig, new))  # three channels: against fp64
    floor = float((RR.resample_polyphase(wavs[4], orig, new, torch.float32).double() - ref).abs().max())
    err = float((together[4][0, 0].double().cpu() - ref).abs().max())
    print(f"ragged {orig} -> {new}, 3 channels: floor {floor:.3e} engine {err:.3e} ratio {err / floor:.2f}")
    assert err <= RR.tolerance(floor)


def test_follows_the_callers_stream():
    rs = _resampler(48000, 24000)
    x = RR.make_noise(48000, 4, channels=2).to(DEV)
    want = rs(x).cpu()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        junk = torch.randn(4096, 4096, device=DEV) @ torch.randn(4096, 4096, device=DEV)
        x2 = x * 1.0  # produced on the side stream right before the call reads it
        host = rs(x2).to("cpu")
    side.synchronize()
    assert torch.equal(host, want) and torch.isfinite(junk).all()


def test_output_does_not_depend_on_memory_it_does_not_own():
    """The inputs sit inside a larger buffer (at an odd offset, so that the aligned 16-byte loads would reach over both ends of
    every row) and the outputs inside another; what surrounds them is zero in one run and NaN in the other, and VX_POISON=1 fills
    the handle's own fresh allocations with 0xFF bytes.  The outputs must be bitwise the same and finite, and the surroundings
    of the outputs untouched."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = (
        "import sys, json, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import os, resample_ref as RR\n"
        "from valle_amd.codec import Resampler\n"
        "fill = float('nan') if os.environ['VX_GUARD'] == 'nan' else 0.0\n"
        "res = []\n"
        "for orig, new in ((44100, 24000), (24000, 48000), (11025, 24000)):\n"
        "    rs = Resampler(orig, new, 4).to('cuda:0')\n"
        "    shapes, ins, outs, bufs = [(2, 1001), (1, 7), (2, 4801)], [], [], []\n"
        "    for i, (ch, L) in enumerate(shapes):\n"
        "        b = torch.full((ch * L + 40,), fill, device='cuda:0')\n"
        "        b[13:13 + ch * L] = RR.make_noise(L, i, channels=ch).reshape(-1).to('cuda:0')\n"
        "        o = torch.full((rs.output_length(L) + 40,), fill, device='cuda:0')\n"
        "        bufs.append((b, o)); ins.append(b.data_ptr() + 52); outs.append(o.data_ptr() + 52)\n"
        "    rs._resample_raw(ins, [s[0] for s in shapes], [s[1] for s in shapes], outs)\n"
        "    torch.cuda.synchronize()\n"
        "    for (ch, L), (b, o) in zip(shapes, bufs):\n"
        "        n = rs.output_length(L)\n"
        "        edge = torch.cat([o[:13], o[13 + n:]])\n"
        "        assert bool(torch.isnan(edge).all()) if fill != fill else bool((edge == 0).all()), 'written outside the output'\n"
        "        assert bool(torch.isfinite(o[13:13 + n]).all()), 'non-finite output'\n"
        "        res.append(o[13:13 + n].cpu().view(torch.int32).tolist())\n"
        "print(json.dumps(res))\n"
        % (root, os.path.join(root, "tests")))
    outs = []
    for poison, guard in (("0", "zero"), ("1", "nan")):
        env = dict(os.environ, VX_POISON=poison, VX_GUARD=guard)
        r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]
    assert len(outs[0]) == 9 and all(len(o) > 0 for o in outs[0])


# ---- composition with the codec ----------------------------------------------------------------------------------------------
_ENC = {}


def _codec():
    _build()
    from valle_amd.codec import CodecConfig, EncodecDecoder

    if "d" not in _ENC:
        geo = E.FULL
        d = EncodecDecoder(CodecConfig(hidden=geo.hidden, filters=geo.filters, codebook_size=geo.codebook_size,
                                       n_codebooks=geo.n_codebooks), max_frames=768, max_batch=4, encoder=True)
        d.load_state_dict(E.make_enc_weights(geo, 3), strict=True)
        _ENC["d"] = d.to(DEV)
    return _ENC["d"]


def test_encode_with_sr_is_resample_then_encode():
    from valle_amd.codec import AudioTokenizer, Resampler

    enc = _codec()
    wav = (RR.make_noise(3 * 48000, 11, channels=2) * 0.1).to(DEV)
    want = enc.encode(Resampler(48000, 24000).to(DEV)(wav))
    got = enc.encode(wav, sr=48000)
    assert got.shape == want.shape == (1, 8, 225) and got.dtype == torch.int64
    assert torch.equal(got, want)
    assert enc.resampler(48000, 24000) is enc.resampler(48000, 24000)  # kept per rate pair
    batch = enc.encode_batch([wav, wav[:1, :5000]], sr=48000)
    assert torch.equal(batch[0], want) and batch[1].shape == (1, 8, 8)
    tok = AudioTokenizer(enc)
    assert torch.equal(tok.encode(wav[None], sr=48000)[0][0], want)


def test_encode_without_sr_is_what_it_was():
    enc = _codec()
    wav = E.make_wave(24001, 8).to(DEV)
    raw = torch.empty((1, 8, 76), dtype=torch.int64, device=DEV)
    flat = wav.reshape(-1).contiguous()
    enc._encode_raw([flat.data_ptr()], [flat.numel()], 8, [raw.data_ptr()])
    assert torch.equal(enc.encode(wav), raw)
    assert torch.equal(enc.encode(wav, sr=24000), raw)
    with pytest.raises(AssertionError):
        enc.encode(torch.zeros(2, 100, device=DEV))  # two channels without sr: refused as before


def test_decode_with_sr_is_decode_then_resample():
    from valle_amd.codec import AudioTokenizer, Resampler

    enc = _codec()
    g = torch.Generator().manual_seed(5)
    codes = torch.randint(0, 1024, (1, 8, 75), generator=g)
    plain = enc.decode(codes)
    assert plain.shape == (1, 1, 24000)
    want = Resampler(24000, 48000).to(DEV)(plain)
    got = enc.decode(codes, sr=48000)
    assert got.shape == want.shape == (1, 1, 48000) and torch.equal(got, want)
    assert torch.equal(enc.decode(codes, sr=24000), plain) and torch.equal(enc.decode(codes), plain)
    assert torch.equal(AudioTokenizer(enc).decode([(codes, None)], sr=48000), want)
    down = enc.decode_batch([codes[0], codes[0, :, :10]], sr=16000)
    assert down[0].shape == (1, 1, 16000) and down[1].shape == (1, 1, RR.out_length(24000, 16000, 3200))


def test_tokenize_audio_on_a_stereo_wav_file(tmp_path):
    from valle_amd.codec import AudioTokenizer, Resampler, convert_audio, load_wav, save_wav, tokenize_audio

    enc = _codec()
    L = 44100 * 2 + 17
    wav = (RR.make_noise(L, 21, channels=2) * 0.1).clamp(-1, 1)
    path = str(tmp_path / "prompt.wav")
    save_wav(path, wav, 44100)
    out = tokenize_audio(AudioTokenizer(enc), path)
    assert isinstance(out, list) and len(out) == 1 and out[0][1] is None
    codes = out[0][0]
    Lr = RR.out_length(44100, 24000, L)
    assert codes.shape == (1, 8, -(-Lr // 320)) and codes.dtype == torch.int64 and codes.is_cuda
    loaded, sr = load_wav(path)
    assert sr == 44100 and loaded.shape == (2, L)
    mono = Resampler(44100, 24000).to(DEV)(loaded)
    assert mono.shape == (1, 1, Lr)
    assert torch.equal(codes, enc.encode(mono))
    assert torch.equal(convert_audio(loaded.to(DEV), sr), mono[0])
    # the file's 16-bit samples resample to what fp64 gives
    ref = torch.from_numpy(RR.resample_direct(loaded, 44100, 24000))
    floor = float((RR.resample_polyphase(loaded, 44100, 24000, torch.float32).double() - ref).abs().max())
    err = float((mono[0, 0].double().cpu() - ref).abs().max())
    print(f"wav prompt 44100 -> 24000: floor {floor:.3e} engine {err:.3e} ratio {err / floor:.2f}")
    assert err <= RR.tolerance(floor)


def test_tokenize_audio_mixes_down_a_stereo_file_already_at_24_khz(tmp_path):
    """The reference calls convert_audio whatever the file's rate: a stereo 24 kHz file is mixed down (orig == new: the channel
    mean, bit for bit) and its codes are those of the mean; a mono 24 kHz file goes to the encoder as it is."""
    from valle_amd.codec import AudioTokenizer, load_wav, save_wav, tokenize_audio

    enc = _codec()
    tok = AudioTokenizer(enc)
    wav = (RR.make_noise(24000 + 11, 31, channels=2) * 0.1).clamp(-1, 1)
    path = str(tmp_path / "stereo24k.wav")
    save_wav(path, wav, 24000)
    loaded, sr = load_wav(path)
    assert sr == 24000 and loaded.shape == (2, 24011)
    want = enc.encode(loaded.mean(0).to(DEV))
    codes = tokenize_audio(tok, path)[0][0]
    assert codes.shape == (1, 8, 76) and torch.equal(codes, want)
    assert torch.equal(tok.encode(loaded[None].to(DEV), sr=24000)[0][0], want)
    assert torch.equal(enc.encode(loaded.to(DEV), sr=24000), want)
    mono = str(tmp_path / "mono24k.wav")
    save_wav(mono, loaded[:1], 24000)
    assert torch.equal(tokenize_audio(tok, mono)[0][0], enc.encode(loaded[:1].to(DEV)))
    with pytest.raises(AssertionError):
        tok.encode(loaded[None].to(DEV))  # without sr: (B, 1, L) as before
