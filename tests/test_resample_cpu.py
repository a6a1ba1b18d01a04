"""CPU: the sample-rate converter's two fp64 restatements (tests/resample_ref.py) against each other, the properties that make
the yardstick a test signal, WAV file I/O, vx_resample_length and the refusals of vx_resampler_create / vx_resample (all
returned before any HIP call), without a GPU.

The bounds of the signal properties are those measured for the rule itself in fp64 (1 s signals, 200 samples trimmed at each
end; measured value -> asserted bound): 1 kHz cosine from 48 / 44.1 kHz 3.4e-5 / 3.6e-5 -> 1e-4; 5 kHz cosine 4.3e-4 -> 1e-3;
16 kHz tone from 48 kHz (above the new Nyquist rate, inside the filter's transition band) 6.1e-3 -> 2e-2; 20 kHz tone 8.2e-4 ->
5e-3; DC gain 4.6e-4 (6.8e-4 from 16 kHz) -> 2e-3."""
import ctypes as C
import math
import os
import re
import struct
import wave

import numpy as np
import pytest
import torch

import resample_ref as RR
from conftest import ROOT

LENGTHS = (1, 7, 1000, 4801)
FP32_FLOOR = 6.5e-7  # largest fp32 floor on unit-variance noise (the GPU test measures it per case)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


# ---- 1. the restatements -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig", RR.RATES_IN)
def test_direct_definition_equals_polyphase_form(orig):
    worst = 0.0
    for L in LENGTHS:
        x = RR.make_noise(L, 100 + L)
        a = RR.resample_direct(x, orig, 24000)
        b = RR.resample_polyphase(x, orig, 24000).numpy()
        assert a.shape == b.shape == (RR.out_length(orig, 24000, L),), (orig, L)
        worst = max(worst, float(np.abs(a - b).max()))
    print(f"{orig} -> 24000: direct against polyphase {worst:.2e}")
    assert worst <= 1e-10


@pytest.mark.parametrize("new", RR.RATES_OUT)
def test_direct_definition_equals_polyphase_form_upwards(new):
    for L in LENGTHS:
        x = RR.make_noise(L, 200 + L, channels=2)
        a = RR.resample_direct(x, 24000, new)
        b = RR.resample_polyphase(x, 24000, new).numpy()
        assert a.shape == b.shape == (RR.out_length(24000, new, L),)
        assert float(np.abs(a - b).max()) <= 1e-10, (new, L)


def test_output_length_and_identity():
    for orig, new in [(r, 24000) for r in RR.RATES_IN] + [(24000, r) for r in RR.RATES_OUT]:
        o, n, _ = RR.ratio(orig, new)
        for L in (1, 2, 7, 146, 147, 148, 4801, 72000):
            assert RR.out_length(orig, new, L) == math.ceil(n * L / o) >= 1
            if L <= 148:
                assert RR.resample_direct(RR.make_noise(L, L), orig, new).shape == (math.ceil(n * L / o),)
    x = RR.make_noise(333, 1, channels=2)
    want = x.double().mean(0)
    assert np.array_equal(RR.resample_direct(x, 24000, 24000), want.numpy())
    assert torch.equal(RR.resample_polyphase(x, 48000, 48000), want)
    assert torch.equal(RR.resample_polyphase(x, 24000, 24000, torch.float32), x.mean(0))


def _tone(f, sr, seconds=1.0):
    return torch.cos(2 * math.pi * f * torch.arange(int(sr * seconds), dtype=torch.float64) / sr)


@pytest.mark.parametrize("orig,f,bound", [(48000, 1000, 1e-4), (44100, 1000, 1e-4), (48000, 5000, 1e-3), (44100, 5000, 1e-3)])
def test_passband_cosine_is_kept(orig, f, bound):
    y = RR.resample_direct(_tone(f, orig), orig, 24000)
    d = float(np.abs(y - _tone(f, 24000).numpy())[200:-200].max())
    print(f"{f} Hz cosine {orig} -> 24000: distance to the ideal cosine {d:.2e}")
    assert d <= bound


@pytest.mark.parametrize("f,bound", [(16000, 2e-2), (20000, 5e-3)])
def test_tone_above_the_new_nyquist_rate_is_removed(f, bound):
    y = RR.resample_direct(_tone(f, 48000), 48000, 24000)
    d = float(np.abs(y[200:-200]).max())
    print(f"{f} Hz tone 48000 -> 24000: residual amplitude {d:.2e}")
    assert d <= bound


@pytest.mark.parametrize("orig", [48000, 16000])
def test_dc_gain(orig):
    y = RR.resample_direct(torch.ones(orig, dtype=torch.float64), orig, 24000)
    d = float(np.abs(y[200:-200] - 1.0).max())
    print(f"DC {orig} -> 24000: gain error {d:.2e}")
    assert d <= 2e-3


@pytest.mark.parametrize("orig,new", [(48000, 24000), (44100, 24000), (16000, 24000), (24000, 44100)])
def test_wrong_restatements_are_visible(orig, new):
    """A dropped tap, and the mean taken after resampling channels that were clipped to [-1, 1] on the way (what a detour over a
    16-bit file per channel would do; the resampling itself is linear, so without the clip the order would not matter), each move
    the output by more than 100 x the fp32 floor; the floor length changes the length wherever o does not divide n L."""
    x = RR.make_noise(4801, 9, channels=2) * 1.5
    right = RR.resample_direct(x, orig, new)
    for v in ("drop_tap", "mean_after_clip"):
        d = float(np.abs(RR.resample_direct(x, orig, new, variant=v) - right).max())
        print(f"{orig} -> {new} {v}: moves the output by {d:.3e}")
        assert d > 100 * FP32_FLOOR, v
    o, n, _ = RR.ratio(orig, new)
    assert (n * 4801) % o != 0
    assert RR.resample_direct(x, orig, new, variant="floor_length").shape[0] == right.shape[0] - 1


def test_fp32_floor_is_small_against_the_signal():
    """The floor form in fp32 stays within 1e-6 of fp64 on unit-variance noise: what 4 x floor admits is far below every wrong
    variant above."""
    for orig, new in ((44100, 24000), (11025, 24000), (24000, 48000)):
        x = RR.make_noise(4801, 3, channels=2)
        f = float((RR.resample_polyphase(x, orig, new, torch.float32).double() - RR.resample_polyphase(x, orig, new)).abs().max())
        print(f"{orig} -> {new}: fp32 floor {f:.2e}")
        assert 0 < f <= 2e-6


# ---- 2. WAV files ----------------------------------------------------------------------------------------------------------
def _write_pcm(path, ints, width, sr, nch):
    """ints: (L, nch) Python ints in the width's signed range (8-bit is stored unsigned, as WAV does)."""
    with wave.open(path, "wb") as f:
        f.setnchannels(nch)
        f.setsampwidth(width)
        f.setframerate(sr)
        if width == 1:
            raw = bytes(int(v) + 128 for row in ints for v in row)
        elif width == 3:
            raw = b"".join(struct.pack("<i", int(v))[:3] for row in ints for v in row)
        else:
            raw = b"".join(struct.pack("<h" if width == 2 else "<i", int(v)) for row in ints for v in row)
        f.writeframes(raw)


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_load_wav_reads_pcm_widths(tmp_path, width):
    from valle_amd.codec import load_wav

    bits = 8 * width
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    rng = np.random.default_rng(width)
    ints = rng.integers(lo, hi + 1, size=(257, 2))
    ints[0], ints[1], ints[2] = (lo, hi), (0, -1), (1, lo + 1)
    p = str(tmp_path / f"pcm{bits}.wav")
    _write_pcm(p, ints.tolist(), width, 44100, 2)
    wav, sr = load_wav(p)
    assert sr == 44100 and wav.shape == (2, 257) and wav.dtype == torch.float32 and wav.is_contiguous()
    want = (ints.T.astype(np.float64) / float(1 << (bits - 1))).astype(np.float32)
    assert np.array_equal(wav.numpy(), want)
    assert float(wav.min()) == -1.0 and float(wav.max()) < 1.0 + (width == 4) * 1e-9


def test_save_wav_round_trip_is_exact_at_16_bits(tmp_path):
    from valle_amd.codec import load_wav, save_wav

    rng = np.random.default_rng(0)
    ints = rng.integers(-32768, 32768, size=(2, 1000))
    ints[:, 0], ints[:, 1] = (-32768, 32767), (0, -1)
    wav = torch.from_numpy(ints.astype(np.float32) / 32768.0)
    p = str(tmp_path / "a.wav")
    save_wav(p, wav, 22050)
    with wave.open(p, "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (2, 2, 22050, 1000)
    back, sr = load_wav(p)
    assert sr == 22050 and torch.equal(back, wav)
    save_wav(p, torch.tensor([[[2.0, -2.0, 0.25]]]), 8000)  # (1, 1, L): clamped to the int16 range, mono
    back, sr = load_wav(p)
    assert sr == 8000 and back.shape == (1, 3) and back[0].tolist() == [32767 / 32768, -1.0, 0.25]


# ---- 3. host side of the C ABI ---------------------------------------------------------------------------------------------------
def test_symbols_and_unchanged_struct_sizes(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = set(re.findall(r"\b(vx_[a-z0-9_]+)\s*\(", hdr))
    names = {"vx_resampler_create", "vx_resampler_destroy", "vx_resample", "vx_resample_length"}
    assert names <= declared and names <= set(engine.declared_symbols())
    assert all(hasattr(lib, n) for n in names)
    assert C.sizeof(engine.VxCodecConfig) == 72 and C.sizeof(engine.VxConfig) == 64 and C.sizeof(engine.VxDecodeParams) == 56


def test_resample_length_matches_the_formula(lib):
    from valle_amd.codec import Resampler, resample_length

    for orig, new in [(r, 24000) for r in RR.RATES_IN] + [(24000, r) for r in RR.RATES_OUT] + [(24000, 24000), (44101, 24000)]:
        for L in (1, 2, 7, 1000, 4801, 144000, 2 ** 31 - 1):
            assert lib.vx_resample_length(orig, new, L) == RR.out_length(orig, new, L), (orig, new, L)
    assert resample_length(44100, 24000, 4801) == 2613
    assert Resampler(48000, 24000).output_length(1) == 1 and Resampler(8000, 24000).output_length(1) == 3
    for bad in ((0, 24000, 5), (24000, -1, 5), (24000, 16000, 0)):
        assert lib.vx_resample_length(*bad) == -1
        with pytest.raises(ValueError):
            resample_length(*bad)


def test_create_refusals(lib):
    h = C.c_void_p()
    assert lib.vx_resampler_create(48000, 24000, 1, None) == 1
    for args, code in (((0, 24000, 1), 1), ((48000, -5, 1), 1), ((48000, 24000, 0), 1),
                       ((2 ** 31 - 1, 2 ** 31 - 2, 1), 5),   # 2^31 phases: the table does not fit
                       ((2 ** 31 - 1, 1, 1), 5)):            # one output's window is longer than the kernel's
        assert lib.vx_resampler_create(*args, C.byref(h)) == code, args
        assert lib.vx_last_error()
    for args in ((48000, 24000, 256), (48000, 24000, 4096), (11025, 24000, 1), (24000, 44100, 4), (24000, 24000, 1), (44101, 24000, 1), (192000, 8000, 1)):
        assert lib.vx_resampler_create(*args, C.byref(h)) == 0, args
        lib.vx_resampler_destroy(h)
    lib.vx_resampler_destroy(None)


def test_resample_refusals_before_any_hip_call(lib):
    from valle_amd.codec import Resampler
    from valle_amd.engine import VxError

    r = Resampler(48000, 24000, max_batch=2)  # never moved to a device: no HIP call may be reached

    def code_of(ins, ch, lens, outs=None):
        with pytest.raises(VxError) as e:
            r._resample_raw(ins, ch, lens, outs or [8] * len(ins))
        return e.value.code

    assert code_of([8], [1], [0]) == 1                    # no samples
    assert code_of([8], [1], [-3]) == 1
    assert code_of([8], [0], [100]) == 1                  # no channel
    assert code_of([0], [1], [100]) == 1                  # null input
    assert code_of([8], [1], [100], outs=[0]) == 1        # null output
    assert code_of([8, 8, 8], [1] * 3, [100] * 3) == 4    # n > max_batch
    assert code_of([8, 8], [2, 1], [100, 0]) == 1         # every utterance is checked
    assert r._h is not None
    assert lib.vx_resample(r._h, 0, None, None, None, None, None) == 1
    assert lib.vx_resample(None, 1, None, None, None, None, None) == 1
    up = Resampler(8000, 24000)
    with pytest.raises(VxError) as e:
        up._resample_raw([8], [1], [2 ** 31 - 1], [8])    # 3 (2^31 - 1) output samples
    assert e.value.code == 5
    r.close()
    up.close()


def test_no_cpu_fallback_and_mono_target_only():
    import encodec_enc_ref as E
    from valle_amd.codec import AudioTokenizer, CodecConfig, EncodecDecoder, Resampler, convert_audio

    x = RR.make_noise(480, 0, channels=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Resampler(48000, 24000)(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        convert_audio(x, 48000)
    with pytest.raises(NotImplementedError):
        convert_audio(x, 48000, 24000, 2)
    d = EncodecDecoder(CodecConfig(hidden=16, filters=4, codebook_size=64), max_frames=8, encoder=True)
    d.load_state_dict(E.make_enc_weights(E.NARROW, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.encode(x, sr=48000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AudioTokenizer(d).encode(x[None], sr=48000)
    with pytest.raises(AssertionError):
        AudioTokenizer(d).encode(x[None])  # without sr: (B, 1, L) as before


def test_resampler_handle_follows_the_device():
    """The C handle keeps its tables on the device of its first call: `.to()` of another device drops it and the next call
    makes a fresh one; before a first call, and for the same device, the handle stays."""
    from valle_amd.codec import Resampler

    r = Resampler(44100, 24000)
    h = r._h
    assert h is not None and r.to("cuda:0")._h is h and r.to("cuda:1")._h is h   # never used: nothing is bound yet
    r._bound = torch.device("cuda", 0)                                           # as after a call on cuda:0
    assert r.to("cuda:0")._h is h
    assert r.to("cuda:1")._h is None and r._bound is None
    assert r._handle() is not None
    r.close()
    assert r._h is None


def test_public_names():
    import valle_amd

    for n in ("Resampler", "convert_audio", "load_wav", "save_wav", "tokenize_audio"):
        assert n in valle_amd.__all__ and callable(getattr(valle_amd, n))
