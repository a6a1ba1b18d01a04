"""No GPU: the host support the translation units share (csrc/host.hpp).

Every unit reports through the one thread-local message behind vx_last_error(), and a failing HIP call names the unit that made
it, also where DevBuf, CallStage or open_device made it on the unit's behalf.  Without a device the first HIP call of each entry
fails: the small handles (vx_fbank, vx_resampler, vx_dtw, vx_gan here; vx_pitch, vx_stft and vx_vocoder in their own files) must
come out of that failed first use as they went in - the same answer a second time, a clean destroy - and the op-level entries
must give their scratch back.  Where a GPU is present the same calls succeed (the buffers are then real device memory), so either
return code is accepted and the message is checked only on failure.  Every handle also closes without ever having reached a
device, every *_create on the shared head (create_head) refuses a null argument and a wrong struct_size in the same words, and
every *_set_weight on the shared weight table (csrc/weights_host.hpp) refuses an unknown key and a wrong shape in the same words."""
import ctypes as C

import pytest
import torch

import ganvoc_ref as GR
from valle_amd import engine as E
from valle_amd.codec import Resampler
from valle_amd.dtw import DTW
from valle_amd.engine import VxDtwConfig
from valle_amd.fbank import BigVGANFbank
from valle_amd.ganvoc import GanVocoder
from valle_amd.pitch import PitchTracker
from valle_amd.stft import MultiResolutionSTFT
from valle_amd.vocoder import GriffinLim

VX_ERR_ARG = 1  # include/vallex.h

DEV = "cuda" if torch.cuda.is_available() else "cpu"  # without a GPU the pointers are never dereferenced


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


def _buf(*shape, dtype=torch.float32):
    return torch.ones(*shape, dtype=dtype, device=DEV)


def _twice(lib, call, hip_call, unit):
    """The call, and the identical call again: VX_OK both times with a GPU, VX_ERR_HIP both times without, naming call and unit."""
    seen = []
    for _ in range(2):
        rc = call()
        assert rc in (0, 2), (rc, lib.vx_last_error())
        if rc == 2:
            msg = lib.vx_last_error().decode()
            assert hip_call in msg and " failed: " in msg and unit + ":" in msg, msg
            seen.append(msg)
        else:
            seen.append(None)
    assert seen[0] == seen[1]
    if DEV == "cuda":
        torch.cuda.synchronize()


def test_fbank_first_use_without_a_device_leaves_a_usable_handle(lib):
    fb = BigVGANFbank(max_batch=2)
    wav, out = _buf(300), _buf(1, 100)
    wp, L, op = (C.c_void_p * 1)(wav.data_ptr()), (C.c_int32 * 1)(300), (C.c_void_p * 1)(out.data_ptr())
    _twice(lib, lambda: lib.vx_fbank_extract(fb._h, 1, wp, L, op, None), "hipGetDevice", "fbank.hip")
    assert lib.vx_fbank_extract(fb._h, 3, wp, L, op, None) == 4  # the host-side checks still answer
    fb.close()


def test_resampler_first_use_without_a_device_leaves_a_usable_handle(lib):
    h = C.c_void_p()
    assert lib.vx_resampler_create(16000, 24000, 2, C.byref(h)) == 0
    wav, out = _buf(64), _buf(96)
    ip, ch, L, op = (C.c_void_p * 1)(wav.data_ptr()), (C.c_int32 * 1)(1), (C.c_int32 * 1)(64), (C.c_void_p * 1)(out.data_ptr())
    _twice(lib, lambda: lib.vx_resample(h, 1, ip, ch, L, op, None), "hipGetDevice", "codec.hip")
    assert lib.vx_resample(h, 3, ip, ch, L, op, None) == 4
    lib.vx_resampler_destroy(h)


def test_dtw_first_use_without_a_device_leaves_a_usable_handle(lib):
    c = VxDtwConfig()
    c.struct_size = C.sizeof(VxDtwConfig)
    c.dim, c.n_ceps, c.max_frames, c.max_batch = 8, 3, 16, 2
    h = C.c_void_p()
    assert lib.vx_dtw_create(C.byref(c), C.byref(h)) == 0
    a, b, total, length = _buf(5, 8), _buf(4, 8), _buf(1, dtype=torch.float64), _buf(1, dtype=torch.int32)
    ap, ta, bp, tb = (C.c_void_p * 1)(a.data_ptr()), (C.c_int32 * 1)(5), (C.c_void_p * 1)(b.data_ptr()), (C.c_int32 * 1)(4)
    _twice(lib, lambda: lib.vx_dtw_compare(h, 1, ap, ta, bp, tb, total.data_ptr(), length.data_ptr(), None, None), "hipGetDevice",
           "dtw.hip")
    assert lib.vx_dtw_compare(h, 3, ap, ta, bp, tb, total.data_ptr(), length.data_ptr(), None, None) == 4
    lib.vx_dtw_destroy(h)


def _gan():
    cfg = GR.GEOMETRIES["g1_snakebeta"]
    return GanVocoder(cfg, state_dict=GR.make_weights(cfg, 1), max_batch=2, max_total_frames=50)


def test_gan_first_use_without_a_device_leaves_a_usable_handle(lib):
    v = _gan()
    mel, wav = _buf(4, 100), _buf(16)
    mp, T, wp = (C.c_void_p * 1)(mel.data_ptr()), (C.c_int32 * 1)(4), (C.c_void_p * 1)(wav.data_ptr())
    _twice(lib, lambda: lib.vx_gan_synthesize(v._h, 1, mp, T, wp, None), "hipGetDevice", "ganvoc.hip")
    assert lib.vx_gan_synthesize(v._h, 3, mp, T, wp, None) == 4  # the host-side checks still answer
    v.close()


def test_every_handle_closes_without_having_reached_a_device(lib):
    made = [BigVGANFbank(max_batch=2), Resampler(16000, 24000, max_batch=2), DTW(dim=8, n_ceps=3, max_frames=16, max_batch=2),
            PitchTracker(max_frames=64, max_batch=2), MultiResolutionSTFT(max_batch=2), GriffinLim(max_batch=2, max_total_frames=50),
            _gan()]
    assert [type(h)._PREFIX for h in made] == ["vx_fbank", "vx_resampler", "vx_dtw", "vx_pitch", "vx_stft", "vx_vocoder", "vx_gan"]
    for h in made:
        assert h._h is not None and h._bound is None
        h.close()
        assert h._h is None
    for prefix in ("vx_fbank", "vx_resampler", "vx_dtw", "vx_pitch", "vx_stft", "vx_vocoder", "vx_gan"):
        getattr(lib, prefix + "_destroy")(None)


def test_create_heads_refuse_in_the_same_words(lib):
    """VX_ERR_ARG, and the entry point's own name in front of the two texts of create_head."""
    for name, cfg_t in (("vx_fbank_create", E.VxFbankConfig), ("vx_dtw_create", E.VxDtwConfig), ("vx_pitch_create", E.VxPitchConfig),
                        ("vx_stft_create", E.VxStftConfig), ("vx_vocoder_create", E.VxVocoderConfig), ("vx_gan_create", E.VxGanConfig),
                        ("vx_spk_create", E.VxSpkConfig), ("vx_asr_create", E.VxAsrConfig), ("vx_wsp_create", E.VxWspConfig),
                        ("vx_codec_create", E.VxCodecConfig)):
        create, size, h = getattr(lib, name), C.sizeof(cfg_t), C.c_void_p()
        c = cfg_t()
        c.struct_size = size
        assert create(C.byref(c), None) == VX_ERR_ARG and lib.vx_last_error().decode() == name + ": null argument"
        assert create(None, C.byref(h)) == VX_ERR_ARG and lib.vx_last_error().decode() == name + ": null argument"
        c.struct_size = size + 4
        assert create(C.byref(c), C.byref(h)) == VX_ERR_ARG
        assert lib.vx_last_error().decode() == "%s: struct_size %d, expected %d" % (name, size + 4, size)
        assert not h.value


def _weighted_handles():
    """prefix -> (owner of an unfinalised handle, its key table) for the five handles on the shared weight table (weights_host.hpp)."""
    import asr_cases as AC
    import spk_cases as SC
    import whisper_cases as WC
    from valle_amd import asr, codec, ganvoc, spk, whisper

    dec = codec.EncodecDecoder(max_frames=8)
    dec.handle(finalize=False)
    gan = GanVocoder(GR.GEOMETRIES["g1_snakebeta"], max_batch=2, max_total_frames=50)
    enc = spk.SpeakerEncoder(SC.config("tiny_wavlm"), max_batch=2, max_seconds=1.0)
    ctc = asr.SpeechRecognizer(AC.config("tiny_group"), AC.vocab("tiny_group"), max_batch=2, max_seconds=1.0)
    wsp = whisper.WhisperRecognizer(WC.config("A"), max_batch=2)
    return {"vx_codec": (dec, codec.expected_keys(dec.cfg)), "vx_gan": (gan, ganvoc.expected_keys(gan.config)),
            "vx_spk": (enc, spk.expected_keys(enc.config, enc.attention)), "vx_asr": (ctc, asr.expected_keys(ctc.config)),
            "vx_wsp": (wsp, whisper.expected_keys(wsp.config))}


def test_set_weight_entries_refuse_in_the_same_words(lib):
    """VX_ERR_WEIGHTS for an unknown key and for a wrong shape - a wrong extent and a wrong rank - from all five *_set_weight; the
    shape text names the shape received and the shape expected.  The right shape is then taken."""
    fmt = lambda s: ", ".join(str(int(v)) for v in s)
    for prefix, (owner, keys) in _weighted_handles().items():
        put = getattr(lib, prefix + "_set_weight")
        key, shape = next((k, tuple(int(v) for v in s)) for k, s in keys.items() if len(s) >= 2)
        buf = torch.zeros(shape[:-1] + (shape[-1] + 1,))

        def rc_of(k, s):
            return put(owner._h, k.encode(), buf.data_ptr(), (C.c_int64 * len(s))(*s), len(s))

        assert rc_of(key + "_g", shape) == 6, prefix
        assert lib.vx_last_error().decode() == "unknown key %s_g" % key, prefix
        for wrong in (shape[:-1] + (shape[-1] + 1,), shape[:-1], shape + (1,)):
            assert rc_of(key, wrong) == 6, (prefix, wrong)
            assert lib.vx_last_error().decode() == "%s: shape (%s), expected (%s)" % (key, fmt(wrong), fmt(shape)), (prefix, wrong)
        assert rc_of(key, shape) == 0, prefix
        owner.close()


def test_op_entries_name_the_failing_call_and_their_unit(lib):
    V = 8
    logits, noise = _buf(V), _buf(V)
    out, lp = (C.c_int32 * 2)(), C.c_float()
    _twice(lib, lambda: lib.vx_op_sample(logits.data_ptr(), V, 2, 1.0, noise.data_ptr(), out, None), "hipMalloc", "engine.hip")
    _twice(lib, lambda: lib.vx_op_sample_topp(logits.data_ptr(), V, 2, 1.0, 0.5, noise.data_ptr(), out, None), "hipMalloc", "engine.hip")
    _twice(lib, lambda: lib.vx_op_sample_logprob(logits.data_ptr(), V, 2, 1.0, 0.5, noise.data_ptr(), out, C.byref(lp), None),
           "hipMalloc", "engine.hip")
    a, b, cost = _buf(5, 8), _buf(4, 8), _buf(5, 4)
    _twice(lib, lambda: lib.vx_op_dtw_cost(8, 3, a.data_ptr(), 5, b.data_ptr(), 4, cost.data_ptr(), None), "hipMalloc", "dtw.hip")
    total, length = _buf(1, dtype=torch.float64), _buf(1, dtype=torch.int32)
    desc = (C.c_int64 * 4)(5, 4, 0, 0)
    _twice(lib, lambda: lib.vx_op_dtw_path(cost.data_ptr(), 1, desc, total.data_ptr(), length.data_ptr(), None, None), "hipMalloc",
           "dtw.hip")
    assert lib.vx_op_sample(logits.data_ptr(), 1, 2, 1.0, noise.data_ptr(), out, None) == 5  # an argument error replaces the message
    assert b"sample: V=1" in lib.vx_last_error()
