"""No GPU: the log-mel filterbank's restatements (tests/fbank_ref.py), the mel basis, the host side of the C ABI (vx_fbank_*)
and the Python surface of valle_amd.fbank.

* the fp64 four-step restatement (the kernel's organisation of the DFT) equals the fp64 definition (torch.stft) to 1e-10;
* the frame rule at L = 127, 128, 383, 384, 1024;
* the mel basis: shape, sign, no empty filter, ascending peaks, a second formulation written filter by filter, and the built-in
  table of the C side;
* vx_fbank_create / vx_fbank_extract refuse what the header says they refuse, without any HIP call;
* config round trip, feature_dim, frame_shift, mix, compute_energy, mel_distance, no CPU fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import fbank_ref as FR
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


@pytest.fixture(scope="module")
def basis(lib):
    from valle_amd.fbank import slaney_mel_basis

    return slaney_mel_basis(24000, 1024, 100, 0.0, 12000.0)


# ---- 1. the restatements -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (128, 1024, 1025, 4801, 24000))
def test_four_step_equals_the_definition_in_fp64(basis, L):
    for amp in (0.1, 1.0):
        x = FR.make_noise(L, L + int(10 * amp), amp)
        want = FR.fbank_definition(x, basis)
        got = FR.fbank_four_step(x, basis)
        assert want.shape == got.shape == (FR.n_frames(L), 100) and want.dtype == torch.float64
        assert float((got - want).abs().max()) < 1e-10


def test_fp32_floor_is_about_one_ulp_of_the_log(basis):
    x = FR.make_noise(4801, 3)
    ref = FR.fbank_definition(x, basis)
    floor = float((FR.fbank_definition(x, basis, torch.float32).double() - ref).abs().max())
    assert ref.dtype == torch.float64 and 1e-8 < floor < 5e-6  # fp32 ulp at |x| in 4 .. 8 is 4.8e-7
    assert FR.share_near_clip(x, basis) == 0.0


def test_frame_rule(lib):
    from valle_amd.fbank import num_frames

    for L, want in ((127, 0), (128, 1), (383, 1), (384, 2), (1024, 4)):
        assert FR.n_frames(L) == num_frames(L) == lib.vx_fbank_frames(L) == want, L
    for L in (0, 1, 255, 256, 4801, 72001, 2 ** 31 - 1, 2 ** 40 + 128):
        assert lib.vx_fbank_frames(L) == num_frames(L) == (L + 128) // 256
    assert lib.vx_fbank_frames(-5) == 0
    # the zero padding completes the last frame: never negative
    for L in range(128, 2048):
        assert (FR.n_frames(L) - 1) * 256 + 1024 - L >= 0


# ---- 2. the mel basis --------------------------------------------------------------------------------------------------------
def test_mel_basis_properties(basis):
    assert tuple(basis.shape) == (100, 513) and basis.dtype == torch.float32
    assert bool((basis >= 0).all())
    nz = (basis > 0).sum(1)
    assert int(nz.min()) >= 1, "an empty filter"
    assert (int(nz.min()), int(nz.max())) == (2, 34)
    peaks = basis.argmax(1)
    assert bool((peaks[1:] > peaks[:-1]).all()), "peaks are not strictly ascending"
    # a filter's non-zero bins are one band
    for m in range(100):
        idx = torch.nonzero(basis[m] > 0).reshape(-1)
        assert int(idx[-1] - idx[0]) + 1 == idx.numel()


def test_mel_basis_against_a_second_formulation():
    from valle_amd.fbank import slaney_mel_basis, slaney_mel_basis_f64

    for n_mels, fmin, fmax in ((100, 0.0, 12000.0), (80, 0.0, 8000.0), (37, 50.0, 11000.0), (128, 0.0, 12000.0)):
        loops = FR.mel_basis_loops(24000, 1024, n_mels, fmin, fmax)
        ours = slaney_mel_basis_f64(24000, 1024, n_mels, fmin, fmax)
        assert ours.dtype == np.float64 and ours.shape == loops.shape == (n_mels, 513)
        assert float(np.abs(ours - loops).max()) < 1e-12
        # the table is that, rounded once
        assert np.array_equal(slaney_mel_basis(24000, 1024, n_mels, fmin, fmax).numpy(), ours.astype(np.float32))
    from valle_amd import fbank as FB

    w64 = FB._mel_to_hz(np.linspace(FB._hz_to_mel(0.0), FB._hz_to_mel(12000.0), 102))
    assert abs(float(w64[0])) < 1e-12 and abs(float(w64[-1]) - 12000.0) < 1e-8
    assert abs(float(FB._hz_to_mel(1000.0)) - 15.0) < 1e-12 and abs(float(FB._mel_to_hz(15.0)) - 1000.0) < 1e-9


def test_builtin_basis_of_the_c_side_is_the_packages(lib, basis):
    from valle_amd.engine import VxFbankConfig

    for n_mels, fmin, fmax in ((100, 0.0, 12000.0), (37, 50.0, 11000.0)):
        c = _config(n_mels=n_mels, fmin=fmin, fmax=fmax)
        h = C.c_void_p()
        assert lib.vx_fbank_create(C.byref(c), C.byref(h)) == 0
        out = np.full((n_mels, 513), np.nan, dtype=np.float32)
        assert lib.vx_fbank_get_mel_basis(h, out.ctypes.data) == 0
        loops = FR.mel_basis_loops(24000, 1024, n_mels, fmin, fmax)
        assert np.isfinite(out).all()
        # fp64 rounded once: within an fp32 ulp of the largest weight of the fp64 table
        assert float(np.abs(out.astype(np.float64) - loops).max()) <= 2.0 ** -23 * float(np.abs(loops).max())
        # a table of the caller's replaces it
        mine = np.arange(n_mels * 513, dtype=np.float32).reshape(n_mels, 513)
        assert lib.vx_fbank_set_mel_basis(h, mine.ctypes.data) == 0
        assert lib.vx_fbank_get_mel_basis(h, out.ctypes.data) == 0 and np.array_equal(out, mine)
        assert lib.vx_fbank_set_mel_basis(h, None) == 1 and lib.vx_fbank_set_mel_basis(None, mine.ctypes.data) == 1
        lib.vx_fbank_destroy(h)
    assert C.sizeof(VxFbankConfig) == 36


# ---- 3. host side of the C ABI -----------------------------------------------------------------------------------------------
def _config(**kw):
    from valle_amd.engine import VxFbankConfig

    c = VxFbankConfig()
    c.struct_size = C.sizeof(VxFbankConfig)
    c.sample_rate, c.n_fft, c.hop, c.n_mels, c.fmin, c.fmax, c.clip, c.max_batch = 24000, 1024, 256, 100, 0.0, 12000.0, 1e-5, 4
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_symbols(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = set(re.findall(r"\b(vx_[a-z0-9_]+)\s*\(", hdr))
    names = {"vx_fbank_create", "vx_fbank_destroy", "vx_fbank_set_mel_basis", "vx_fbank_frames", "vx_fbank_extract"}
    assert names <= declared and names <= set(engine.declared_symbols())
    assert all(hasattr(lib, n) for n in names)
    assert C.sizeof(engine.VxCodecConfig) == 72 and C.sizeof(engine.VxConfig) == 64 and C.sizeof(engine.VxDecodeParams) == 56


def test_create_refusals(lib):
    h = C.c_void_p()
    assert lib.vx_fbank_create(C.byref(_config()), None) == 1
    assert lib.vx_fbank_create(None, C.byref(h)) == 1
    for kw, code in (({"struct_size": 0}, 1), ({"struct_size": 40}, 1), ({"max_batch": 0}, 1), ({"clip": 0.0}, 1),
                     ({"clip": float("nan")}, 1),
                     ({"sample_rate": 16000}, 5), ({"n_fft": 2048}, 5), ({"hop": 300}, 5), ({"n_mels": 0}, 5), ({"n_mels": 129}, 5),
                     ({"fmin": -1.0}, 5), ({"fmin": 8000.0, "fmax": 8000.0}, 5), ({"fmax": 12000.5}, 5),
                     ({"fmin": float("nan")}, 5)):
        assert lib.vx_fbank_create(C.byref(_config(**kw)), C.byref(h)) == code, kw
        assert lib.vx_last_error()
    for kw in ({}, {"n_mels": 1}, {"n_mels": 128}, {"fmin": 50.0, "fmax": 7600.0}, {"max_batch": 4096}):
        assert lib.vx_fbank_create(C.byref(_config(**kw)), C.byref(h)) == 0, kw
        lib.vx_fbank_destroy(h)
    lib.vx_fbank_destroy(None)


def test_extract_refusals_before_any_hip_call(lib):
    from valle_amd.engine import VxError
    from valle_amd.fbank import BigVGANFbank

    fb = BigVGANFbank(max_batch=2)  # never moved to a device: no HIP call may be reached

    def code_of(ins, lens, outs=None):
        with pytest.raises(VxError) as e:
            fb._extract_raw(ins, lens, outs or [8] * len(ins))
        return e.value.code

    assert code_of([8], [0]) == 1                     # no samples
    assert code_of([8], [-3]) == 1
    assert code_of([0], [1000]) == 1                  # null input
    assert code_of([8], [1000], outs=[0]) == 1        # null output
    assert code_of([8, 8, 8], [1000] * 3) == 4        # n > max_batch
    assert code_of([8, 8], [1000, 0]) == 1            # every utterance is checked
    assert fb._h is not None
    assert lib.vx_fbank_extract(fb._h, 0, None, None, None, None) == 1
    assert lib.vx_fbank_extract(None, 1, None, None, None, None) == 1
    fb._extract_raw([8, 8], [127, 1], [8, 8])         # no frame anywhere: nothing to do, and no device is touched
    assert fb._bound is None
    fb.close()
    assert fb._h is None


# ---- 4. the Python surface ---------------------------------------------------------------------------------------------------
def test_config_and_reference_surface(lib):
    from valle_amd.fbank import BigVGANFbank, BigVGANFbankConfig, get_fbank_extractor

    cfg = BigVGANFbankConfig()
    d = cfg.to_dict()
    assert d == {"frame_length": 1024 / 24000.0, "frame_shift": 256 / 24000.0, "remove_dc_offset": True, "round_to_power_of_two": True,
                 "low_freq": 0.0, "high_freq": 12000.0, "num_mel_bins": 100, "use_energy": False}
    assert BigVGANFbankConfig.from_dict(d) == cfg
    fb = get_fbank_extractor(device="cpu")
    assert isinstance(fb, BigVGANFbank) and fb.name == "fbank" and fb.config_type is BigVGANFbankConfig
    assert fb.feature_dim(24000) == 100 and fb.frame_shift == 256 / 24000.0
    assert tuple(fb.mel_basis.shape) == (100, 513)
    a = np.log(np.array([[1.0, 2.0], [3.0, 4.0]]))
    b = np.log(np.array([[0.5, 0.5], [1.0, 0.0 + 1e-30]]))
    assert np.allclose(BigVGANFbank.mix(a, b, 2.0), np.log(np.array([[2.0, 3.0], [5.0, 4.0]])))
    assert np.allclose(BigVGANFbank.mix(np.full((1, 1), -80.0), np.full((1, 1), -80.0), 1.0), np.log(1e-10))  # the floor
    assert abs(BigVGANFbank.compute_energy(a) - 10.0) < 1e-12
    small = BigVGANFbank(BigVGANFbankConfig(num_mel_bins=37, low_freq=50.0, high_freq=11000.0))
    assert small.feature_dim(24000) == 37 and tuple(small.mel_basis.shape) == (37, 513)
    with pytest.raises(ValueError):
        BigVGANFbank(mel_basis=torch.zeros(100, 512))
    from valle_amd.engine import VxError

    with pytest.raises(VxError) as e:
        BigVGANFbank(BigVGANFbankConfig(num_mel_bins=200))
    assert e.value.code == 5
    with pytest.raises(VxError):
        BigVGANFbank(BigVGANFbankConfig(frame_shift=0.01))


def test_no_cpu_fallback_and_sampling_rate():
    from valle_amd.fbank import BigVGANFbank

    fb = BigVGANFbank()
    x = FR.make_noise(1000, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fb.extract(x.numpy(), 24000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fb.extract_batch([x])
    with pytest.raises(AssertionError):
        fb.extract(x, 16000)


def test_handle_follows_the_device():
    from valle_amd.fbank import BigVGANFbank

    fb = BigVGANFbank()
    h = fb._h
    assert h is not None and fb.to("cuda:0")._h is h and fb.to("cuda:1")._h is h   # never used: nothing is bound yet
    fb._bound = torch.device("cuda", 0)                                            # as after a call on cuda:0
    assert fb.to("cuda:0")._h is h
    assert fb.to("cuda:1")._h is None and fb._bound is None
    assert fb._handle() is not None
    fb.close()


def test_mel_distance_on_the_host():
    from valle_amd.fbank import mel_distance

    a = torch.arange(12.0).reshape(4, 3)
    assert float(mel_distance(a, a)) == 0.0
    assert float(mel_distance(a, a[:2] + 1.5)) == 1.5       # the common frames
    with pytest.raises(ValueError):
        mel_distance(a, a[:0])
    with pytest.raises(AssertionError):
        mel_distance(a, torch.zeros(4, 2))


def test_public_names():
    import valle_amd

    for n in ("BigVGANFbank", "BigVGANFbankConfig", "get_fbank_extractor", "mel_distance", "slaney_mel_basis"):
        assert n in valle_amd.__all__ and callable(getattr(valle_amd, n))
    from valle_amd.codec import EncodecDecoder

    assert callable(EncodecDecoder.roundtrip_mel_distance)
