"""No GPU: the Griffin-Lim vocoder's restatement (tests/vocoder_ref.py), the host side of the C ABI (vx_vocoder_*) and the Python
surface of valle_amd.vocoder.

* header, ctypes table and library agree on the vx_vocoder_* names; sizeof(VxVocoderConfig) == 40;
* vx_vocoder_create / vx_vocoder_synthesize refuse what the header says they refuse, in its order, without any HIP call;
* the least-squares inverse the C side computes by Cholesky equals numpy.linalg.pinv of the fp64 Slaney basis rounded to fp32,
  within one fp32 ulp per entry; a rank-deficient basis is refused, a caller's table is taken as it is;
* the restatement checks itself: S equals the STFT inside tests/fbank_ref.py, I(S(x)) returns x where the envelope is above its
  floor, and the spectral convergence falls over 32 iterations;
* valid arguments without a GPU fail at the first HIP call and leave the handle usable, as the other handles do."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import fbank_ref as FR
import vocoder_ref as VR
from conftest import ROOT

NAMES = {"vx_vocoder_create", "vx_vocoder_destroy", "vx_vocoder_set_mel_basis", "vx_vocoder_set_inverse", "vx_vocoder_get_inverse",
         "vx_vocoder_samples", "vx_vocoder_synthesize", "vx_vocoder_synthesize_warm"}
DEV = "cuda" if torch.cuda.is_available() else "cpu"  # without a GPU the pointers are never dereferenced


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


def _config(**kw):
    from valle_amd.engine import VxVocoderConfig

    c = VxVocoderConfig()
    c.struct_size = C.sizeof(VxVocoderConfig)
    c.sample_rate, c.n_fft, c.hop, c.n_mels, c.fmin, c.fmax, c.env_floor = 24000, 1024, 256, 100, 0.0, 12000.0, 0.1
    c.max_batch, c.max_total_frames = 4, 100
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ---- 1. the C ABI's names and refusals ----------------------------------------------------------------------------------------
def test_symbols_and_struct_size(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = set(re.findall(r"\b(vx_[a-z0-9_]+)\s*\(", hdr))
    assert {n for n in declared if n.startswith("vx_vocoder_")} == NAMES
    assert {n for n in engine.declared_symbols() if n.startswith("vx_vocoder_")} == NAMES
    assert all(hasattr(lib, n) for n in NAMES)
    assert C.sizeof(engine.VxVocoderConfig) == 40
    assert [f[0] for f in engine.VxVocoderConfig._fields_] == ["struct_size", "sample_rate", "n_fft", "hop", "n_mels", "fmin", "fmax",
                                                               "env_floor", "max_batch", "max_total_frames"]


def test_create_refusals(lib):
    h = C.c_void_p()
    assert lib.vx_vocoder_create(C.byref(_config()), None) == 1
    assert lib.vx_vocoder_create(None, C.byref(h)) == 1
    for kw, code in (({"struct_size": 0}, 1), ({"struct_size": 36}, 1), ({"max_batch": 0}, 1), ({"max_total_frames": 0}, 1),
                     ({"env_floor": 0.0}, 1), ({"env_floor": -0.1}, 1), ({"env_floor": float("nan")}, 1),
                     ({"env_floor": float("inf")}, 1),
                     ({"sample_rate": 16000}, 5), ({"n_fft": 2048}, 5), ({"hop": 300}, 5), ({"n_mels": 0}, 5), ({"n_mels": 129}, 5),
                     ({"fmin": -1.0}, 5), ({"fmin": 8000.0, "fmax": 8000.0}, 5), ({"fmax": 12000.5}, 5),
                     ({"fmin": float("nan")}, 5), ({"max_total_frames": 2 ** 21 + 1}, 5)):
        assert lib.vx_vocoder_create(C.byref(_config(**kw)), C.byref(h)) == code, kw
        assert lib.vx_last_error()
    for kw in ({}, {"n_mels": 1}, {"n_mels": 80, "fmax": 8000.0}, {"fmin": 50.0, "fmax": 7600.0}, {"max_batch": 4096}, {"env_floor": 1e-3}):
        assert lib.vx_vocoder_create(C.byref(_config(**kw)), C.byref(h)) == 0, kw
        lib.vx_vocoder_destroy(h)
    lib.vx_vocoder_destroy(None)


def test_samples(lib):
    from valle_amd.fbank import num_frames
    from valle_amd.vocoder import num_samples

    for T in (0, 1, 2, 17, 1875, 2 ** 21, 2 ** 40):
        assert lib.vx_vocoder_samples(T) == num_samples(T) == 256 * T
        assert lib.vx_fbank_frames(256 * T) == num_frames(256 * T) == T
    assert lib.vx_vocoder_samples(-3) == 0


def test_synthesize_refusals_before_any_hip_call(lib):
    from valle_amd.engine import VxError
    from valle_amd.vocoder import GriffinLim

    gl = GriffinLim(max_batch=2, max_total_frames=50)  # never moved to a device: no HIP call may be reached

    def code_of(mels, T, init=None, n_iter=1, momentum=0.5, wavs=None, phases=None, warm=False):
        with pytest.raises(VxError) as e:
            gl._synthesize_raw(mels, T, init, n_iter, momentum, wavs or [8] * len(mels), phases, warm=warm)
        return e.value.code

    assert code_of([8], [4], n_iter=-1) == 1
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert code_of([8], [4], momentum=bad) == 1, bad
    assert code_of([8], [-1]) == 1                          # a negative frame count
    assert code_of([0], [4]) == 1                           # null input
    assert code_of([8], [4], wavs=[0]) == 1                 # null output
    assert code_of([8], [4], init=[0]) == 1                 # an init_phase array with a null entry
    assert code_of([8], [4], phases=[0]) == 1               # a phase_out array with a null entry
    assert code_of([8, 8, 8], [4] * 3) == 4                 # n > max_batch
    assert code_of([8, 8, 8], [4] * 3, n_iter=-1) == 1      # the scalar arguments are checked before the capacity
    assert code_of([8, 8], [4, -1]) == 1                    # every utterance is checked
    assert code_of([8, 8], [30, 21]) == 4                   # 51 frames > max_total_frames
    assert code_of([8], [51]) == 4
    assert code_of([8, 0], [51, 4]) == 4                    # in order: the capacity of utterance 0 before the null of utterance 1
    h = gl._h
    assert h is not None
    assert lib.vx_vocoder_synthesize(h, 0, None, None, None, 1, 0.5, None, None, None) == 1
    assert lib.vx_vocoder_synthesize(None, 1, None, None, None, 1, 0.5, None, None, None) == 1
    one, T = (C.c_void_p * 1)(8), (C.c_int32 * 1)(4)
    assert lib.vx_vocoder_synthesize_warm(h, 1, one, T, None, 1, 0.5, one, None, None) == 1  # a warm start needs its start
    gl._synthesize_raw([8, 0], [0, 0], None, 3, 0.99, [8, 0], None)  # no frame anywhere: nothing to do, no device is touched
    gl._synthesize_raw([0], [0], [0], 0, 0.0, [0], [0], warm=True)
    assert gl._bound is None
    gl.close()
    assert gl._h is None


def test_valid_arguments_without_a_device_leave_a_usable_handle(lib):
    from valle_amd.vocoder import GriffinLim

    gl = GriffinLim(max_batch=2, max_total_frames=50)
    mel = torch.zeros(3, 100, device=DEV)
    wav = torch.zeros(768, device=DEV)
    mp, T, wp = (C.c_void_p * 1)(mel.data_ptr()), (C.c_int32 * 1)(3), (C.c_void_p * 1)(wav.data_ptr())
    seen = []
    for _ in range(2):
        rc = lib.vx_vocoder_synthesize(gl._h, 1, mp, T, None, 1, 0.99, wp, None, None)
        assert rc in (0, 2), (rc, lib.vx_last_error())
        msg = lib.vx_last_error().decode() if rc == 2 else None
        if rc == 2:
            assert "hipGetDevice" in msg and " failed: " in msg and "vocoder.hip:" in msg, msg
        seen.append(msg)
    assert seen[0] == seen[1]
    if DEV == "cuda":
        torch.cuda.synchronize()
    assert lib.vx_vocoder_synthesize(gl._h, 3, mp, T, None, 1, 0.99, wp, None, None) == 4  # the host-side checks still answer
    gl.close()


# ---- 2. the least-squares inverse of the mel basis ----------------------------------------------------------------------------
def _get_inverse(lib, h, n_mels):
    out = np.full((513, n_mels), np.nan, dtype=np.float32)
    assert lib.vx_vocoder_get_inverse(h, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("n_mels,fmin,fmax", ((100, 0.0, 12000.0), (80, 0.0, 8000.0), (37, 50.0, 11000.0)))
def test_inverse_is_the_pseudo_inverse_rounded_once(lib, n_mels, fmin, fmax):
    """Two fp64 methods (Cholesky of B B^T there, an SVD here) agree to cond(B B^T) eps |P|: 1.4e-13 for the 100-band table (cond
    30.9, max |P| 40.1), which is above an ulp of the table's smallest entries.  So: one fp32 ulp of the entry, plus 1e-12 for the
    difference of the two fp64 methods."""
    from valle_amd.fbank import slaney_mel_basis_f64

    h = C.c_void_p()
    assert lib.vx_vocoder_create(C.byref(_config(n_mels=n_mels, fmin=fmin, fmax=fmax)), C.byref(h)) == 0
    got = _get_inverse(lib, h, n_mels)
    want = VR.mel_inverse(slaney_mel_basis_f64(24000, 1024, n_mels, fmin, fmax))
    assert want.shape == (513, n_mels) and np.isfinite(got).all()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    excess = np.abs(got.astype(np.float64) - want) - ulp
    print(f"inverse {n_mels} mels: max |P| {np.abs(want).max():.2f}, worst |got - pinv| - ulp {excess.max():.3e}")
    assert float(excess.max()) <= 1e-12
    if n_mels == 100:
        assert abs(float(np.abs(want).max()) - 40.1) < 0.1
    lib.vx_vocoder_destroy(h)


def test_set_mel_basis_and_set_inverse(lib):
    from valle_amd.fbank import slaney_mel_basis

    h = C.c_void_p()
    assert lib.vx_vocoder_create(C.byref(_config(n_mels=37)), C.byref(h)) == 0
    before = _get_inverse(lib, h, 37)
    # a caller's basis: its inverse, from the fp32 table as given
    mine = slaney_mel_basis(24000, 1024, 37, 100.0, 9000.0).numpy()
    assert lib.vx_vocoder_set_mel_basis(h, mine.ctypes.data) == 0
    got = _get_inverse(lib, h, 37)
    want = VR.mel_inverse(mine.astype(np.float64))
    assert float((np.abs(got - want) - np.spacing(np.abs(want).astype(np.float32))).max()) <= 1e-12
    # rank-deficient: two equal filters, an empty filter, a non-finite weight -> refused, and the handle keeps what it had
    for spoil in ("equal", "empty", "nan"):
        bad = mine.copy()
        if spoil == "equal":
            bad[5] = bad[6]
        elif spoil == "empty":
            bad[9] = 0.0
        else:
            bad[3, 40] = np.nan
        assert lib.vx_vocoder_set_mel_basis(h, bad.ctypes.data) == 5, spoil
        assert b"Cholesky" in lib.vx_last_error()
        assert np.array_equal(_get_inverse(lib, h, 37), got)
    # the caller's own inverse, as it is
    table = np.arange(513 * 37, dtype=np.float32).reshape(513, 37)
    assert lib.vx_vocoder_set_inverse(h, table.ctypes.data) == 0
    assert np.array_equal(_get_inverse(lib, h, 37), table)
    assert lib.vx_vocoder_set_mel_basis(h, None) == 1 and lib.vx_vocoder_set_mel_basis(None, mine.ctypes.data) == 1
    assert lib.vx_vocoder_set_inverse(h, None) == 1 and lib.vx_vocoder_get_inverse(h, None) == 1
    assert not np.array_equal(before, got)
    lib.vx_vocoder_destroy(h)


# ---- 3. the restatement checks itself -----------------------------------------------------------------------------------------
def test_forward_is_the_filterbanks_stft():
    x = FR.make_noise(256 * 9, 5).double()
    S = VR.forward(x)
    window = torch.hann_window(1024, dtype=torch.float64)
    padded = torch.cat([x, torch.zeros(768, dtype=torch.float64)])
    want = torch.stft(padded[None], 1024, hop_length=256, win_length=1024, window=window, center=False, normalized=False,
                      onesided=True, return_complex=True)[0].T
    assert S.shape == want.shape == (9, 513)
    assert float((S - want).abs().max()) < 1e-10
    # and its magnitudes are the ones inside fbank_ref: basis @ sqrt(|S|^2 + 1e-9)
    basis = torch.eye(513, dtype=torch.float64)
    assert float((FR.mel_pre_log(x, basis).T - torch.sqrt(S.abs() ** 2 + 1e-9)).abs().max()) < 1e-10


@pytest.mark.parametrize("T", (1, 2, 3, 4, 5, 12))
def test_inverse_of_forward_returns_the_signal(T):
    x = FR.make_noise(256 * T, 7 + T).double()
    y = VR.inverse(VR.forward(x))
    env = VR.envelope(T)[: 256 * T]
    ok = env >= VR.ENV_FLOOR
    assert y.shape == x.shape and int(ok.sum()) == 256 * T - 195  # w^2 < 0.1 on the first 195 samples: about 8 ms
    assert float((y - x)[ok].abs().max()) < 1e-12
    # below the floor the signal is scaled by env / floor: the fade-in at the start
    assert float((y - x * env / VR.ENV_FLOOR)[~ok].abs().max()) < 1e-12
    if T >= 4:
        assert float((env[768: 256 * T] - 1.5).abs().max()) < 1e-12


def test_spectral_convergence_falls():
    from valle_amd.fbank import slaney_mel_basis, slaney_mel_basis_f64

    x = VR.test_signal(40)
    logmel = FR.fbank_definition(x, slaney_mel_basis()).float()
    assert logmel.shape == (40, 100)
    P = torch.from_numpy(VR.mel_inverse(slaney_mel_basis_f64(24000, 1024, 100, 0.0, 12000.0)).astype(np.float32))
    mag = VR.magnitude(logmel, P)
    assert mag.shape == (40, 513) and bool((mag >= 0).all())
    y0, ang0, _ = VR.griffinlim(mag, 0)
    y32, ang32, _ = VR.griffinlim(mag, 32)
    sc0, sc32 = VR.spectral_convergence(y0, mag), VR.spectral_convergence(y32, mag)
    print(f"spectral convergence fp64: {sc0:.4f} at 0 iterations, {sc32:.4f} at 32")
    assert y32.shape == (256 * 40,) and sc32 < sc0
    assert float((ang32.abs() - 1).abs().max()) < 1e-9 and bool((ang0 == 1).all())


# ---- 4. the Python surface ----------------------------------------------------------------------------------------------------
def test_python_surface():
    import valle_amd
    from valle_amd.engine import VxError
    from valle_amd.fbank import BigVGANFbankConfig
    from valle_amd.models import Transformer
    from valle_amd.vocoder import GriffinLim, mel_to_waveform

    for n in ("GriffinLim", "mel_to_waveform"):
        assert n in valle_amd.__all__ and callable(getattr(valle_amd, n))
    assert callable(Transformer.inference_waveform)
    gl = GriffinLim()
    assert tuple(gl.inverse.shape) == (513, 100)
    mel = torch.zeros(4, 100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gl(mel)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gl.synthesize_batch([mel])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mel_to_waveform(mel)
    with pytest.raises(ValueError):
        GriffinLim(mel_basis=torch.zeros(100, 512))
    with pytest.raises(ValueError):
        GriffinLim(inverse=torch.zeros(100, 513))
    with pytest.raises(VxError) as e:
        GriffinLim(BigVGANFbankConfig(num_mel_bins=200))
    assert e.value.code == 5
    with pytest.raises(VxError) as e:
        GriffinLim(mel_basis=torch.zeros(100, 513))  # no Cholesky factor
    assert e.value.code == 5
    small = GriffinLim(BigVGANFbankConfig(num_mel_bins=37, low_freq=50.0, high_freq=11000.0))
    assert tuple(small.inverse.shape) == (513, 37)
    h = gl._h
    assert gl.to("cuda:0")._h is h          # never used: nothing is bound yet
    gl._bound = torch.device("cuda", 0)     # as after a call on cuda:0
    assert gl.to("cuda:1")._h is None and gl._bound is None
    gl.close()
    small.close()


def test_save_writes_24_khz_pcm(tmp_path):
    from valle_amd.codec import load_wav
    from valle_amd.vocoder import GriffinLim

    wav = torch.linspace(-0.5, 0.5, 512)
    path = str(tmp_path / "v.wav")
    GriffinLim.save(path, wav)
    back, sr = load_wav(path)
    assert sr == 24000 and tuple(back.shape) == (1, 512) and float((back[0] - wav).abs().max()) <= 2.0 ** -15
