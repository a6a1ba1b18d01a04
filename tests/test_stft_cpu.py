"""No GPU: the restatement of the multi-resolution STFT distance (tests/stft_ref.py), the host side of the C ABI (vx_stft_*) and
the Python surface of valle_amd.stft.

* the torch form and the loop form of the reference agree in fp64, at the shortest length served, one hop above it and with a
  window at an odd offset; known answers (identity, silence, a scaled copy);
* vx_stft_create / vx_stft_compare / vx_stft_magnitude refuse what the header says they refuse, in its order, without any HIP
  call: 1024 samples are refused, 1025 pass every check up to the point where a device is needed;
* STFTConfig, MultiResolutionSTFT, MSTFTResult, mstft_distance, copy_synthesis_distance: the exports, no CPU fallback, the figures
  from the sums."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import stft_ref as SR
from conftest import ROOT

DEV = "cuda" if torch.cuda.is_available() else "cpu"  # without a GPU the pointers are never dereferenced


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


# ---- 1. the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,L", [((2048, 240, 1200), 1025), ((2048, 240, 1200), 1025 + 240), ((1024, 120, 600), 1025),
                                   ((512, 50, 240), 1025 + 50), (SR.ODD, 1025), (SR.ODD, 257)])
def test_torch_and_loop_forms_agree(res, L):
    """To 1e-12 of the largest magnitude: both are fp64, one an FFT and one a matrix product with tables of its own."""
    x = SR.make_noise(L, 11 + L, 0.5)
    a, b = SR.magnitude(x, res).numpy(), SR.magnitude_loops(x.numpy(), res)
    assert a.shape == b.shape == (SR.n_frames(L, res), res[0] // 2 + 1)
    assert float(np.abs(a - b).max()) <= 1e-12 * float(a.max())


def test_frames_and_shortest_length():
    assert [SR.n_frames(1025, r) for r in SR.RESOLUTIONS] == [9, 5, 21] and SR.min_samples() == 1025
    assert SR.n_frames(24000, (1024, 120, 600)) == 201 and SR.min_samples([SR.ODD]) == 257
    with pytest.raises(RuntimeError):  # torch's own reflect-padding rule: 1024 samples do not serve n_fft 2048
        SR.magnitude(torch.zeros(1024), (2048, 240, 1200))


def test_known_answers():
    x, y = SR.make_noise(3000, 1, 0.3), SR.make_noise(2900, 2, 0.3)
    sc, lm, total = SR.distance(x, x)
    assert sc == [0.0] * 3 and lm == [0.0] * 3 and total == 0.0
    sc, lm, total = SR.distance(x, y)
    sc2, lm2, _ = SR.distance(y, x)
    assert lm == lm2 and sc != sc2 and math.isclose(total, sum(a + b for a, b in zip(sc, lm)) / 3)
    # a copy at half the amplitude: |Y - X| = |Y| / 2 and ln Y - ln X = ln 2 wherever the clamp is not met
    x1 = SR.make_noise(3000, 1, 1.0)
    assert all(float(SR.power(0.5 * x1, r).min()) > SR.EPS for r in SR.RESOLUTIONS)
    sc, lm, _ = SR.distance(0.5 * x1, x1)
    assert all(math.isclose(v, 0.5, rel_tol=1e-9) for v in sc) and all(math.isclose(v, math.log(2), rel_tol=1e-9) for v in lm)
    # digital silence: every cell is the floor 1e-4
    z = torch.zeros(2000)
    assert (SR.magnitude(z, SR.RESOLUTIONS[0]) == math.sqrt(1e-8)).all() and math.isclose(math.sqrt(1e-8), 1e-4, rel_tol=1e-15)
    sc, lm, total = SR.distance(z, z)
    assert total == 0.0
    sc, lm, total = SR.distance(x, z)  # a silent target: ||Y||^2 = cells eps, finite
    assert all(math.isfinite(v) and v > 100 for v in sc) and math.isfinite(total)
    assert SR.share_near_clamp(z, SR.RESOLUTIONS[0]) == 1.0 and SR.share_near_clamp(x, SR.RESOLUTIONS[0]) == 0.0


def test_sums_by_hand():
    X, Y = np.array([[1.0, 2.0], [4.0, 1e-4]]), np.array([[2.0, 2.0], [1.0, 1e-4]])
    s = SR.sums_from_magnitudes(X, Y)
    assert s.tolist() == pytest.approx([1.0 + 9.0, 4.0 + 4.0 + 1.0 + 1e-8, math.log(2) + math.log(4), 4.0], rel=1e-15)
    sc, lm = SR.figures_from_sums(s)
    assert math.isclose(sc, math.sqrt(10 / (9 + 1e-8))) and math.isclose(lm, math.log(8) / 4)


# ---- 2. host side of the C ABI -------------------------------------------------------------------------------------------------
def _config(resolutions=SR.RESOLUTIONS, **kw):
    from valle_amd.engine import VxStftConfig

    c = VxStftConfig()
    c.struct_size = C.sizeof(VxStftConfig)
    c.sample_rate, c.n_res, c.eps, c.max_samples, c.max_batch = 24000, len(resolutions), 1e-8, 100000, 4
    for i, r in enumerate(resolutions):
        c.n_fft[i], c.hop[i], c.win[i] = r
    for k, v in kw.items():
        setattr(c, k, v)
    return c


NAMES = {"vx_stft_create", "vx_stft_destroy", "vx_stft_frames", "vx_stft_compare", "vx_stft_magnitude"}


def test_symbols_and_struct_sizes(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = set(re.findall(r"\b(vx_[a-z0-9_]+)\s*\(", hdr))
    assert NAMES <= declared and NAMES <= set(engine.declared_symbols())
    assert {n for n in declared | set(engine.declared_symbols()) if "stft" in n} == NAMES
    assert all(hasattr(lib, n) for n in NAMES)
    assert C.sizeof(engine.VxStftConfig) == 72 and engine.STFT_NSUMS == 4
    # the existing structs are as they were
    assert C.sizeof(engine.VxPitchConfig) == 28 and engine.PITCH_NSUMS == 11
    m = re.search(r"typedef struct vx_stft_config \{(.*?)\} vx_stft_config;", hdr, re.S)
    fields = re.findall(r"^\s*(?:int32_t|float)\s+(\w+)", m.group(1), re.M)
    assert fields == [f[0] for f in engine.VxStftConfig._fields_]


def test_create_refusals(lib):
    h = C.c_void_p()
    assert lib.vx_stft_create(C.byref(_config()), None) == 1
    assert lib.vx_stft_create(None, C.byref(h)) == 1

    def res(i, **kw):  # the default triple with resolution i changed
        r = [list(v) for v in SR.RESOLUTIONS]
        for k, v in kw.items():
            r[i][("n_fft", "hop", "win").index(k)] = v
        return _config([tuple(v) for v in r])

    for cfg, code in ((_config(struct_size=0), 1), (_config(struct_size=76), 1), (_config(max_batch=0), 1), (_config(max_samples=0), 1),
                      (_config(eps=0.0), 1), (_config(eps=float("nan")), 1), (_config(eps=float("inf")), 1),
                      (_config(max_batch=0, sample_rate=16000), 1),  # the argument errors come first
                      (_config(sample_rate=16000), 5), (_config(n_res=0), 5), (_config(n_res=5), 5),
                      (res(0, n_fft=256), 5), (res(1, n_fft=4096), 5), (res(2, n_fft=768), 5),
                      (res(0, win=0), 5), (res(0, win=1025), 5), (res(2, hop=0), 5), (res(2, hop=513), 5),
                      (_config(max_batch=65), 5), (_config(max_samples=1024), 5)):
        assert lib.vx_stft_create(C.byref(cfg), C.byref(h)) == code
        assert lib.vx_last_error()
    for cfg, frames in ((_config(), [9, 5, 21]), (_config([SR.ODD]), [28]), (_config([(2048, 2048, 1), (512, 1, 512)]), [1, 1026]),
                        (_config(max_batch=64, max_samples=1025), [9, 5, 21]), (_config(SR.RESOLUTIONS + (SR.ODD,)), [9, 5, 21, 28])):
        assert lib.vx_stft_create(C.byref(cfg), C.byref(h)) == 0
        assert [lib.vx_stft_frames(h, r, 1025) for r in range(cfg.n_res)] == frames
        assert lib.vx_stft_frames(h, cfg.n_res, 1025) == 0 and lib.vx_stft_frames(h, -1, 1025) == 0 and lib.vx_stft_frames(h, 0, -1) == 0
        lib.vx_stft_destroy(h)
    assert lib.vx_stft_frames(None, 0, 1025) == 0
    lib.vx_stft_destroy(None)


def test_compare_and_magnitude_refusals_before_any_hip_call(lib):
    from valle_amd.engine import VxError
    from valle_amd.stft import MultiResolutionSTFT, STFTConfig

    m = MultiResolutionSTFT(STFTConfig(max_samples=5000), max_batch=2)  # never moved to a device: no HIP call may be reached

    def code_of(fn, *args):
        with pytest.raises(VxError) as e:
            fn(*args)
        return e.value.code, str(e.value)

    sums = np.zeros(2 * 3 * 4)
    sp = sums.ctypes.data
    assert code_of(m._compare_raw, None, [2000], [8], [2000], sp)[0] == 1            # null arrays
    assert code_of(m._compare_raw, [8], [2000], None, [2000], sp)[0] == 1
    assert code_of(m._compare_raw, [8], [2000], [8], [2000], None)[0] == 1
    one, L = (C.c_void_p * 1)(8), (C.c_int32 * 1)(2000)
    assert lib.vx_stft_compare(None, 1, one, L, one, L, sp, None) == 1
    assert lib.vx_stft_compare(m._h, 1, one, None, one, L, sp, None) == 1
    assert lib.vx_stft_compare(m._h, 0, one, L, one, L, sp, None) == 1
    assert code_of(m._compare_raw, [8] * 3, [2000] * 3, [8] * 3, [2000] * 3, sp)[0] == 4  # n > max_batch
    assert code_of(m._compare_raw, [0] * 3, [0] * 3, [0] * 3, [0] * 3, sp)[0] == 4        # ... before any pair is looked at
    assert code_of(m._compare_raw, [0], [2000], [8], [2000], sp)[0] == 1             # null pointers
    assert code_of(m._compare_raw, [8], [2000], [0], [2000], sp)[0] == 1
    code, msg = code_of(m._compare_raw, [8, 8], [2000, 1024], [8, 8], [2000, 3000], sp)   # 1024 samples: refused, the pair is named
    assert code == 1 and "pair 1" in msg and "1024" in msg
    code, msg = code_of(m._compare_raw, [8, 8], [2000, 3000], [8, 8], [2000, 1024], sp)   # the common length counts
    assert code == 1 and "pair 1" in msg
    code, msg = code_of(m._compare_raw, [8, 8], [5000, 5001], [8, 8], [6000, 5001], sp)   # the common length against max_samples
    assert code == 4 and "pair 1" in msg and "5001" in msg
    assert code_of(m._compare_raw, [8, 8], [5001, 1024], [8, 8], [5001, 1024], sp)[0] == 4  # the pairs in order
    assert code_of(m._compare_raw, [8, 0], [1024, 2000], [8, 8], [2000, 2000], sp)[0] == 1
    # 1025 samples pass every check: the call gets as far as the device
    wav = torch.zeros(1025, device=DEV)
    out = torch.zeros(3 * 4, dtype=torch.float64, device=DEV)
    rc = lib.vx_stft_compare(m._h, 1, (C.c_void_p * 1)(wav.data_ptr()), (C.c_int32 * 1)(1025), (C.c_void_p * 1)(wav.data_ptr()),
                             (C.c_int32 * 1)(1025), out.data_ptr(), None)
    assert rc == (0 if DEV == "cuda" else 2), lib.vx_last_error()
    if DEV == "cuda":
        torch.cuda.synchronize()
    else:
        msg = lib.vx_last_error().decode()
        assert " failed: " in msg and "stft.hip:" in msg, msg
    # magnitude
    assert code_of(m._magnitude_raw, 0, None, [2000], [8])[0] == 1
    assert code_of(m._magnitude_raw, 0, [8], [2000], None)[0] == 1
    assert code_of(m._magnitude_raw, 3, [8], [2000], [8])[0] == 1 and code_of(m._magnitude_raw, -1, [8], [2000], [8])[0] == 1
    assert lib.vx_stft_magnitude(m._h, 0, 0, one, L, one, None) == 1
    assert code_of(m._magnitude_raw, 0, [8] * 3, [2000] * 3, [8] * 3)[0] == 4
    assert code_of(m._magnitude_raw, 0, [0], [2000], [8])[0] == 1 and code_of(m._magnitude_raw, 0, [8], [2000], [0])[0] == 1
    code, msg = code_of(m._magnitude_raw, 1, [8, 8], [2000, 1024], [8, 8])           # n_fft 2048 needs 1025
    assert code == 1 and "signal 1" in msg
    code, msg = code_of(m._magnitude_raw, 2, [8, 8], [257, 256], [8, 8])             # n_fft 512 needs 257
    assert code == 1 and "signal 1" in msg
    assert code_of(m._magnitude_raw, 0, [8], [5001], [8])[0] == 4
    if DEV == "cpu":
        assert m._bound is None
    m.close()
    assert m._h is None


def test_first_use_without_a_device_leaves_a_usable_handle(lib):
    """The pattern of test_host_cpu: VX_OK both times with a GPU, VX_ERR_HIP both times without, naming the call and stft.hip."""
    h = C.c_void_p()
    assert lib.vx_stft_create(C.byref(_config(max_batch=2)), C.byref(h)) == 0
    wav = torch.ones(1500, device=DEV)
    out = torch.zeros((SR.n_frames(1500, SR.RESOLUTIONS[0]), 513), device=DEV)
    wp, L, op = (C.c_void_p * 1)(wav.data_ptr()), (C.c_int32 * 1)(1500), (C.c_void_p * 1)(out.data_ptr())
    seen = []
    for _ in range(2):
        rc = lib.vx_stft_magnitude(h, 0, 1, wp, L, op, None)
        assert rc in (0, 2), (rc, lib.vx_last_error())
        msg = lib.vx_last_error().decode() if rc == 2 else None
        if rc == 2:
            assert "hipGetDevice" in msg and " failed: " in msg and "stft.hip:" in msg, msg
        seen.append(msg)
    assert seen[0] == seen[1]
    if DEV == "cuda":
        torch.cuda.synchronize()
    assert lib.vx_stft_magnitude(h, 0, 3, wp, L, op, None) == 4  # the host-side checks still answer
    lib.vx_stft_destroy(h)


# ---- 3. the Python surface -----------------------------------------------------------------------------------------------------
def test_object_and_exports():
    import valle_amd
    from valle_amd.engine import VxError
    from valle_amd.stft import MSTFTResult, MultiResolutionSTFT, STFTConfig, copy_synthesis_distance, mstft_distance

    for n in ("STFTConfig", "MultiResolutionSTFT", "MSTFTResult", "mstft_distance", "copy_synthesis_distance"):
        assert n in valle_amd.__all__ and callable(getattr(valle_amd, n))
    assert valle_amd.MultiResolutionSTFT is MultiResolutionSTFT and valle_amd.mstft_distance is mstft_distance
    assert valle_amd.copy_synthesis_distance is copy_synthesis_distance
    cfg = STFTConfig()
    assert cfg.resolutions == SR.RESOLUTIONS and cfg.eps == 1e-8 and cfg.sample_rate == 24000 and cfg.min_samples == 1025
    assert STFTConfig.from_dict(cfg.to_dict()) == cfg and STFTConfig(resolutions=[[512, 37, 255]]).min_samples == 257
    m = MultiResolutionSTFT()
    assert m.max_batch == 64 and m.n_res == 3 and m.n_bins == [513, 1025, 257] and m.device.type == "cpu"
    assert [m.frames(1025, r) for r in range(3)] == [9, 5, 21]
    for kw in ({"resolutions": [(256, 64, 256)]}, {"resolutions": [(512, 600, 512)]}, {"resolutions": []},
               {"resolutions": [(512, 50, 240)] * 5}, {"sample_rate": 16000}):
        with pytest.raises(VxError) as e:
            MultiResolutionSTFT(STFTConfig(**kw))
        assert e.value.code == 5
    with pytest.raises(VxError) as e:
        MultiResolutionSTFT(max_batch=65)
    assert e.value.code == 5
    with pytest.raises(VxError) as e:
        MultiResolutionSTFT(STFTConfig(eps=0.0))
    assert e.value.code == 1
    assert MSTFTResult._fields == ("sc", "log_mag", "total", "frames")
    h = m._h
    assert m.to("cuda:0")._h is h and m.to("cuda:1")._h is h     # never used: nothing is bound yet
    m._bound = torch.device("cuda", 0)
    assert m.to("cuda:1")._h is None and m._handle() is not None
    m.close()
    m.close()
    from valle_amd.codec import EncodecDecoder
    from valle_amd.meltf import Transformer

    assert callable(EncodecDecoder.roundtrip_mstft) and callable(EncodecDecoder.roundtrip_mel_distance)
    assert "copy_synthesis_distance" in Transformer.inference_waveform.__doc__


def test_no_cpu_fallback_and_short_pairs():
    from valle_amd.stft import MultiResolutionSTFT, copy_synthesis_distance, mstft_distance

    m = MultiResolutionSTFT()
    w = torch.zeros(3000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.compare(w, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.magnitude(w, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mstft_distance(w, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        copy_synthesis_distance(w, lambda mel: w)
    m.device = torch.device("cuda", 0)  # as after .to("cuda:0"): host tensors are not moved
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.compare(w, w)
    with pytest.raises(ValueError):
        m.compare_batch([], [])
    with pytest.raises(ValueError):
        m.compare_batch([w], [])
    # a too-short pair is refused before the library is called, and before the missing device is
    m.device = torch.device("cpu")
    with pytest.raises(ValueError, match="pair 1: common length 1024"):
        m.compare_batch([w, w], [w, torch.zeros(1024)])
    with pytest.raises(ValueError, match="signal 0: 1024"):
        m.magnitude(torch.zeros(1024), 1)
    with pytest.raises(ValueError):
        m.magnitude(w, 3)
    with pytest.raises(ValueError, match="1024"):
        mstft_distance(w, torch.zeros(1024))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # 1025 samples pass the check
        m.compare(torch.zeros(1025), w)
    m.close()


def test_figures_from_the_sums():
    from valle_amd.stft import result_from_sums

    x, y = SR.make_noise(3000, 5, 0.2), SR.make_noise(2800, 6, 0.4)
    rows = np.stack([SR.sums_from_magnitudes(SR.magnitude(x[:2800], r).numpy(), SR.magnitude(y, r).numpy()) for r in SR.RESOLUTIONS])
    r = result_from_sums(torch.from_numpy(rows), [513, 1025, 257])
    sc, lm, total = SR.distance(x, y)
    assert r.sc.tolist() == pytest.approx(sc, rel=1e-15) and r.log_mag.tolist() == pytest.approx(lm, rel=1e-15)
    assert math.isclose(r.total, total, rel_tol=1e-15)
    assert r.frames.tolist() == [SR.n_frames(2800, q) for q in SR.RESOLUTIONS]
