"""No GPU: the restatement of the pitch tracker (tests/pitch_ref.py), the host side of the C ABI (vx_pitch_*) and the Python
surface of valle_amd.pitch.

* known answers on the reference: a pure and a 5-harmonic tone at lags that are and are not integers, silence, white noise, a
  tone at twice fmax; the vectorised lag search against the loops; the fp32 restatement against the fp64 one on the GPU test's
  own inputs (the decided-frame rule it is held to there);
* vx_pitch_create / vx_pitch_track / vx_pitch_compare / vx_op_pitch_diff refuse what the header says they refuse, in its order,
  without any HIP call; without a device the first use fails the same way twice and the handle is destroyed cleanly;
* PitchTracker, PitchTrack, F0Result, f0_distance: the exports, no CPU fallback, the figures from the sums."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import pitch_ref as PR
from conftest import ROOT

DEV = "cuda" if torch.cuda.is_available() else "cpu"  # without a GPU the pointers are never dereferenced


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


def _inner(L, tau_max=400):
    """Frames whose 1024 samples lie inside an utterance of L samples."""
    return slice(0, (L - 1024) // PR.HOP + 1)


# ---- 1. the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_harm", (1, 5))
@pytest.mark.parametrize("f0", (240.0, 24000 / 102.87, 96.0, 24000 / 60.4, 431.7))
def test_tones_are_found_within_a_tenth_of_a_percent(f0, n_harm):
    L = 6000
    x = PR.harmonic(L, f0, n_harm, seed=int(f0))
    for dtype in (np.float64, np.float32):
        r = PR.track(x, dtype=dtype)
        s = _inner(L)
        assert r["voiced"][s].all() and s.stop >= 19
        assert float(np.abs(r["f0"][s].astype(np.float64) / f0 - 1.0).max()) < 1e-3
        assert float(r["aperiodicity"][s].max()) < 0.02
        assert np.array_equal(r["lag"][s], np.full(s.stop, int(round(24000 / f0))))


def test_silence_is_unvoiced_and_flat():
    for L in (128, 5000):
        r = PR.track(np.zeros(L, np.float32))
        assert r["dp"].shape == (PR.num_frames(L), 401) and (r["dp"] == 1.0).all()
        assert not r["voiced"].any() and (r["f0"] == 0).all() and (r["lag"] == 40).all() and (r["aperiodicity"] == 1.0).all()
    assert PR.track(np.zeros(127, np.float32))["f0"].shape == (0,) and PR.num_frames(127) == 0 and PR.num_frames(128) == 1


def test_white_noise_is_unvoiced():
    x = (0.1 * np.random.default_rng(0).standard_normal(12000)).astype(np.float32)
    r = PR.track(x)
    s = _inner(12000)
    assert not r["voiced"][s].any() and (r["f0"][s] == 0).all()
    assert float(r["aperiodicity"][s].min()) > 0.5 and ((r["lag"] >= 40) & (r["lag"] <= 400)).all()


def test_a_tone_at_twice_fmax_is_reported_an_octave_down():
    """1200 Hz with the band ending at 600: the period of 20 samples is below tau_min = 40, and the first lag of the range is
    two periods.  YIN has no way to know: the frame is voiced at fmax."""
    x = PR.harmonic(6000, 1200.0, 1, seed=1)
    r = PR.track(x)
    s = _inner(6000)
    assert r["voiced"][s].all() and (r["lag"][s] == 40).all()
    assert float(np.abs(r["f0"][s] / 600.0 - 1.0).max()) < 1e-3
    r = PR.track(x, fmin=47.0, fmax=2000.0)  # with the period in the band it is found; the offset is clamped to half a lag
    assert r["voiced"][s].all() and (r["lag"][s] == 20).all() and float(np.abs(1200.0 / r["f0"][s] - 1.0).max()) <= 0.5 / 20


def test_lag_range_and_frames():
    assert PR.lag_range(60, 600) == (40, 400) and PR.lag_range(47, 2000) == (12, 511) and PR.lag_range(46.875, 2000) == (12, 512)
    assert [PR.num_frames(L) for L in (0, 127, 128, 383, 384, 24000)] == [0, 0, 1, 1, 2, 94]


def test_vectorised_search_equals_the_loops():
    g = np.random.default_rng(3)
    for L, band in ((9000, (60, 600)), (5000, (47, 2000))):
        tmin, tmax = PR.lag_range(*band)
        for dp in (PR.cmnd(PR.make_signal(L, 7), *band), PR.cmnd(PR.make_signal(L, 8), *band, dtype=np.float32),
                   g.random((12, tmax + 1)) * 0.3, np.ones((3, tmax + 1)), np.round(g.random((12, tmax + 1)), 1)):
            for thr in (0.1, 0.35):
                l0, v0, m0 = PR.pick(dp, tmin, tmax, thr)
                l1, v1, m1 = PR.pick_loops(dp, tmin, tmax, thr)
                assert np.array_equal(l0, l1) and np.array_equal(v0, v1) and np.array_equal(m0, m1)
    # by hand: threshold hit at 41, descent to 43; no hit, first of two equal minima
    dp = np.ones((2, 401))
    dp[0, 41:46] = [0.09, 0.05, 0.02, 0.03, 0.01]
    dp[1, 100], dp[1, 200] = 0.5, 0.5
    lag, voiced, margin = PR.pick(dp, 40, 400, 0.1)
    assert lag.tolist() == [43, 100] and voiced.tolist() == [True, False]
    assert math.isclose(margin[0], 0.01) and margin[1] == 0.0


def test_refinement():
    dp = np.ones((3, 401))
    dp[0, 99:102] = [0.04, 0.02, 0.03]    # den = 0.03, offset = 0.01 / 0.06
    dp[1, 399:401] = [0.5, 0.01]          # tau* = tau_max: no neighbour, no offset
    dp[2, 50] = 0.05
    dp[2, 49], dp[2, 51] = 0.05, 0.05     # den = 0: no offset
    f0, ap = PR.refine(dp, np.array([100, 400, 50]), np.array([True, True, False]), 400)
    assert math.isclose(f0[0], 24000 / (100 + 1 / 6)) and f0[1] == 60.0 and f0[2] == 0.0 and ap.tolist() == [0.02, 0.01, 0.05]


@pytest.mark.parametrize("band", PR.BANDS)
@pytest.mark.parametrize("L", PR.LENGTHS)
def test_fp32_restatement_meets_the_rule_the_kernel_is_held_to(L, band):
    """On the GPU test's inputs: lag and voiced of the fp32 restatement equal fp64 on every decided frame, at most 5 % of the
    frames (one below 20 frames) are undecided, and on decided voiced frames its f0 is within the rule of itself."""
    x = PR.make_signal(L, PR.SEEDS[L])
    r64, r32 = PR.track(x, *band), PR.track(x, *band, dtype=np.float32)
    T = PR.num_frames(L)
    assert r64["dp"].shape == (T, PR.lag_range(*band)[1] + 1) and r32["dp"].dtype == np.float32
    if T == 0:
        return
    floor = float(np.abs(r32["dp"].astype(np.float64) - r64["dp"]).max())
    decided = r64["margin"] > PR.TOL_FACTOR * floor
    assert 0 < floor < 5e-5
    assert int((~decided).sum()) <= PR.undecided_allowed(T), (int((~decided).sum()), T)
    assert np.array_equal(r32["lag"][decided], r64["lag"][decided]) and np.array_equal(r32["voiced"][decided], r64["voiced"][decided])
    if L >= 24000:  # the three segments are there
        n = PR.segments(L).stop
        assert r64["voiced"][:n].all() and not r64["voiced"][n + 6:].any()


def test_compare_sums_by_hand():
    fa = np.array([100.0, 0.0, 200.0, 400.0], np.float32)
    fb = np.array([200.0, 50.0, 0.0], np.float32)
    s = PR.compare_sums(fa, fb, [(0, 0), (1, 0), (2, 1), (3, 1), (3, 2), (9, -4)])  # the last cell is clamped to (3, 0)
    assert s[:3].tolist() == [6, 4, 2]  # voiced in both: (0, 0), (2, 1), (3, 1), (3, 0)
    c = [-1200.0, 2400.0, 3600.0, 1200.0]
    ln = math.log
    assert math.isclose(s[3], sum(c)) and math.isclose(s[4], sum(v * v for v in c))
    assert math.isclose(s[5], 100.0 ** 2 + 150.0 ** 2 + 350.0 ** 2 + 200.0 ** 2)
    assert math.isclose(s[6], ln(100) + ln(200) + 2 * ln(400)) and math.isclose(s[7], 2 * ln(200) + 2 * ln(50))
    assert math.isclose(s[10], ln(100) * ln(200) + ln(200) * ln(50) + ln(400) * ln(50) + ln(400) * ln(200))


# ---- 2. host side of the C ABI -------------------------------------------------------------------------------------------------
def _config(**kw):
    from valle_amd.engine import VxPitchConfig

    c = VxPitchConfig()
    c.struct_size = C.sizeof(VxPitchConfig)
    c.sample_rate, c.fmin_hz, c.fmax_hz, c.threshold, c.max_frames, c.max_batch = 24000, 60.0, 600.0, 0.1, 1000, 4
    for k, v in kw.items():
        setattr(c, k, v)
    return c


NAMES = {"vx_pitch_create", "vx_pitch_destroy", "vx_pitch_lag_range", "vx_pitch_track", "vx_pitch_compare", "vx_op_pitch_diff"}


def test_symbols(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = set(re.findall(r"\b(vx_[a-z0-9_]+)\s*\(", hdr))
    assert NAMES <= declared and NAMES <= set(engine.declared_symbols())
    assert {n for n in declared | set(engine.declared_symbols()) if "pitch" in n} == NAMES
    assert all(hasattr(lib, n) for n in NAMES)
    assert C.sizeof(engine.VxPitchConfig) == 28 and engine.PITCH_NSUMS == 11


def test_create_refusals(lib):
    h = C.c_void_p()
    assert lib.vx_pitch_create(C.byref(_config()), None) == 1
    assert lib.vx_pitch_create(None, C.byref(h)) == 1
    for kw, code in (({"struct_size": 0}, 1), ({"struct_size": 32}, 1), ({"max_batch": 0}, 1), ({"max_frames": 0}, 1),
                     ({"threshold": 0.0}, 1), ({"threshold": float("nan")}, 1), ({"threshold": float("inf")}, 1),
                     ({"max_batch": 0, "sample_rate": 16000}, 1),  # the argument errors come first
                     ({"sample_rate": 16000}, 5), ({"sample_rate": 48000}, 5),
                     ({"fmin_hz": 46.8}, 5),                     # tau_max = 513
                     ({"fmax_hz": 2000.5}, 5),                   # tau_min = 11
                     ({"fmin_hz": 0.0}, 5), ({"fmin_hz": -60.0}, 5), ({"fmax_hz": float("nan")}, 5), ({"fmin_hz": float("inf")}, 5),
                     ({"fmin_hz": 600.0, "fmax_hz": 600.0}, 5),  # tau_min = tau_max
                     ({"fmin_hz": 700.0, "fmax_hz": 600.0}, 5),
                     ({"max_batch": 65}, 5)):
        assert lib.vx_pitch_create(C.byref(_config(**kw)), C.byref(h)) == code, kw
        assert lib.vx_last_error()
    lo, hi = C.c_int32(), C.c_int32()
    for kw, rng in (({}, (40, 400)), ({"fmin_hz": 47.0, "fmax_hz": 2000.0}, (12, 511)), ({"fmin_hz": 46.875}, (40, 512)),
                    ({"fmin_hz": 599.0}, (40, 41)), ({"max_batch": 64, "max_frames": 1}, (40, 400))):
        assert lib.vx_pitch_create(C.byref(_config(**kw)), C.byref(h)) == 0, kw
        assert lib.vx_pitch_lag_range(h, C.byref(lo), C.byref(hi)) == 0 and (lo.value, hi.value) == rng == PR.lag_range(
            kw.get("fmin_hz", 60.0), kw.get("fmax_hz", 600.0))
        assert lib.vx_pitch_lag_range(h, None, C.byref(hi)) == 1
        lib.vx_pitch_destroy(h)
    assert lib.vx_pitch_lag_range(None, C.byref(lo), C.byref(hi)) == 1
    lib.vx_pitch_destroy(None)


def test_track_and_compare_refusals_before_any_hip_call(lib):
    from valle_amd.engine import VxError
    from valle_amd.pitch import PitchTracker

    tr = PitchTracker(max_frames=10, max_batch=2)  # never moved to a device: no HIP call may be reached

    def code_of(fn, *args):
        with pytest.raises(VxError) as e:
            fn(*args)
        return e.value.code, str(e.value)

    assert code_of(tr._track_raw, None, [300])[0] == 1                    # null arrays
    assert lib.vx_pitch_track(tr._h, 1, (C.c_void_p * 1)(8), None, None, None, None, None, None) == 1
    assert lib.vx_pitch_track(None, 1, (C.c_void_p * 1)(8), (C.c_int32 * 1)(300), None, None, None, None, None) == 1
    assert lib.vx_pitch_track(tr._h, 0, (C.c_void_p * 1)(8), (C.c_int32 * 1)(300), None, None, None, None, None) == 1
    assert code_of(tr._track_raw, [8] * 3, [300] * 3)[0] == 4             # n > max_batch
    assert code_of(tr._track_raw, [0] * 3, [-1] * 3)[0] == 4              # ... before any utterance is looked at
    assert code_of(tr._track_raw, [0], [300])[0] == 1                     # null input
    assert code_of(tr._track_raw, [8], [-1])[0] == 1                      # a negative length
    code, msg = code_of(tr._track_raw, [8, 8], [300, 2688])               # 11 frames > max_frames: the utterance is named
    assert code == 4 and "utterance 1" in msg and "11 frames" in msg
    assert code_of(tr._track_raw, [8, 8], [2688, -1])[0] == 4             # the utterances in order
    assert code_of(tr._track_raw, [8, 0], [-1, 300])[0] == 1
    tr._track_raw([8, 8], [0, 127])                                       # no frame anywhere: nothing to do, no HIP call
    # compare
    sums = np.zeros(22)
    ok = dict(a=[8], Ta=[5], b=[8], Tb=[4], p=[8], pl=[6])

    def cmp_code(**kw):
        a = {**ok, **kw}
        return code_of(tr._compare_raw, a["a"], a["Ta"], a["b"], a["Tb"], a["p"], a["pl"], a.get("sums", sums.ctypes.data))

    assert cmp_code(sums=None)[0] == 1
    assert cmp_code(a=[8] * 3, Ta=[0] * 3, b=[8] * 3, Tb=[4] * 3, p=[8] * 3, pl=[6] * 3)[0] == 4  # n > max_batch first
    assert cmp_code(a=[0])[0] == 1 and cmp_code(b=[0])[0] == 1 and cmp_code(p=[0])[0] == 1
    assert cmp_code(Ta=[0])[0] == 1 and cmp_code(Tb=[-3])[0] == 1 and cmp_code(pl=[0])[0] == 1
    code, msg = cmp_code(a=[8, 8], Ta=[5, 11], b=[8, 8], Tb=[4, 4], p=[8, 8], pl=[6, 6])
    assert code == 4 and "pair 1" in msg
    code, msg = cmp_code(pl=[9])                                           # longer than any warp path of 5 x 4
    assert code == 4 and "pair 0" in msg
    assert cmp_code(a=[8, 0], Ta=[11, 5], b=[8, 8], Tb=[4, 4], p=[8, 8], pl=[6, 6])[0] == 4  # the pairs in order
    assert lib.vx_pitch_compare(tr._h, 0, None, None, None, None, None, None, None, None) == 1
    assert lib.vx_pitch_compare(None, 1, None, None, None, None, None, None, None, None) == 1
    assert tr._h is not None and tr._bound is None
    tr.close()
    assert tr._h is None
    # the test entry
    assert lib.vx_op_pitch_diff(60.0, 600.0, None, 300, 8, None) == 1 and lib.vx_op_pitch_diff(60.0, 600.0, 8, 300, None, None) == 1
    assert lib.vx_op_pitch_diff(60.0, 600.0, 8, -1, 8, None) == 1 and lib.vx_op_pitch_diff(40.0, 600.0, 8, 300, 8, None) == 1
    assert lib.vx_op_pitch_diff(60.0, 600.0, 8, 100, 8, None) == 0        # no frame: nothing to do


def test_first_use_without_a_device_leaves_a_usable_handle(lib):
    """The pattern of test_host_cpu: VX_OK both times with a GPU, VX_ERR_HIP both times without, naming the call and pitch.hip."""
    def twice(call, hip_call):
        seen = []
        for _ in range(2):
            rc = call()
            assert rc in (0, 2), (rc, lib.vx_last_error())
            msg = lib.vx_last_error().decode() if rc == 2 else None
            if rc == 2:
                assert hip_call in msg and " failed: " in msg and "pitch.hip:" in msg, msg
            seen.append(msg)
        assert seen[0] == seen[1]
        if DEV == "cuda":
            torch.cuda.synchronize()

    h = C.c_void_p()
    assert lib.vx_pitch_create(C.byref(_config(max_batch=2)), C.byref(h)) == 0
    wav = torch.ones(600, device=DEV)
    f0, lag = torch.zeros(2, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    wp, L = (C.c_void_p * 1)(wav.data_ptr()), (C.c_int32 * 1)(600)
    fp, lp = (C.c_void_p * 1)(f0.data_ptr()), (C.c_void_p * 1)(lag.data_ptr())
    twice(lambda: lib.vx_pitch_track(h, 1, wp, L, fp, None, lp, None, None), "hipGetDevice")
    path = torch.zeros((3, 2), dtype=torch.int32, device=DEV)
    sums = torch.zeros(11, dtype=torch.float64, device=DEV)
    pp, two, three = (C.c_void_p * 1)(path.data_ptr()), (C.c_int32 * 1)(2), (C.c_int32 * 1)(3)
    twice(lambda: lib.vx_pitch_compare(h, 1, fp, two, fp, two, pp, three, sums.data_ptr(), None), "hipGetDevice")
    assert lib.vx_pitch_track(h, 3, wp, L, fp, None, lp, None, None) == 4  # the host-side checks still answer
    lib.vx_pitch_destroy(h)
    dp = torch.zeros((2, 401), device=DEV)
    twice(lambda: lib.vx_op_pitch_diff(60.0, 600.0, wav.data_ptr(), 600, dp.data_ptr(), None), "hipMalloc")


# ---- 3. the Python surface -----------------------------------------------------------------------------------------------------
def test_object_and_exports():
    import valle_amd
    from valle_amd.engine import VxError
    from valle_amd.pitch import F0Result, PitchTrack, PitchTracker, f0_distance, num_frames

    for n in ("PitchTracker", "PitchTrack", "F0Result", "f0_distance"):
        assert n in valle_amd.__all__ and callable(getattr(valle_amd, n))
    assert valle_amd.PitchTracker is PitchTracker and valle_amd.f0_distance is f0_distance
    t = PitchTracker()
    assert (t.fmin, t.fmax, t.threshold, t.tau_min, t.tau_max, t.max_batch) == (60.0, 600.0, 0.1, 40, 400, 64) and t.device.type == "cpu"
    assert (PitchTracker(47, 2000).tau_min, PitchTracker(47, 2000).tau_max) == (12, 511)
    for kw in ({"fmin": 30}, {"fmax": 4000}, {"fmin": 700}, {"max_batch": 65}):
        with pytest.raises(VxError) as e:
            PitchTracker(**kw)
        assert e.value.code == 5
    with pytest.raises(VxError) as e:
        PitchTracker(threshold=0.0)
    assert e.value.code == 1
    assert PitchTrack._fields == ("f0", "aperiodicity", "lag", "voiced")
    assert [f for f in F0Result.__dataclass_fields__] == ["rmse_cents", "rmse_hz", "log_f0_corr", "vuv_error", "n_voiced", "length", "mcd_db"]
    assert [num_frames(L) for L in (127, 128, 24000)] == [0, 1, 94]
    h = t._h
    assert t.to("cuda:0")._h is h and t.to("cuda:1")._h is h     # never used: nothing is bound yet
    t._bound = torch.device("cuda", 0)
    assert t.to("cuda:1")._h is None and t._handle() is not None
    t.close()
    t.close()


def test_no_cpu_fallback():
    from valle_amd.pitch import PitchTracker, f0_distance

    t = PitchTracker()
    w = torch.zeros(1000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.track(w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.track_batch([w, w], sr=16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.compare_sums([(w, w, torch.zeros((3, 2), dtype=torch.int32))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f0_distance(w, w)
    with pytest.raises(ValueError):
        f0_distance([], [])
    with pytest.raises(ValueError):
        f0_distance([w], [])
    t.device = torch.device("cuda", 0)  # as after .to("cuda:0"): host tensors are not moved
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.track(w)
    with pytest.raises(AssertionError):
        t.track(torch.zeros(2, 1000, device="meta"))
    t.close()


def test_figures_from_the_sums():
    from valle_amd.pitch import result_from_sums

    g = np.random.default_rng(0)
    fa = (150 + 40 * g.random(50)).astype(np.float32)
    fb = (fa * 2 ** (0.5 / 12) * (1 + 0.01 * g.standard_normal(50))).astype(np.float32)
    fa[:5], fb[3:9] = 0, 0
    path = np.stack([np.arange(50)] * 2, 1)
    r = result_from_sums(PR.compare_sums(fa, fb, path), 1.5)
    both = (fa > 0) & (fb > 0)
    c = 1200 * np.log2(fa[both].astype(np.float64) / fb[both])
    assert r.length == 50 and r.n_voiced == int(both.sum()) == 41 and math.isclose(r.vuv_error, 7 / 50) and r.mcd_db == 1.5
    assert math.isclose(r.rmse_cents, math.sqrt((c * c).mean())) and 40 < r.rmse_cents < 70
    assert math.isclose(r.rmse_hz, math.sqrt(((fa[both].astype(np.float64) - fb[both]) ** 2).mean()))
    assert math.isclose(r.log_f0_corr, np.corrcoef(np.log(fa[both].astype(np.float64)), np.log(fb[both].astype(np.float64)))[0, 1], rel_tol=1e-9)
    one = result_from_sums(PR.compare_sums(fa[10:11], fb[10:11], [(0, 0)]))
    assert one.n_voiced == 1 and math.isnan(one.log_f0_corr) and not math.isnan(one.rmse_cents) and math.isnan(one.mcd_db)
    flat = result_from_sums(PR.compare_sums(np.full(8, 200, np.float32), fb[10:18], path[:8]))
    assert math.isnan(flat.log_f0_corr)  # no variance in one of the two
    none = result_from_sums(PR.compare_sums(fa[:5], fb[:5], path[:5]))
    assert none.n_voiced == 0 and math.isnan(none.rmse_cents) and math.isnan(none.rmse_hz) and none.vuv_error == 3 / 5
