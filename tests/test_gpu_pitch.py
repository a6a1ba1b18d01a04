"""GPU: the pitch tracker (pitch_kernels.hpp behind vx_pitch_*, valle_amd.pitch) against the restatement of tests/pitch_ref.py.

The inputs are pitch_ref.LENGTHS x pitch_ref.BANDS on pitch_ref.make_signal (a vibrato'd harmonic segment, a silent one, a
noise-only one, a 1e-3 noise floor); the references are computed once per (length, band) and shared.

1. d' (vx_op_pitch_diff) against fp64.  Floor: the fp32 restatement's largest error on the same utterance.  Bound: engine error
   <= 4 x floor (pitch_ref.TOL_FACTOR, the project's rule); every ratio is printed before it is asserted.
   Measured: ratios 0.66 .. 1.79.
2. decisions (PitchTracker.track): lag and voiced equal fp64 on every decided frame (margin > 4 x floor); at most 5 % of an
   utterance's frames are undecided (one below 20 frames); aperiodicity is d' at the lag; on decided voiced frames
   |f0 - f0_ref64| <= 4 x the fp32 restatement's largest f0 error there.  Exact silence: d' = 1, unvoiced, lag = tau_min.
3. a ragged batch of 5 lengths equals each utterance alone bitwise, in two orders, with inputs one float past a 16-byte boundary
   in NaN-filled buffers and outputs inside canary-filled ones; the canaries stay.
4. vx_pitch_compare on hand-built tracks and paths against numpy fp64 to 1e-12 relative; f0_distance: w against itself, against
   a copy shifted by 100 cents through resampling, against a time-stretched copy (syllables repeated)."""
import math

import numpy as np
import pytest
import torch

import pitch_ref as PR
from valle_amd import engine as E
from valle_amd.pitch import PitchTracker, f0_distance, result_from_sums

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CACHE = {}


def _build():
    import __graft_entry__ as ge

    ge.build()


def _tracker(band=PR.BANDS[0]):
    _build()
    if ("tracker", band) not in _CACHE:
        _CACHE[("tracker", band)] = PitchTracker(band[0], band[1], max_batch=8).to(DEV)
    return _CACHE[("tracker", band)]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ref(L, band):
    """(signal, fp64 track, fp32 track, floor of d'), computed once."""
    if ("ref", L, band) not in _CACHE:
        x = PR.make_signal(L, PR.SEEDS[L])
        r64, r32 = PR.track(x, *band), PR.track(x, *band, dtype=np.float32)
        floor = float(np.abs(r32["dp"].astype(np.float64) - r64["dp"]).max()) if r64["dp"].size else 0.0
        _CACHE[("ref", L, band)] = (x, r64, r32, floor)
    return _CACHE[("ref", L, band)]


# ---- 1. d' -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", PR.BANDS)
@pytest.mark.parametrize("L", PR.LENGTHS)
def test_dprime_against_fp64(L, band):
    _build()
    x, r64, _, floor = _ref(L, band)
    tau_max = PR.lag_range(*band)[1]
    got = E.op_pitch_diff(_dev(x), band[0], band[1], tau_max).cpu().numpy()
    assert got.shape == r64["dp"].shape == (PR.num_frames(L), tau_max + 1)
    if got.size == 0:
        return
    err = float(np.abs(got.astype(np.float64) - r64["dp"]).max())
    print(f"d' L={L} band={band}: engine {err:.3e}, floor {floor:.3e}, ratio {err / floor:.2f}")
    assert np.isfinite(got).all() and (got[:, 0] == 1.0).all()
    assert err <= PR.tolerance(floor), f"L={L} band={band}: engine {err:.3e} > {PR.TOL_FACTOR} x floor {floor:.3e}"


# ---- 2. decisions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", PR.BANDS)
@pytest.mark.parametrize("L", PR.LENGTHS)
def test_decisions_against_fp64(L, band):
    x, r64, r32, floor = _ref(L, band)
    tr = _tracker(band).track(_dev(x))
    T = PR.num_frames(L)
    assert tr.f0.shape == tr.aperiodicity.shape == tr.lag.shape == tr.voiced.shape == (T,)
    assert (tr.f0.dtype, tr.aperiodicity.dtype, tr.lag.dtype, tr.voiced.dtype) == (torch.float32, torch.float32, torch.int32, torch.bool)
    if T == 0:
        return
    f0, ap, lag, voiced = (t.cpu().numpy() for t in tr)
    tau_min, tau_max = PR.lag_range(*band)
    decided = r64["margin"] > PR.TOL_FACTOR * floor
    und = int((~decided).sum())
    wrong = int(((lag != r64["lag"]) | (voiced != r64["voiced"]))[decided].sum())
    print(f"decisions L={L} band={band}: {T} frames, {und} undecided (allowed {PR.undecided_allowed(T)}), {wrong} decided frames differ, "
          f"{int(voiced.sum())} voiced")
    assert und <= PR.undecided_allowed(T)
    assert wrong == 0
    assert ((lag >= tau_min) & (lag <= tau_max)).all() and ((f0 > 0) == voiced).all()
    dp = E.op_pitch_diff(_dev(x), band[0], band[1], tau_max).cpu().numpy()
    assert np.array_equal(ap, dp[np.arange(T), lag])  # the launch that tracks and the one that shows d' agree bit for bit
    assert float(np.abs(ap.astype(np.float64) - r64["dp"][np.arange(T), lag])[decided].max(initial=0.0)) <= PR.tolerance(floor)
    dv = decided & r64["voiced"]
    if dv.any():
        f0_floor = float(np.abs(r32["f0"].astype(np.float64) - r64["f0"])[dv].max())
        f0_err = float(np.abs(f0.astype(np.float64) - r64["f0"])[dv].max())
        print(f"f0 L={L} band={band}: engine {f0_err:.3e} Hz, floor {f0_floor:.3e} Hz, ratio {f0_err / f0_floor:.2f}")
        assert f0_err <= PR.tolerance(f0_floor)


def test_exact_silence_and_a_steady_tone():
    t = _tracker()
    tr = t.track(torch.zeros(5000, device=DEV))
    assert tr.f0.shape == (20,) and not tr.voiced.any() and (tr.f0 == 0).all() and (tr.lag == 40).all() and (tr.aperiodicity == 1).all()
    assert (E.op_pitch_diff(torch.zeros(5000, device=DEV), 60.0, 600.0, 400) == 1).all()
    tr = t.track(_dev(PR.harmonic(6000, 24000 / 102.87, 5, seed=3)))
    inner = slice(0, (6000 - 1024) // 256 + 1)
    assert tr.voiced[inner].all() and (tr.lag[inner] == 103).all()
    assert float((tr.f0[inner].double() / (24000 / 102.87) - 1).abs().max()) < 1e-3


# ---- 3. batch independence -------------------------------------------------------------------------------------------------------
def test_ragged_batch_is_bitwise_each_alone_and_keeps_the_canaries():
    band = PR.BANDS[0]
    t = _tracker(band)
    lengths = (1000, 4097, 127, 24000, 4096)
    alone = {L: [v.cpu().numpy() for v in t.track(_dev(_ref(L, band)[0]))] for L in lengths}
    PAD = 8
    for order in (lengths, lengths[::-1]):
        ins, outs = [], []
        for L in order:
            buf = torch.full((L + 2 * PAD,), float("nan"), device=DEV)  # a read past either end poisons the frame
            buf[1:1 + L] = _dev(_ref(L, band)[0])
            assert buf.data_ptr() % 16 == 0
            T = PR.num_frames(L)
            ins.append(buf)
            outs.append((torch.full((T + 2 * PAD,), -7.0, device=DEV), torch.full((T + 2 * PAD,), -7.0, device=DEV),
                         torch.full((T + 2 * PAD,), -7, dtype=torch.int32, device=DEV),
                         torch.full((T + 2 * PAD,), 77, dtype=torch.uint8, device=DEV)))
        live = list(range(len(order)))  # 127 samples included: no frame, no tile, nothing written
        with torch.cuda.device(DEV):
            t._track_raw([ins[i][1:].data_ptr() for i in live], [order[i] for i in live],
                         *[[outs[i][k][PAD:].data_ptr() for i in live] for k in range(4)])
        torch.cuda.synchronize()
        for i, L in enumerate(order):
            T = PR.num_frames(L)
            for k, canary in enumerate((-7.0, -7.0, -7, 77)):
                o = outs[i][k].cpu().numpy()
                assert (o[:PAD] == canary).all() and (o[PAD + T:] == canary).all(), f"L={L} output {k}: a canary is gone"
                want = alone[L][k].astype(o.dtype)
                assert o[PAD:PAD + T].tobytes() == want.tobytes(), f"L={L} output {k}: the batch differs from the utterance alone"
    # the public call, and the same call again
    a = t.track_batch([_dev(_ref(L, band)[0]) for L in lengths])
    b = t.track_batch([_dev(_ref(L, band)[0]) for L in lengths])
    for L, ta, tb in zip(lengths, a, b):
        for k in range(4):
            assert torch.equal(ta[k], tb[k]) and ta[k].cpu().numpy().tobytes() == alone[L][k].tobytes()


def test_null_outputs_are_skipped():
    band = PR.BANDS[0]
    t = _tracker(band)
    x = _dev(_ref(4097, band)[0])
    want = t.track(x)
    lag = torch.full((16,), -7, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        t._track_raw([x.data_ptr()], [4097], None, None, [lag.data_ptr()], None)
    assert torch.equal(lag, want.lag)


# ---- 4. the figures along a path -------------------------------------------------------------------------------------------------
def _compare_cases():
    g = np.random.default_rng(21)

    def trk(T, unvoiced):
        f = (120.0 + 80.0 * g.random(T)).astype(np.float32)
        f[unvoiced] = 0
        return f

    diag = lambda T: np.stack([np.arange(T)] * 2, 1).astype(np.int32)
    cases = []
    fa, fb = trk(40, slice(0, 0)), trk(40, slice(0, 0))
    cases.append(("all voiced", fa, (fb * 1.3).astype(np.float32), diag(40)))
    cases.append(("identical", fa, fa, diag(40)))
    cases.append(("no voiced overlap", trk(30, slice(0, 15)), trk(30, slice(15, 30)), diag(30)))
    rows = np.repeat(np.arange(20), 3)
    cases.append(("repeated rows", trk(20, slice(3, 6)), (trk(60, slice(10, 25)) * 1.2).astype(np.float32),
                  np.stack([rows, np.arange(60)], 1).astype(np.int32)))
    i = np.sort(g.integers(0, 300, 700))
    j = np.sort(g.integers(0, 500, 700))
    cases.append(("long", trk(300, slice(100, 130)), (trk(500, slice(40, 90)) * 1.1).astype(np.float32), np.stack([i, j], 1).astype(np.int32)))
    cases.append(("one cell", fa[:1], fb[:1], diag(1)))
    out = np.array([[-3, 0], [1, 1], [5, 2], [2, 99]], dtype=np.int32)  # clamped to (0, 0), (1, 1), (3, 2), (2, 3)
    cases.append(("clamped", fa[:4], (fb[:4] * 1.3).astype(np.float32), out))
    return cases


def test_compare_sums_against_numpy():
    t = _tracker()
    cases = _compare_cases()
    batch = t.compare_sums([(_dev(fa), _dev(fb), _dev(p)) for _, fa, fb, p in cases]).numpy()
    for z, (name, fa, fb, p) in enumerate(cases):
        want = PR.compare_sums(fa, fb, p)
        assert np.array_equal(batch[z, :3], want[:3]), name
        for q in range(3, 11):
            assert math.isclose(batch[z, q], want[q], rel_tol=1e-12, abs_tol=0.0), f"{name}: sum {q}: {batch[z, q]!r} != {want[q]!r}"
        alone = t.compare_sums([(_dev(fa), _dev(fb), _dev(p))]).numpy()[0]
        assert alone.tobytes() == batch[z].tobytes(), f"{name}: alone differs from the batch"
        r, w = result_from_sums(batch[z]), result_from_sums(want)
        for f in ("rmse_cents", "rmse_hz", "log_f0_corr", "vuv_error"):
            gv, wv = getattr(r, f), getattr(w, f)
            assert (math.isnan(gv) and math.isnan(wv)) or math.isclose(gv, wv, rel_tol=1e-9), (name, f)
    r = result_from_sums(batch[1])
    assert r.rmse_cents == 0 and r.rmse_hz == 0 and r.vuv_error == 0 and r.n_voiced == 40
    assert math.isnan(result_from_sums(batch[2]).rmse_cents) and result_from_sums(batch[2]).vuv_error == 1.0


def test_f0_distance():
    _build()
    w = _dev(PR.make_signal(24000, 24000))
    r = f0_distance(w, w)
    assert r.rmse_cents == 0 and r.rmse_hz == 0 and r.vuv_error == 0 and r.mcd_db == 0 and r.length == 94 and r.n_voiced >= 35
    # 100 cents up through resampling: every voiced cell is a semitone apart
    v = PR.voice(24000, 1)
    up = PR.resampled(v, 2.0 ** (1.0 / 12.0))
    r = f0_distance(_dev(up), _dev(v))
    print(f"shifted copy: rmse_cents {r.rmse_cents:.4f}, n_voiced {r.n_voiced} of {r.length}, vuv {r.vuv_error:.3f}, mcd {r.mcd_db:.2f} dB")
    assert abs(r.rmse_cents - 100.0) < 1.0 and r.n_voiced >= 80 and r.vuv_error < 0.05
    # a time-stretched copy: under the warp every voiced cell meets its own copy; frame by frame the syllables slide apart
    s = PR.syllables(8, 1)
    z = PR.stretched(s)
    rs = f0_distance([_dev(z), _dev(up)], [_dev(s), _dev(v)])
    assert repr(rs[1]) == repr(r)  # a pair in a batch is what it is alone
    tr = _tracker()
    ts, tz = tr.track(_dev(s)), tr.track(_dev(z))
    n = ts.f0.numel()
    flat = result_from_sums(tr.compare_sums([(tz.f0[:n].contiguous(), ts.f0, _dev(np.stack([np.arange(n)] * 2, 1).astype(np.int32)))])[0].tolist())
    print(f"stretched copy: rmse_cents {rs[0].rmse_cents:.4f} under the warp, {flat.rmse_cents:.1f} frame by frame")
    assert rs[0].rmse_cents < 1.0 and rs[0].n_voiced >= 50
    assert flat.rmse_cents > 100.0  # the syllables are whole tones apart
    with pytest.raises(ValueError):
        f0_distance(w[:100], w)
    # with a rate: both sides resampled once, as mel_cepstral_distortion does
    from valle_amd.dtw import mel_cepstral_distortion

    w48 = _dev(PR.make_signal(48000, 5))
    r48 = f0_distance(w48, w48[:40000], sr=48000)
    assert r48.mcd_db == mel_cepstral_distortion(w48, w48[:40000], sr=48000).mcd_db and r48.length >= 94
