"""GPU: the multi-resolution STFT distance (stft_kernels.hpp behind vx_stft_*, valle_amd.stft) against tests/stft_ref.py.

Inputs: Gaussian noise of amplitude 0.1 and 1.0 at L in {1025, 1025 + hop, 2400, 24000, 33 hop} (33 = the frames of a magnitude
tile + 1, which is also two compare tiles and a frame) at each default resolution and at (512, 37, 255); the seed is a formula of
the case (stft_ref.make_clear_noise moves on from a seed whose fp64 spectrogram has a cell near the clamp).  The references are
computed once per case and shared.

(a) magnitudes (vx_stft_magnitude, outputs pre-filled with NaN) against fp64.  First share_near_clamp == 0: no cell's power is
    within a factor 2 of eps, so the clamp decides the same in every precision.  Floor: the same formula in torch fp32 on the host
    against fp64, max |.|; bound: engine error <= 4 x floor (stft_ref.TOL_FACTOR, the project's rule), for the magnitude and, with
    a floor of its own, for its logarithm.  Every ratio is printed before it is asserted.  Measured: DESIGN.md section 7.
(b) the four sums of vx_stft_compare against numpy fp64 on the engine's own magnitudes: 1e-12 relative (both sides are fp64 on
    the same fp32 numbers: a rounding bound, not a measurement); the cell counts exactly.
(c) composition: see test_composition's docstring for the bound.
(d) digital silence.  (e) a ragged batch is bitwise every pair alone, twice.  (f) memory the call does not own.
(g) the caller's stream and the front ends: mstft_distance(sr=), copy_synthesis_distance, EncodecDecoder.roundtrip_mstft."""
import math

import numpy as np
import pytest
import torch

import stft_ref as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL_RES = SR.RESOLUTIONS + (SR.ODD,)
AMPS = (0.1, 1.0)
_CACHE = {}


def lengths(res):
    return (1025, 1025 + res[1], 2400, 24000, 33 * res[1])


def seed_of(L, res, amp):
    return L + 7 * ALL_RES.index(res) + (100003 if amp == 1.0 else 0)


CASES = [(res, L, amp) for res in ALL_RES for L in lengths(res) for amp in AMPS]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    yield
    for k in [k for k in _CACHE if k[0] == "obj"]:
        _CACHE.pop(k).close()


def _obj(key="default"):
    from valle_amd.stft import MultiResolutionSTFT, STFTConfig

    if ("obj", key) not in _CACHE:
        cfg = STFTConfig(resolutions=[SR.ODD]) if key == "odd" else STFTConfig()
        _CACHE[("obj", key)] = MultiResolutionSTFT(cfg, max_batch=8).to(DEV)
    return _CACHE[("obj", key)]


def _obj_for(res):
    """(object, index of `res` in it)."""
    return (_obj("odd"), 0) if res == SR.ODD else (_obj(), SR.RESOLUTIONS.index(res))


def _ref(res, L, amp):
    """(signal, fp64 magnitudes, floor of the magnitude, floor of its logarithm), computed once; never modified."""
    key = ("ref", res, L, amp)
    if key not in _CACHE:
        x = SR.make_clear_noise(L, seed_of(L, res, amp), amp, [res])
        m64 = SR.magnitude(x, res, torch.float64).numpy()
        m32 = SR.magnitude(x, res, torch.float32).numpy().astype(np.float64)
        _CACHE[key] = (x, m64, float(np.abs(m32 - m64).max()), float(np.abs(np.log(m32) - np.log(m64)).max()))
    return _CACHE[key]


def _magnitude_nan_prefilled(obj, ri, x):
    """One signal through vx_stft_magnitude into an output that holds NaN before the call."""
    res = obj.config.resolutions[ri]
    out = torch.full((obj.frames(x.numel(), ri), res[0] // 2 + 1), float("nan"), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        obj._magnitude_raw(ri, [x.data_ptr()], [x.numel()], [out.data_ptr()])
    return out


# ---- (a) magnitudes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,L,amp", CASES)
def test_magnitudes_against_fp64(res, L, amp):
    x, m64, floor, floor_log = _ref(res, L, amp)
    assert SR.share_near_clamp(x, res) == 0.0
    obj, ri = _obj_for(res)
    got = _magnitude_nan_prefilled(obj, ri, x.to(DEV)).cpu().numpy().astype(np.float64)
    assert got.shape == m64.shape == (SR.n_frames(L, res), res[0] // 2 + 1)
    assert np.isfinite(got).all() and (got > 0).all()
    err, err_log = float(np.abs(got - m64).max()), float(np.abs(np.log(got) - np.log(m64)).max())
    print(f"|S| {res} L={L} amp={amp}: engine {err:.3e}, floor {floor:.3e}, ratio {err / floor:.2f}; "
          f"ln: engine {err_log:.3e}, floor {floor_log:.3e}, ratio {err_log / floor_log:.2f}; min |S| {m64.min():.2e}")
    assert err <= SR.tolerance(floor), f"{res} L={L} amp={amp}: engine {err:.3e} > {SR.TOL_FACTOR} x floor {floor:.3e}"
    assert err_log <= SR.tolerance(floor_log), f"{res} L={L} amp={amp}: ln: engine {err_log:.3e} > {SR.TOL_FACTOR} x floor {floor_log:.3e}"


def test_magnitude_batch_is_each_signal_alone():
    obj = _obj()
    xs = [SR.make_noise(L, 40 + i, 0.3).to(DEV) for i, L in enumerate((1025, 4000, 1300, 9000))]
    for ri in range(3):
        both = obj.magnitude_batch(xs, ri)
        for x, m in zip(xs, both):
            assert torch.equal(m, obj.magnitude(x, ri)) and m.shape == (obj.frames(x.numel(), ri), obj.n_bins[ri])


# ---- (b) sums ------------------------------------------------------------------------------------------------------------------
PAIRS = ((1025, 1025, 1.0, 1.0), (2400, 2500, 0.1, 1.0), (8000, 7921, 1.0, 0.1), (24000, 24000, 0.5, 0.5))


def _pair(i):
    Lx, Ly, ax, ay = PAIRS[i]
    if ("pair", i) not in _CACHE:
        cut = min(Lx, Ly)
        _CACHE[("pair", i)] = (SR.make_clear_noise(Lx, 200 + i, ax, SR.RESOLUTIONS, cut), SR.make_clear_noise(Ly, 300 + i, ay, SR.RESOLUTIONS, cut))
    return _CACHE[("pair", i)]


@pytest.mark.parametrize("i", range(len(PAIRS)))
def test_sums_against_the_engines_own_magnitudes(i):
    obj = _obj()
    x, y = _pair(i)
    L = min(x.numel(), y.numel())
    sums = obj.compare_sums([x.to(DEV)], [y.to(DEV)])[0].numpy()
    assert sums.shape == (3, 4)
    for ri, res in enumerate(SR.RESOLUTIONS):
        X = obj.magnitude(x[:L].to(DEV), ri).cpu().numpy()
        Y = obj.magnitude(y[:L].to(DEV), ri).cpu().numpy()
        want = SR.sums_from_magnitudes(X, Y)
        rel = np.abs(sums[ri, :3] - want[:3]) / want[:3]
        print(f"sums pair {i} {res}: relative {rel}")
        assert sums[ri, 3] == want[3] == SR.n_frames(L, res) * (res[0] // 2 + 1)
        assert (rel <= 1e-12).all(), (res, sums[ri], want)


# ---- (c) composition -----------------------------------------------------------------------------------------------------------
def test_identity_and_symmetry():
    obj = _obj()
    x, y = (t.to(DEV) for t in _pair(1))
    r = obj.compare(x, x)
    assert (r.sc == 0).all() and (r.log_mag == 0).all() and r.total == 0.0 and r.frames.tolist() == [SR.n_frames(2400, q) for q in SR.RESOLUTIONS]
    a, b = obj.compare(x, y), obj.compare(y, x)
    assert torch.equal(a.log_mag, b.log_mag) and (a.sc != b.sc).all() and torch.equal(a.frames, b.frames)
    sums = obj.compare_sums([x], [y])[0]
    assert torch.equal(a.sc, torch.sqrt(sums[:, 0] / sums[:, 1])) and torch.equal(a.log_mag, sums[:, 2] / sums[:, 3])
    assert a.total == float((a.sc + a.log_mag).mean())


@pytest.mark.parametrize("i", range(len(PAIRS)))
def test_composition(i):
    """The end-to-end figures against the fp64 definition, within what (a) implies.  With X^, Y^ the engine's magnitudes and every
    cell of them within d_X = 4 floor_X (d_Y = 4 floor_Y) of X (Y), and every logarithm within 4 floor_log:
      lm:  |ln Y^ - ln X^| differs from |ln Y - ln X| by at most 4 floor_log_X + 4 floor_log_Y per cell, and so does the mean.
           With both floors at their larger one that is the 8 x the log floor of the rule.
      sc:  ||Y^ - X^|| differs from ||Y - X|| by at most ||dX|| + ||dY||, and 1 / ||Y^|| from 1 / ||Y|| by ||dY|| / (||Y|| ||Y^||);
           to first order |sc^ - sc| <= (||dX|| + (1 + sc) ||dY||) / ||Y||, with ||d|| <= 4 floor sqrt(cells).
    The floors are those of this pair's own signals (torch fp32 on the host against fp64)."""
    obj = _obj()
    x, y = _pair(i)
    L = min(x.numel(), y.numel())
    got = obj.compare(x.to(DEV), y.to(DEV))
    sc, lm, total = SR.distance(x, y)
    tol_total = 0.0
    for ri, res in enumerate(SR.RESOLUTIONS):
        X64, Y64 = SR.magnitude(x[:L], res).numpy(), SR.magnitude(y[:L], res).numpy()
        X32, Y32 = SR.magnitude(x[:L], res, torch.float32).numpy().astype(np.float64), SR.magnitude(y[:L], res, torch.float32).numpy().astype(np.float64)
        assert SR.share_near_clamp(x[:L], res) == 0.0 and SR.share_near_clamp(y[:L], res) == 0.0
        fx, fy = float(np.abs(X32 - X64).max()), float(np.abs(Y32 - Y64).max())
        flog = max(float(np.abs(np.log(X32) - np.log(X64)).max()), float(np.abs(np.log(Y32) - np.log(Y64)).max()))
        root = math.sqrt(X64.size)
        tol_lm = 8 * flog
        tol_sc = (SR.TOL_FACTOR * fx * root + (1 + sc[ri]) * SR.TOL_FACTOR * fy * root) / float(np.sqrt((Y64 * Y64).sum()))
        d_sc, d_lm = abs(float(got.sc[ri]) - sc[ri]), abs(float(got.log_mag[ri]) - lm[ri])
        print(f"pair {i} {res}: sc {sc[ri]:.6f} d {d_sc:.2e} (bound {tol_sc:.2e}); lm {lm[ri]:.6f} d {d_lm:.2e} (bound {tol_lm:.2e})")
        assert d_sc <= tol_sc and d_lm <= tol_lm
        tol_total += (tol_sc + tol_lm) / 3
    assert abs(got.total - total) <= tol_total


# ---- (d) digital silence -------------------------------------------------------------------------------------------------------
def test_digital_silence():
    obj = _obj()
    z = torch.zeros(3000, device=DEV)
    x = SR.make_noise(3100, 9, 0.2).to(DEV)
    floor = np.sqrt(np.float32(1e-8))
    assert floor.dtype == np.float32 and math.isclose(float(floor), 1e-4, rel_tol=1e-6)
    for ri in range(3):
        m = _magnitude_nan_prefilled(obj, ri, z)
        assert (m.cpu().numpy() == floor).all()
    r = obj.compare(z, z)
    assert (r.sc == 0).all() and (r.log_mag == 0).all() and r.total == 0.0
    r = obj.compare(x, z)  # a silent target: ||Y||^2 = cells eps
    assert torch.isfinite(r.sc).all() and torch.isfinite(r.log_mag).all() and math.isfinite(r.total) and (r.sc > 100).all()
    s = obj.compare_sums([x], [z])[0]
    eps = float(np.float32(1e-8))
    assert torch.allclose(s[:, 1], s[:, 3] * float(floor) ** 2, rtol=1e-12, atol=0) and math.isclose(float(floor) ** 2, eps, rel_tol=1e-6)
    r = obj.compare(z, x)
    assert torch.isfinite(r.sc).all() and torch.isfinite(r.log_mag).all()


# ---- (e) ragged batch ----------------------------------------------------------------------------------------------------------
COMMON = (1025, 1026, 2400, 4801, 72001)
EXTRA = ((0, 300), (77, 0), (0, 0), (1, 5000), (129, 0))  # samples of pred / target past the common length


def _off_by_one_float(x, tail=64):
    """x inside a NaN-filled buffer, one float past its (at least 16-byte aligned) start."""
    buf = torch.full((x.numel() + 1 + tail,), float("nan"), dtype=torch.float32, device=DEV)
    buf[1:1 + x.numel()] = x.to(DEV)
    v = buf[1:1 + x.numel()]
    assert v.data_ptr() % 16 == 4
    return v


def test_ragged_batch_is_every_pair_alone():
    obj = _obj()
    xs, ys = [], []
    for i, (L, (ex, ey)) in enumerate(zip(COMMON, EXTRA)):
        xs.append(_off_by_one_float(SR.make_noise(L + ex, 500 + i, 0.3)))
        ys.append(_off_by_one_float(SR.make_noise(L + ey, 600 + i, 0.5)))
    batch = obj.compare_sums(xs, ys)
    again = obj.compare_sums(xs, ys)
    assert batch.shape == (5, 3, 4) and torch.equal(batch, again) and torch.isfinite(batch).all()
    for i in range(5):
        assert torch.equal(obj.compare_sums([xs[i]], [ys[i]])[0], batch[i]), i
        assert batch[i, :, 3].tolist() == [SR.n_frames(COMMON[i], r) * (r[0] // 2 + 1) for r in SR.RESOLUTIONS]
    order = [4, 2, 0, 3, 1]
    perm = obj.compare_sums([xs[i] for i in order], [ys[i] for i in order])
    assert torch.equal(perm, batch[order])


# ---- (f) memory the call does not own ------------------------------------------------------------------------------------------
def test_guards_and_samples_past_the_common_length():
    obj = _obj()
    x, y = SR.make_noise(2600, 21, 0.4), SR.make_noise(3900, 22, 0.4)
    clean = obj.compare_sums([x.to(DEV)], [y.to(DEV)])
    assert torch.equal(obj.compare_sums([x.to(DEV)], [y[:2600].to(DEV)]), clean)
    ynan = y.clone()
    ynan[2600:] = float("nan")  # past the common length of the longer signal: never read into the result
    assert torch.equal(obj.compare_sums([x.to(DEV)], [ynan.to(DEV)]), clean)
    assert torch.equal(obj.compare_sums([_off_by_one_float(x)], [_off_by_one_float(y[:2600])]), clean)  # NaN right behind both
    # sums inside a NaN-filled block
    G = 16
    block = torch.full((G + 12 + G,), float("nan"), dtype=torch.float64, device=DEV)
    xd, yd = x.to(DEV), y.to(DEV)
    with torch.cuda.device(DEV):
        obj._compare_raw([xd.data_ptr()], [2600], [yd.data_ptr()], [3900], block.data_ptr() + 8 * G)
    torch.cuda.synchronize()
    assert torch.isnan(block[:G]).all() and torch.isnan(block[G + 12:]).all() and torch.equal(block[G:G + 12].cpu().reshape(1, 3, 4), clean)
    # ... and in host memory
    host = np.full(G + 12 + G, np.nan)
    with torch.cuda.device(DEV):
        obj._compare_raw([xd.data_ptr()], [2600], [yd.data_ptr()], [3900], host.ctypes.data + 8 * G)
    torch.cuda.synchronize()
    assert np.isnan(host[:G]).all() and np.isnan(host[G + 12:]).all() and np.array_equal(host[G:G + 12].reshape(1, 3, 4), clean.numpy())
    # magnitudes inside a NaN-filled block
    for ri in range(3):
        n = obj.frames(2600, ri) * obj.n_bins[ri]
        blk = torch.full((64 + n + 64,), float("nan"), dtype=torch.float32, device=DEV)
        with torch.cuda.device(DEV):
            obj._magnitude_raw(ri, [xd.data_ptr()], [2600], [blk.data_ptr() + 4 * 64])
        torch.cuda.synchronize()
        assert torch.isnan(blk[:64]).all() and torch.isnan(blk[64 + n:]).all()
        assert torch.equal(blk[64:64 + n].reshape(-1, obj.n_bins[ri]), obj.magnitude(xd, ri))


# ---- (g) stream and front ends -------------------------------------------------------------------------------------------------
def test_follows_the_callers_stream():
    obj = _obj()
    x, y = SR.make_noise(48000, 4, 0.5).to(DEV), SR.make_noise(48000, 5, 0.5).to(DEV)
    want = obj.compare_sums([x], [y])
    want_mag = obj.magnitude(x, 1).cpu()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        junk = torch.randn(4096, 4096, device=DEV) @ torch.randn(4096, 4096, device=DEV)
        x2 = x * 1.0  # produced on the side stream right before the call reads it
        got = obj.compare_sums([x2], [y])
        got_mag = obj.magnitude(x2, 1).to("cpu")
    side.synchronize()
    assert torch.equal(got, want) and torch.equal(got_mag, want_mag) and torch.isfinite(junk).all()


def test_mstft_distance_resamples_first():
    import resample_ref as RR
    from valle_amd.codec import Resampler
    from valle_amd.stft import mstft_distance, shared_mstft

    a, b = (RR.make_noise(16000, 5) * 0.1).to(DEV), (RR.make_noise(17000, 6) * 0.1).to(DEV)
    rs = Resampler(16000, 24000).to(DEV)
    a24, b24 = rs(a), rs(b)
    want = shared_mstft(DEV).compare(a24.reshape(-1), b24.reshape(-1))
    assert mstft_distance(a, b, sr=16000) == want.total and math.isfinite(want.total) and want.total > 0
    assert mstft_distance(a24, b24) == want.total == mstft_distance(a24, b24, sr=24000)
    with pytest.raises(ValueError):
        mstft_distance(a24[..., :1024], b24)


def test_copy_synthesis_distance_is_the_manual_composition():
    import ganvoc_ref as GR
    from valle_amd.fbank import BigVGANFbank
    from valle_amd.ganvoc import GanVocoder
    from valle_amd.stft import copy_synthesis_distance, shared_mstft
    from valle_amd.vocoder import GriffinLim

    wav = SR.make_noise(24000, 31, 0.1).to(DEV)
    fb = BigVGANFbank().to(DEV)
    mel = fb.extract_batch([wav])[0]
    gl = GriffinLim().to(DEV)
    cfg = GR.GEOMETRIES["g2_snake"]  # hop 16: 94 frames give 1504 samples
    gan = GanVocoder(cfg, state_dict=GR.make_weights(cfg, 1), max_batch=2, max_total_frames=256).to(DEV)
    for voc in (gl, gan):
        rec = voc(mel)
        want = shared_mstft(DEV).compare(rec, wav)
        for got in (copy_synthesis_distance(wav, voc), copy_synthesis_distance(wav, voc, fbank=fb)):
            assert torch.equal(got.sc, want.sc) and torch.equal(got.log_mag, want.log_mag) and got.total == want.total
            assert math.isfinite(got.total) and got.total > 0
            assert got.frames.tolist() == [SR.n_frames(min(rec.numel(), 24000), r) for r in SR.RESOLUTIONS]
    gan.close()


def test_roundtrip_mstft_is_the_hand_composed_chain():
    import encodec_enc_ref as E
    from valle_amd.codec import CodecConfig, EncodecDecoder
    from valle_amd.stft import shared_mstft

    geo = E.FULL
    enc = EncodecDecoder(CodecConfig(hidden=geo.hidden, filters=geo.filters, codebook_size=geo.codebook_size,
                                     n_codebooks=geo.n_codebooks), max_frames=256, max_batch=2, encoder=True)
    enc.load_state_dict(E.make_enc_weights(geo, 3), strict=True)
    enc.to(DEV)
    wav = E.make_wave(24001, 8).to(DEV)
    rec = enc.decode(enc.encode(wav))
    want = shared_mstft(DEV).compare(rec.reshape(-1), wav.reshape(-1))
    got = enc.roundtrip_mstft(wav)
    assert torch.equal(got.sc, want.sc) and torch.equal(got.log_mag, want.log_mag) and got.total == want.total and math.isfinite(got.total)
    assert got.frames.tolist() == [SR.n_frames(24001, r) for r in SR.RESOLUTIONS]
    before = enc.roundtrip_mel_distance(wav)
    assert before.dim() == 0 and torch.isfinite(before)  # untouched: still the log-mel figure
