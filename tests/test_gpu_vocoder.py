"""GPU: the Griffin-Lim vocoder (vocoder_kernels.hpp behind vx_vocoder_synthesize, valle_amd.vocoder.GriffinLim) against the fp64
restatement of tests/vocoder_ref.py.

The signal is vocoder_ref.test_signal (a frequency-modulated 180 Hz tone, a 1234 Hz tone, 0.02 noise) analysed by
tests/fbank_ref.py; the table P is the engine's own (test_vocoder_cpu.py holds it to numpy's pinv).  Yardstick: the restatement in
fp64.  Floor: the same formula in torch fp32 on the host.  Bound: engine error <= 4 x floor (vocoder_ref.TOL_FACTOR, the
project's rule); every figure is printed before it is asserted.  Outputs hold NaN before every call.

1. n_iter = 0 (magnitude and inverse kernels alone): the waveform, at every partly covered envelope, one tile, a tile plus one
   frame and several tiles.
2. one and two iterations at T = 21: the waveform is ill-conditioned where |a| is small, so the returned phases are compared,
   weighted: max |a_fp64| |ang - ang_fp64|, from the zero-phase start and from a seeded init_phase.
3. 32 iterations at T = 40: the spectral convergence of the engine's y, computed in fp64.
4. the round trip through the existing filterbank.
5. a ragged batch at odd pointer offsets: bitwise its solo results, repeatable, the warm start, nothing written outside.
6. Transformer.inference_waveform on a fixture."""
import json
import math
import os

import pytest
import torch

import fbank_ref as FR
import vocoder_ref as VR
from test_meltf_cpu import load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_GL, _REF, _PARITY = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    yield
    for g in _GL.values():
        g.close()
    _GL.clear()
    out = os.environ.get("VX_VOCODER_PARITY_OUT")  # profiles/vocoder_parity.json is written from here
    if out and _PARITY:
        with open(out, "w") as f:
            json.dump(_PARITY, f, indent=1, sort_keys=True)


def _gl(max_batch=8):
    from valle_amd.vocoder import GriffinLim

    if max_batch not in _GL:
        _GL[max_batch] = GriffinLim(max_batch=max_batch).to(DEV)
    return _GL[max_batch]


def _logmel(T):
    """(T, 100) float32 on the host: what the filterbank's definition gives for 256 T samples of the test signal."""
    from valle_amd.fbank import slaney_mel_basis

    key = ("mel", T)
    if key not in _REF:
        _REF[key] = FR.fbank_definition(VR.test_signal(T), slaney_mel_basis()).float().contiguous()
        assert _REF[key].shape == (T, 100)
    return _REF[key]


def _init(T, seed=11):
    g = torch.Generator().manual_seed(seed + T)
    return torch.rand((T, 513), generator=g) * 6.2831853


def _reference(T, n_iter, seeded, dtype):
    """(y, ang, a of the last iteration, mag) of the restatement in `dtype`, computed once."""
    key = (T, n_iter, seeded, dtype)
    if key not in _REF:
        mag = VR.magnitude(_logmel(T), _gl().inverse, dtype)
        init = VR.unit_phase(_init(T), dtype) if seeded else None
        _REF[key] = VR.griffinlim(mag, n_iter, 0.99, init, dtype) + (mag,)
    return _REF[key]


def _run(gl, mels, n_iter, momentum=0.99, inits=None, warm=False, phase=True, offset=0, fill=float("nan")):
    """One raw call: every input `offset` floats into a buffer of `fill`, every output likewise with a float of `fill` after it.
    -> (wavs, phases, the whole output buffers)."""
    def place(t):
        buf = torch.full((t.numel() + offset + 1,), fill, dtype=torch.float32, device=DEV)
        buf[offset: offset + t.numel()] = t.reshape(-1).to(DEV)
        return buf

    def room(n):
        return torch.full((n + offset + 1,), float("nan"), dtype=torch.float32, device=DEV)

    def ptr(b, n):
        return b.data_ptr() + 4 * offset if n else 0

    Ts = [m.shape[0] for m in mels]
    ins = [place(m) for m in mels]
    ini = None if inits is None else [place(p) for p in inits]
    wav = [room(256 * T) for T in Ts]
    ph = [room(1026 * T) for T in Ts] if phase else None
    gl._synthesize_raw([ptr(b, T) for b, T in zip(ins, Ts)], Ts, None if ini is None else [ptr(b, T) for b, T in zip(ini, Ts)],
                       n_iter, momentum, [ptr(b, T) for b, T in zip(wav, Ts)],
                       None if ph is None else [ptr(b, T) for b, T in zip(ph, Ts)], warm=warm)
    torch.cuda.synchronize()
    wavs = [b[offset: offset + 256 * T].clone() for b, T in zip(wav, Ts)]
    phases = [b[offset: offset + 1026 * T].clone().reshape(T, 513, 2) for b, T in zip(ph, Ts)] if phase else None
    return wavs, phases, wav + (ph or [])


def _guards_hold(bufs, Ts_sizes, offset):
    for b, n in zip(bufs, Ts_sizes):
        assert bool(torch.isnan(b[:offset]).all()) and bool(torch.isnan(b[offset + n:]).all()), "a write outside an output"
        assert not bool(torch.isnan(b[offset: offset + n]).any()), "an output cell was not written"


# ---- 1. n_iter = 0 ------------------------------------------------------------------------------------------------------------
def test_tile_size_is_the_one_the_cases_assume():
    from valle_amd.vocoder import TILE_FRAMES, TILE_FRAMES_SMALL

    # a call of few frames runs on tiles of 4, a large one on tiles of 16 (test_a_large_call_is_bitwise_its_solo_results).  Cases
    # below: 4 and 16 (one tile), 5 and 17 (a tile plus one frame), 21 and 40 (several tiles)
    assert (TILE_FRAMES_SMALL, TILE_FRAMES) == (4, 16)


@pytest.mark.parametrize("T", (1, 2, 3, 4, 5, 16, 17, 21, 40))
def test_zero_iterations_against_fp64(T):
    gl = _gl()
    wavs, phases, bufs = _run(gl, [_logmel(T)], 0)
    _guards_hold(bufs, [256 * T, 1026 * T], 0)
    got = wavs[0].double().cpu()
    y64 = _reference(T, 0, False, torch.float64)[0]
    y32 = _reference(T, 0, False, torch.float32)[0]
    floor = float((y32.double() - y64).abs().max())
    err = float((got - y64).abs().max())
    print(f"vocoder n_iter=0 T={T}: max |y| {float(y64.abs().max()):.3f} floor {floor:.3e} engine {err:.3e} ratio {err / max(floor, 1e-300):.2f}")
    assert got.shape == (256 * T,) and floor > 0
    assert err <= VR.tolerance(floor)
    ang = phases[0].cpu()
    assert bool((ang[..., 0] == 1).all()) and bool((ang[..., 1] == 0).all())  # the zero-phase start comes back as it is


# ---- 2. one and two iterations: the phases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seeded", (False, True))
@pytest.mark.parametrize("n_iter", (1, 2))
def test_phases_after_one_and_two_iterations(n_iter, seeded):
    T = 21
    gl = _gl()
    inits = [_init(T)] if seeded else None
    wavs, phases, bufs = _run(gl, [_logmel(T)], n_iter, inits=inits)
    _guards_hold(bufs, [256 * T, 1026 * T], 0)
    _, ang64, a64, _ = _reference(T, n_iter, seeded, torch.float64)
    _, ang32, _, _ = _reference(T, n_iter, seeded, torch.float32)
    got = torch.view_as_complex(phases[0].cpu().double().contiguous())
    w = a64.abs()
    floor = float((w * (ang32.to(torch.complex128) - ang64).abs()).max())
    err = float((w * (got - ang64).abs()).max())
    print(f"vocoder phases n_iter={n_iter} seeded={seeded}: smallest |a| {float(w.min()):.2e} floor {floor:.3e} engine {err:.3e} "
          f"ratio {err / max(floor, 1e-300):.2f}")
    assert floor > 0 and err <= VR.tolerance(floor)
    assert float((got.abs() - 1).abs().max()) < 1e-5


# ---- 3. 32 iterations: spectral convergence -----------------------------------------------------------------------------------
def test_spectral_convergence_after_32_iterations():
    T = 40
    gl = _gl()
    y0 = _run(gl, [_logmel(T)], 0, phase=False)[0][0].cpu()
    y32 = _run(gl, [_logmel(T)], 32, phase=False)[0][0].cpu()
    r64_0, r64_32, r32_32 = (_reference(T, 0, False, torch.float64), _reference(T, 32, False, torch.float64),
                             _reference(T, 32, False, torch.float32))
    mag = r64_0[3]
    sc = {"engine_0": VR.spectral_convergence(y0, mag), "engine_32": VR.spectral_convergence(y32, mag),
          "fp64_0": VR.spectral_convergence(r64_0[0], mag), "fp64_32": VR.spectral_convergence(r64_32[0], mag),
          "host_fp32_32": VR.spectral_convergence(r32_32[0], mag)}
    print("vocoder spectral convergence T=40: " + " ".join(f"{k} {v:.6f}" for k, v in sc.items()))
    _PARITY["spectral_convergence_T40"] = sc
    assert sc["engine_32"] < sc["engine_0"]
    assert sc["engine_32"] < sc["fp64_0"]
    assert abs(sc["engine_32"] - sc["fp64_32"]) <= VR.TOL_FACTOR * max(abs(sc["host_fp32_32"] - sc["fp64_32"]), 1e-4)


# ---- 4. the round trip through the filterbank ---------------------------------------------------------------------------------
def test_round_trip_through_the_filterbank():
    from valle_amd.fbank import BigVGANFbank, mel_distance

    gl = _gl()
    fb = BigVGANFbank(max_batch=2).to(DEV)
    m = _logmel(40).to(DEV)
    back = fb.extract_batch([gl(m, n_iter=0), gl(m, n_iter=32)])
    assert back[0].shape == back[1].shape == m.shape
    d0, d32 = float(mel_distance(back[0], m)), float(mel_distance(back[1], m))
    print(f"vocoder round trip T=40: mel distance {d0:.4f} at 0 iterations, {d32:.4f} at 32")
    _PARITY["round_trip_mel_distance_T40"] = {"n_iter_0": d0, "n_iter_32": d32}
    assert math.isfinite(d0) and math.isfinite(d32)
    assert d32 < d0
    fb.close()


# ---- 5. ragged batch ----------------------------------------------------------------------------------------------------------
def test_ragged_batch_is_bitwise_its_solo_results():
    gl = _gl()
    Ts = (0, 1, 3, 17, 40)
    mels = [_logmel(T) if T else torch.zeros(0, 100) for T in Ts]
    inits = [_init(T) if T else torch.zeros(0, 513) for T in Ts]
    sizes = [256 * T for T in Ts] + [1026 * T for T in Ts]
    w0, p0, bufs = _run(gl, mels, 3, inits=inits, offset=1)
    _guards_hold(bufs, sizes, 1)
    w1, p1, _ = _run(gl, mels, 3, inits=inits, offset=3, fill=0.0)  # what surrounds the inputs does not matter; two calls agree
    for i, T in enumerate(Ts):
        assert torch.equal(w0[i], w1[i]) and torch.equal(p0[i], p1[i]), T
        if T == 0:
            continue
        ws, ps, _ = _run(gl, [mels[i]], 3, inits=[inits[i]])
        assert torch.equal(w0[i], ws[0]) and torch.equal(p0[i], ps[0]), f"T={T}: the batch differs from the utterance alone"
    # another order of the same utterances
    w2, p2, _ = _run(gl, mels[::-1], 3, inits=inits[::-1], offset=1)
    for i in range(len(Ts)):
        assert torch.equal(w0[i], w2[len(Ts) - 1 - i]) and torch.equal(p0[i], p2[len(Ts) - 1 - i])
    # the warm start: the returned phases with n_iter = 0 give the waveform again, bit for bit
    w3, p3, bufs3 = _run(gl, mels, 0, inits=p0, warm=True, offset=1)
    _guards_hold(bufs3, sizes, 1)
    for i in range(len(Ts)):
        assert torch.equal(w3[i], w0[i]) and torch.equal(p3[i], p0[i])


def test_a_large_call_is_bitwise_its_solo_results():
    """A call of few frames runs on tiles of 4 frames, a large one (here 8 x 1100 frames, above 2 x 16 frames per CU) on tiles of
    16: the bits must not depend on which."""
    gl = _gl()
    g = torch.Generator().manual_seed(3)
    mels = [(torch.randn((1100, 100), generator=g) * 2.0 - 4.0).to(DEV) for _ in range(8)]
    wavs, phases = gl.synthesize_batch(mels, n_iter=2, return_phase=True)
    for i in (0, 7):
        w, p = gl(mels[i], n_iter=2, return_phase=True)
        assert bool(torch.isfinite(w).all()) and torch.equal(w, wavs[i]) and torch.equal(p, phases[i]), i


def test_synthesize_batch_equals_the_calls():
    from valle_amd.vocoder import GriffinLim

    small = GriffinLim(max_batch=2, max_total_frames=48).to(DEV)  # 5 utterances: several calls, by count and by frames
    mels = [_logmel(T).to(DEV) if T else torch.zeros(0, 100, device=DEV) for T in (17, 0, 3, 40, 1)]
    wavs, phases = small.synthesize_batch(mels, n_iter=2, rand_init=True, seed=5, return_phase=True)
    for i, m in enumerate(mels):
        assert wavs[i].shape == (256 * m.shape[0],) and phases[i].shape == (m.shape[0], 513, 2)
        if m.shape[0] == 0:
            continue
        g = torch.Generator().manual_seed(5 + i)
        start = (torch.rand((m.shape[0], 513), generator=g) * (2.0 * 3.141592653589793)).to(DEV)
        w, p = _gl()(m, n_iter=2, init_phase=start, return_phase=True)
        assert torch.equal(w, wavs[i]) and torch.equal(p, phases[i]), i
    again = small.synthesize_batch(mels, n_iter=2, rand_init=True, seed=5)
    assert all(torch.equal(a, b) for a, b in zip(again, wavs))
    small.close()


# ---- 6. text -> mel -> waveform -----------------------------------------------------------------------------------------------
def _model(name):
    from valle_amd.models import Transformer

    f = load_fixture(name)
    c = f["cfg"]
    m = Transformer(c.d_model, c.nhead, c.num_layers, norm_first=c.norm_first, add_prenet=c.add_prenet, precision="fp32", max_text=16,
                    max_frames=96, print_eos=False)
    m.load_state_dict(f["sd"])
    return m.to(DEV).eval(), f


def test_inference_waveform():
    from valle_amd.vocoder import GriffinLim

    m, f = _model("a_prenorm")
    x, x_lens = f["x"][None].to(DEV), torch.tensor([f["S"]])
    mel, wav = m.inference_waveform(x, x_lens)
    assert torch.equal(mel, m.inference(x, x_lens)) and mel.shape[0] == 1 and mel.shape[1] >= 1
    assert wav.shape == (256 * mel.shape[1],) and wav.device == mel.device and bool(torch.isfinite(wav).all())
    mine = GriffinLim().to(DEV)
    assert torch.equal(wav, mine(mel[0]))
    _, fewer = m.inference_waveform(x, x_lens, vocoder=mine, n_iter=4)
    assert torch.equal(fewer, mine(mel[0], n_iter=4)) and not torch.equal(fewer, wav)
    mine.close()
    m2, f2 = _model("f_stop_first")
    mel2, wav2 = m2.inference_waveform(f2["x"][None].to(DEV), torch.tensor([f2["S"]]))
    assert mel2.shape == (1, 0, 100) and wav2.shape == (0,) and wav2.device == mel2.device
