"""GPU: the mel-spectrogram Transformer (vx_mel_*, valle_amd.models.Transformer) against the fp64 restatement of
tests/meltf_ref.py, through the fixtures of tests/golden/meltf (tools/gen_meltf_golden.py) in fp32 and bf16.

Tolerances are the project's own: fp32 engine 5e-4 absolute (the AR logits bound of test_gpu_engine.py); bf16 engine 0.03 x the
largest magnitude of the reference row (test_gpu_engine.py's teacher-forced bound), for stop logits 0.03 x the largest |stop
logit| of the sequence.
  1. teacher-forced row pass: predict and stop_logits at every row;
  2. teacher-forced decode (the cached step fed the fixture's frames): every step's frame and stop logit, and step against row pass;
  3. free-running fp32: frame count, stop reason, every frame; bf16: frame 0, the stop pass inside the window the reference's
     logits leave (+-2 tol), later drift printed (and written where VX_MELTF_PARITY_OUT names a file);
  4. properties: repeat and graph / no-graph bitwise, texts of different lengths back to back, NaN-prefilled output, max_frames
     prefix, the first-pass stop, capacity;
  5. d 1024 / 16 heads (the tuned width) on random weights against the restatement computed here; d 256 / 4 heads with 70 text
     ids the same way (encoder stack and both cross-attention kernels past one 64-key tile);
  6. the output goes into mel_distance and the mel-cepstral DTW against a BigVGANFbank result of another length."""
import json
import os

import pytest
import torch

from meltf_ref import MelRef
from test_meltf_cpu import FIXTURES, load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FP32_TOL, BF16_REL = 5e-4, 0.03
_ENG, _PARITY, _TUNED = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    yield
    for e in _ENG.values():
        e.close()
    _ENG.clear()
    out = os.environ.get("VX_MELTF_PARITY_OUT")
    if out and _PARITY:
        with open(out, "w") as f:
            json.dump(_PARITY, f, indent=1, sort_keys=True)


def engine(name, prec, no_graph=False, max_frames=96):
    from valle_amd.engine import MelEngine

    key = (name, prec, no_graph, max_frames)
    if key not in _ENG:
        f = load_fixture(name)
        e = MelEngine(f["cfg"], precision=prec, max_text=16, max_frames=max_frames, no_graph=no_graph)
        e.load_state_dict(f["sd"])
        _ENG[key] = e
    return _ENG[key]


def check_rows(got, ref, prec, what):
    """(T, 100) frames against fp64, row by row."""
    err = (got.double().cpu() - ref).abs()
    tol = torch.full((ref.shape[0],), FP32_TOL, dtype=torch.float64) if prec == "fp32" else BF16_REL * ref.abs().amax(1)
    worst = float((err.amax(1) / tol).max()) if ref.shape[0] else 0.0
    print(f"{what}: max err {float(err.max()) if err.numel() else 0.0:.3e}, worst err / tol {worst:.3f}")
    assert worst <= 1.0, what


def check_stops(got, ref, prec, what):
    err = (got.double().cpu() - ref).abs()
    tol = FP32_TOL if prec == "fp32" else BF16_REL * float(ref.abs().max())
    print(f"{what}: max err {float(err.max()):.3e}, tol {tol:.3e}")
    assert float(err.max()) <= tol, what


@pytest.mark.parametrize("prec", ("fp32", "bf16"))
@pytest.mark.parametrize("name", FIXTURES)
def test_teacher_forced_rows_and_steps(name, prec):
    f = load_fixture(name)
    e = engine(name, prec)
    T = f["run_frames"].shape[0]
    fed = f["run_frames"].float()
    predict, stops = e.teacher_forced(f["x"], fed)
    check_rows(predict, f["run_frames"], prec, f"{name} {prec} row pass predict")
    check_stops(stops, f["run_stops"][:T], prec, f"{name} {prec} row pass stop")
    e.encode(f["x"])
    e.decode_forced(fed)
    frames, reason, st = e.result()
    assert frames.shape == (T, 100) and reason == "max_frames" and st.shape == (T,)
    check_rows(frames, f["run_frames"], prec, f"{name} {prec} cached step predict")
    check_stops(st, f["run_stops"][:T], prec, f"{name} {prec} cached step stop")
    check_rows(frames, predict.double().cpu(), prec, f"{name} {prec} cached step against row pass")
    check_stops(st, stops.double().cpu(), prec, f"{name} {prec} cached step against row pass, stop")


@pytest.mark.parametrize("name", FIXTURES)
def test_free_running_fp32(name):
    f = load_fixture(name)
    e = engine(name, "fp32")
    e.encode(f["x"])
    e.decode(-1)
    frames, reason, stops = e.result()
    n = f["n_frames"]
    assert frames.shape == (n, 100) and reason == f["reason"] and stops.shape == (n + 1,)
    check_rows(frames, f["run_frames"][:n], "fp32", f"{name} free-running fp32 frames")
    check_stops(stops, f["run_stops"][: n + 1], "fp32", f"{name} free-running fp32 stop")


@pytest.mark.parametrize("name", FIXTURES)
def test_free_running_bf16(name):
    f = load_fixture(name)
    e = engine(name, "bf16")
    e.encode(f["x"])
    e.decode(-1)
    frames, reason, stops = e.result()
    ref, n_len = f["run_stops"], 10 * f["S"]  # pass n_len is the length rule's
    tol = BF16_REL * float(ref[: f["n_frames"] + 1].abs().max())
    above = lambda t: next((p for p in range(n_len) if float(ref[p]) > t), n_len)  # noqa: E731
    lo, hi = above(-2 * tol), above(2 * tol)
    stop_pass = stops.numel() - 1
    assert frames.shape[0] == stop_pass and lo <= stop_pass <= hi, (name, lo, stop_pass, hi)
    assert reason == ("length" if stop_pass == n_len else "logit")
    if stop_pass and f["n_frames"]:
        check_rows(frames[:1], f["run_frames"][:1], "bf16", f"{name} free-running bf16 frame 0")
    n = min(stop_pass, f["n_frames"])
    drift = (frames[:n].double().cpu() - f["run_frames"][:n]).abs().amax(1) if n else torch.zeros(0)
    _PARITY[name] = dict(frames=int(stop_pass), reference_frames=f["n_frames"], drift_frame0=float(drift[0]) if n else 0.0,
                         drift_max=float(drift.max()) if n else 0.0, drift_last=float(drift[-1]) if n else 0.0)
    print(f"{name} free-running bf16: {stop_pass} frames (reference {f['n_frames']}), drift {_PARITY[name]}")


def test_properties_fp32():
    from valle_amd.engine import VxError

    f = load_fixture("a_prenorm")
    e = engine("a_prenorm", "fp32")

    def run(eng, x, max_frames=-1):
        eng.encode(x)
        eng.decode(max_frames)
        fr, why, st = eng.result()
        return fr.clone(), why, st.clone()

    full, why, st = run(e, f["x"])
    again, _, st2 = run(e, f["x"])
    assert why == "length" and torch.equal(full, again) and torch.equal(st, st2)  # two runs: the same bits
    ng, _, st3 = run(engine("a_prenorm", "fp32", no_graph=True), f["x"])
    assert torch.equal(full, ng) and torch.equal(st, st3)  # graph replay and kernel-by-kernel: the same bits
    # one handle, texts of different lengths back to back: each is what a fresh handle gives
    short, why_s, _ = run(e, f["x"][:4])
    assert short.shape == (40, 100) and why_s == "length"
    assert torch.equal(run(e, f["x"])[0], full)
    fresh = engine("a_prenorm", "fp32", max_frames=64)
    assert torch.equal(run(fresh, f["x"][:4])[0], short)
    # max_frames below 10 S: its own reason and a bitwise prefix; the output buffer past n_frames is not touched
    cut, why_c, st_c = run(e, f["x"], 7)
    assert why_c == "max_frames" and torch.equal(cut, full[:7]) and torch.equal(st_c, st[:8])
    out = torch.full((12, 100), float("nan"))
    got, _, _ = e.result(out=out)
    assert got.shape == (7, 100) and torch.equal(out[:7], full[:7]) and bool(torch.isnan(out[7:]).all())
    dev = torch.full((12, 100), float("nan"), device=DEV)
    e.result(out=dev)
    assert torch.equal(dev[:7].cpu(), full[:7]) and bool(torch.isnan(dev[7:]).all())
    # a decode that would run past the handle's capacity without stopping is an error, not garbage
    small = engine("a_prenorm", "fp32", max_frames=20)
    small.encode(f["x"])
    with pytest.raises(VxError) as ei:
        small.decode(-1)
    assert ei.value.code == 4
    with pytest.raises(VxError) as ei:
        small.decode(21)
    assert ei.value.code == 4


def test_first_pass_stop_returns_no_frames():
    from valle_amd.models import Transformer

    f = load_fixture("f_stop_first")
    c = f["cfg"]
    m = Transformer(c.d_model, c.nhead, c.num_layers, norm_first=c.norm_first, add_prenet=c.add_prenet, precision="fp32", max_text=16,
                    max_frames=64, print_eos=False)
    m.load_state_dict(f["sd"])
    m.to(DEV).eval()
    out, stops, reason = m.inference(f["x"][None].to(DEV), torch.tensor([f["S"]]), return_stop_logits=True)
    assert out.shape == (1, 0, 100) and out.dtype == torch.float32 and out.device.type == "cuda"
    assert reason == "logit" and stops.shape == (1,) and float(stops[0]) > 0


@pytest.mark.parametrize("prec", ("fp32", "bf16"))
def test_tuned_width(prec):
    """d 1024, 16 heads, one layer, 4 ids, 8 teacher-forced frames: the step's opening kernel at the width it is tuned for."""
    from valle_amd.config import MelConfig
    from valle_amd.engine import MelEngine
    from valle_amd.weights import mel_synthetic_state_dict, sine_table

    if not _TUNED:
        cfg = MelConfig(1024, 16, 1, True, False)
        sd = mel_synthetic_state_dict(cfg, 11)
        g = torch.Generator().manual_seed(5)
        x = torch.randint(3, 100, (4,), generator=g)
        fed = torch.randn(8, 100, generator=g)
        ref = MelRef(sd, 1024, 16, 1, dtype=torch.float64, pe=sine_table(64, 1024)).teacher_forced(x, fed)
        _TUNED["v"] = (cfg, sd, x, fed, ref)
    cfg, sd, x, fed, (rp, rs) = _TUNED["v"]
    e = MelEngine(cfg, precision=prec, max_text=8, max_frames=16)
    try:
        e.load_state_dict(sd)
        predict, stops = e.teacher_forced(x, fed)
        check_rows(predict, rp, prec, f"d1024 {prec} row pass predict")
        check_stops(stops, rs, prec, f"d1024 {prec} row pass stop")
        e.decode_forced(fed)
        frames, reason, st = e.result()
        assert reason == "max_frames" and frames.shape == (8, 100)
        check_rows(frames, rp, prec, f"d1024 {prec} cached step predict")
        check_stops(st, rs, prec, f"d1024 {prec} cached step stop")
    finally:
        e.close()


@pytest.mark.parametrize("prec", ("fp32", "bf16"))
def test_text_past_one_key_tile(prec):
    """d 256, 4 heads of 64, one layer, 70 ids (max_text 80), 8 teacher-forced frames: the encoder stack, the row pass's
    cross-attention (a second, ragged 64-key tile) and the step's (9 keys per split, the last split short) past 64 text keys."""
    from valle_amd.config import MelConfig
    from valle_amd.engine import MelEngine
    from valle_amd.weights import mel_synthetic_state_dict, sine_table

    if "long" not in _TUNED:
        cfg = MelConfig(256, 4, 1, True, False)
        sd = mel_synthetic_state_dict(cfg, 13)
        g = torch.Generator().manual_seed(7)
        x = torch.randint(3, 100, (70,), generator=g)
        fed = torch.randn(8, 100, generator=g)
        ref = MelRef(sd, 256, 4, 1, dtype=torch.float64, pe=sine_table(96, 256)).teacher_forced(x, fed)
        _TUNED["long"] = (cfg, sd, x, fed, ref)
    cfg, sd, x, fed, (rp, rs) = _TUNED["long"]
    e = MelEngine(cfg, precision=prec, max_text=80, max_frames=16)
    try:
        e.load_state_dict(sd)
        predict, stops = e.teacher_forced(x, fed)
        check_rows(predict, rp, prec, f"70 ids {prec} row pass predict")
        check_stops(stops, rs, prec, f"70 ids {prec} row pass stop")
        e.decode_forced(fed)
        frames, reason, st = e.result()
        assert reason == "max_frames" and frames.shape == (8, 100)
        check_rows(frames, rp, prec, f"70 ids {prec} cached step predict")
        check_stops(st, rs, prec, f"70 ids {prec} cached step stop")
    finally:
        e.close()


def test_output_feeds_the_mel_metrics():
    from valle_amd.dtw import shared_dtw
    from valle_amd.fbank import BigVGANFbank, mel_distance
    from valle_amd.models import Transformer

    f = load_fixture("d_hd64_stop")
    c = f["cfg"]
    m = Transformer(c.d_model, c.nhead, c.num_layers, precision="bf16", max_text=16, max_frames=96, print_eos=False, device=DEV).eval()
    m.load_state_dict(f["sd"])
    mel = m.inference(f["x"][None].to(DEV), torch.tensor([f["S"]]))[0]
    assert mel.dtype == torch.float32 and mel.shape[1] == 100 and mel.shape[0] >= 1
    g = torch.Generator().manual_seed(3)
    wav = (0.1 * torch.randn(12000, generator=g)).to(DEV)
    rec = BigVGANFbank().to(DEV).extract_batch([wav])[0]
    assert rec.shape[1] == 100 and rec.shape[0] != mel.shape[0]
    for v in (mel_distance(mel, rec), mel_distance(mel, rec, warp=True)):
        assert v.dim() == 0 and bool(torch.isfinite(v))
    r = shared_dtw(mel.device, 100, 13).compare(mel, rec)
    assert r.length >= max(mel.shape[0], rec.shape[0]) and bool(torch.isfinite(torch.tensor(r.mcd_db)))
    predict, stops = m.teacher_forced(f["x"][None], torch.tensor([f["S"]]), rec[:32])
    assert predict.shape == (32, 100) and stops.shape == (32,) and bool(torch.isfinite(torch.nn.functional.mse_loss(predict, rec[:32])))
