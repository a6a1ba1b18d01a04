"""GPU: the log-mel filterbank (fbank_kernel behind vx_fbank_extract, valle_amd.fbank.BigVGANFbank) against the fp64 definition
of tests/fbank_ref.py.

* parity: Gaussian noise of amplitude 0.1 and 1.0, L in {128, 1024, 1025, 4801, 24000, tile + 1 frames}, outputs pre-filled
  with NaN.  Yardstick: the reference's formula (torch.stft) in fp64.  Floor: the same formula in torch fp32 on the host.
  Bound: engine error <= 4 x floor (fbank_ref.TOL_FACTOR, the rule of the codec's and the resampler's tests); every ratio is
  printed before it is asserted.  No fp64 mel cell of these inputs lies within [0.5e-5, 2e-5], which is asserted first: the
  clamp cannot make a cell undecidable;
* digital silence: every cell the same bits, within the bound of log(1e-5);
* fewer than 128 samples: an empty result, nothing written;
* a ragged batch at odd pointer offsets: every utterance bitwise its solo result, two calls bitwise equal;
* a dense random basis of 37 filters supplied by the caller: parity under the same rule;
* no dependence on memory the call does not own (guards of zeros / NaN, VX_POISON on the handle's own allocations), in fresh
  child processes;
* the call follows the caller's stream;
* composition: extract == extract_batch, sr= is resample-then-extract, mel_distance, EncodecDecoder.roundtrip_mel_distance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import encodec_enc_ref as E
import fbank_ref as FR
import resample_ref as RR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_FB = {}


def _build():
    import __graft_entry__ as ge

    ge.build()


def _fbank(key="default"):
    _build()
    from valle_amd.fbank import BigVGANFbank, BigVGANFbankConfig

    if key not in _FB:
        if key == "dense37":
            g = torch.Generator().manual_seed(37)
            basis = torch.rand(37, 513, generator=g) * 0.02
            _FB[key] = BigVGANFbank(BigVGANFbankConfig(num_mel_bins=37), mel_basis=basis, max_batch=8).to(DEV)
        else:
            _FB[key] = BigVGANFbank(max_batch=8).to(DEV)
    return _FB[key]


def _tile_plus_one():
    from valle_amd.fbank import TILE_FRAMES

    return (TILE_FRAMES + 1) * 256


def _run_nan_prefilled(fb, x):
    """One utterance through vx_fbank_extract into an output that holds NaN before the call."""
    x = x.reshape(-1).to(DEV).contiguous()
    out = torch.full((FR.n_frames(x.numel()), fb.mel_basis.shape[0]), float("nan"), device=DEV)
    fb._extract_raw([x.data_ptr()], [x.numel()], [out.data_ptr()])
    return out


def _check_parity(fb, x, tag):
    basis = fb.mel_basis
    assert FR.share_near_clip(x, basis) == 0.0, f"{tag}: an fp64 mel cell lies within a factor 2 of the clip"
    ref64 = FR.fbank_definition(x, basis)
    ref32 = FR.fbank_definition(x, basis, torch.float32)
    got = _run_nan_prefilled(fb, x)
    assert got.shape == ref64.shape == ref32.shape == (FR.n_frames(x.numel()), basis.shape[0])
    assert not torch.isnan(got).any(), f"{tag}: NaN sentinel left in the output"
    floor = float((ref32.double() - ref64).abs().max())
    err = float((got.double().cpu() - ref64).abs().max())
    print(f"fbank {tag}: frames {got.shape[0]} floor {floor:.3e} engine {err:.3e} ratio {err / max(floor, 1e-300):.2f}")
    return None if err <= FR.tolerance(floor) else f"{tag}: engine {err:.3e} > {FR.TOL_FACTOR} x floor {floor:.3e}"


@pytest.mark.parametrize("amp", (0.1, 1.0))
def test_parity_with_fp64(amp):
    fb = _fbank()
    failures = []
    for L in (128, 1024, 1025, 4801, 24000, _tile_plus_one()):
        x = FR.make_noise(L, 7 * L + int(10 * amp), amp)
        failures.append(_check_parity(fb, x, f"amp {amp} L={L}"))
    assert not any(failures), [f for f in failures if f]


def test_parity_with_a_dense_basis_of_the_callers():
    fb = _fbank("dense37")
    assert fb.feature_dim(24000) == 37 and int((fb.mel_basis > 0).sum(1).min()) > 500
    failures = []
    for amp in (0.1, 1.0):
        for L in (1025, 4801):
            x = FR.make_noise(L, 3 * L + int(10 * amp), amp)
            failures.append(_check_parity(fb, x, f"dense 37, amp {amp} L={L}"))
    assert not any(failures), [f for f in failures if f]


def test_digital_silence():
    fb = _fbank()
    x = torch.zeros(4801)
    got = _run_nan_prefilled(fb, x).cpu()
    assert got.shape == (19, 100)
    bits = got.view(torch.int32)
    assert bool((bits == bits[0, 0]).all()), "silence: the cells differ"
    ref64 = FR.fbank_definition(x, fb.mel_basis)
    assert float((ref64 - np.log(1e-5)).abs().max()) == 0.0
    floor = float((FR.fbank_definition(x, fb.mel_basis, torch.float32).double() - ref64).abs().max())
    err = abs(float(got[0, 0].double()) - np.log(1e-5))
    print(f"fbank silence: floor {floor:.3e} engine {err:.3e} ratio {err / max(floor, 1e-300):.2f}")
    assert err <= FR.tolerance(floor)


def test_fewer_than_128_samples_give_an_empty_result_and_write_nothing():
    fb = _fbank()
    x = FR.make_noise(127, 1).to(DEV)
    out = fb.extract_batch([x])[0]
    assert out.shape == (0, 100) and out.dtype == torch.float32 and out.device.type == "cuda"
    assert fb.extract(x.cpu().numpy(), 24000).shape == (0, 100)
    guard = torch.full((256,), float("nan"), device=DEV)
    fb._extract_raw([x.data_ptr()], [127], [guard.data_ptr() + 64])
    y = FR.make_noise(128, 2).to(DEV)
    first = torch.full((100,), float("nan"), device=DEV)
    fb._extract_raw([x.data_ptr(), y.data_ptr()], [127, 128], [guard.data_ptr() + 64, first.data_ptr()])  # beside one that has a frame
    torch.cuda.synchronize()
    assert bool(torch.isnan(guard).all()), "an utterance without frames was written to"
    assert torch.equal(first, fb.extract_batch([y])[0][0])


def test_ragged_batch_equals_alone_and_repeats_bitwise():
    """Mixed lengths in one call, among them one sample, one below and one at the first frame, and waveforms and outputs that
    start one float past a 16-byte boundary."""
    fb = _fbank()
    lengths = [1, 127, 128, 1025, 4801, 72001]
    bufs, outs = [], []
    for i, L in enumerate(lengths):
        b = torch.zeros(L + 8, device=DEV)
        b[1:1 + L] = FR.make_noise(L, 50 + i, 0.3).to(DEV)
        bufs.append(b)
        outs.append([torch.full((FR.n_frames(L) * 100 + 8,), float("nan"), device=DEV) for _ in range(2)])
    for rep in range(2):
        fb._extract_raw([b.data_ptr() + 4 for b in bufs], lengths, [o[rep].data_ptr() + 4 for o in outs])
    torch.cuda.synchronize()
    for i, L in enumerate(lengths):
        n = FR.n_frames(L) * 100
        together, again = outs[i][0], outs[i][1]
        assert bool(torch.isnan(together[:1]).all()) and bool(torch.isnan(together[1 + n:]).all()), f"utterance {i}: written outside its output"
        alone = fb.extract_batch([bufs[i][1:1 + L].clone()])[0]
        assert alone.shape == (FR.n_frames(L), 100)
        assert torch.equal(together[1:1 + n].view(torch.int32), alone.reshape(-1).view(torch.int32)), f"utterance {i} (L={L}) differs between the batch and alone"
        assert torch.equal(together[1:1 + n].view(torch.int32), again[1:1 + n].view(torch.int32)), f"utterance {i}: two identical calls differ"
        assert bool(torch.isfinite(alone).all())
    # a frame's bits depend on its own samples only: the same audio later in a longer utterance, in another tile
    x = FR.make_noise(256 * 40, 9, 0.3)
    a = fb.extract_batch([x])[0]
    b = fb.extract_batch([x[256 * 5:]])[0]
    assert torch.equal(a[5:38], b[:33])


def test_follows_the_callers_stream():
    fb = _fbank()
    x = FR.make_noise(48000, 4, 0.5).to(DEV)
    want = fb.extract_batch([x])[0].cpu()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        junk = torch.randn(4096, 4096, device=DEV) @ torch.randn(4096, 4096, device=DEV)
        x2 = x * 1.0  # produced on the side stream right before the call reads it
        host = fb.extract_batch([x2])[0].to("cpu")
    side.synchronize()
    assert torch.equal(host, want) and torch.isfinite(junk).all()


def test_output_does_not_depend_on_memory_it_does_not_own():
    """The inputs sit inside a larger buffer (at an odd offset) and the outputs inside another; what surrounds them is zero in one
    run and NaN in the other, and VX_POISON=1 fills the handle's own fresh allocations with 0xFF bytes.  The outputs must be
    bitwise the same and finite, and the surroundings of the outputs untouched."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = (
        "import sys, json, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import os, fbank_ref as FR\n"
        "from valle_amd.fbank import BigVGANFbank\n"
        "fill = float('nan') if os.environ['VX_GUARD'] == 'nan' else 0.0\n"
        "fb = BigVGANFbank(max_batch=4).to('cuda:0')\n"
        "lengths, ins, outs, bufs, res = [1001, 127, 4801, 130], [], [], [], []\n"
        "for i, L in enumerate(lengths):\n"
        "    b = torch.full((L + 40,), fill, device='cuda:0')\n"
        "    b[13:13 + L] = FR.make_noise(L, i, 0.3).to('cuda:0')\n"
        "    o = torch.full((FR.n_frames(L) * 100 + 40,), fill, device='cuda:0')\n"
        "    bufs.append((b, o)); ins.append(b.data_ptr() + 52); outs.append(o.data_ptr() + 52)\n"
        "fb._extract_raw(ins, lengths, outs)\n"
        "torch.cuda.synchronize()\n"
        "for L, (b, o) in zip(lengths, bufs):\n"
        "    n = FR.n_frames(L) * 100\n"
        "    edge = torch.cat([o[:13], o[13 + n:]])\n"
        "    assert bool(torch.isnan(edge).all()) if fill != fill else bool((edge == 0).all()), 'written outside the output'\n"
        "    assert bool(torch.isfinite(o[13:13 + n]).all()), 'non-finite output'\n"
        "    res.append(o[13:13 + n].cpu().view(torch.int32).tolist())\n"
        "print(json.dumps(res))\n"
        % (root, os.path.join(root, "tests")))
    outs = []
    for poison, guard in (("0", "zero"), ("1", "nan")):
        env = dict(os.environ, VX_POISON=poison, VX_GUARD=guard)
        r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]
    assert [len(o) for o in outs[0]] == [400, 0, 1900, 100]


# ---- composition ---------------------------------------------------------------------------------------------------------------
def test_extract_is_extract_batch_and_the_builtin_basis_is_the_packages():
    from valle_amd.fbank import BigVGANFbank, get_fbank_extractor, mel_distance

    fb = _fbank()
    x = FR.make_noise(4801, 12, 0.3)
    dev = fb.extract_batch([x.to(DEV)])[0]
    for samples in (x.numpy(), x, x[None], x[None].numpy()):
        got = fb.extract(samples, 24000)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (19, 100)
        assert np.array_equal(got.view(np.int32), dev.cpu().numpy().view(np.int32))
    assert torch.equal(fb.extract_batch([x[None, None]])[0], dev)
    ref = get_fbank_extractor()  # the reference's call as it is
    assert ref.device.type == "cuda" and np.array_equal(ref.extract(x.numpy(), 24000), dev.cpu().numpy())
    assert float(mel_distance(dev, dev)) == 0.0 and mel_distance(dev, dev).device.type == "cuda"
    other = fb.extract_batch([x * 0.5])[0]
    assert abs(float(mel_distance(dev, other)) - float((dev - other).abs().mean())) == 0.0 and float(mel_distance(dev, other)) > 0.1
    # more utterances than max_batch: served in several calls
    many = BigVGANFbank(max_batch=2).to(DEV).extract_batch([x, x[:1000], x[:100], x[:2000], x])
    assert [tuple(m.shape) for m in many] == [(19, 100), (4, 100), (0, 100), (8, 100), (19, 100)]
    assert torch.equal(many[0], dev) and torch.equal(many[4], dev)


def test_sr_is_resample_then_extract():
    from valle_amd.codec import Resampler

    fb = _fbank()
    wav = (RR.make_noise(48000, 11, channels=2) * 0.1).to(DEV)
    mono = Resampler(48000, 24000).to(DEV)(wav)
    want = fb.extract_batch([mono])[0]
    got = fb.extract_batch([wav], sr=48000)[0]
    assert got.shape == want.shape == (94, 100) and torch.equal(got, want)
    both = fb.extract_batch([wav, wav[:1, :5000]], sr=48000)
    assert torch.equal(both[0], want) and both[1].shape == (10, 100)
    # at 24 kHz: the channel mean alone; mono goes in as it is
    st = fb.extract_batch([wav], sr=24000)[0]
    assert torch.equal(st, fb.extract_batch([(wav[0] + wav[1]) / 2])[0])
    assert torch.equal(fb.extract_batch([wav[0]], sr=24000)[0], fb.extract_batch([wav[0]])[0])


def test_roundtrip_mel_distance_is_the_hand_composed_chain():
    _build()
    from valle_amd.codec import CodecConfig, EncodecDecoder, Resampler
    from valle_amd.fbank import mel_distance

    geo = E.FULL
    enc = EncodecDecoder(CodecConfig(hidden=geo.hidden, filters=geo.filters, codebook_size=geo.codebook_size,
                                     n_codebooks=geo.n_codebooks), max_frames=256, max_batch=2, encoder=True)
    enc.load_state_dict(E.make_enc_weights(geo, 3), strict=True)
    enc.to(DEV)
    fb = _fbank()
    wav = E.make_wave(24001, 8).to(DEV)
    rec = enc.decode(enc.encode(wav))
    assert rec.shape == (1, 1, 24320)
    a, b = fb.extract_batch([wav, rec])
    assert a.shape == (94, 100) and b.shape == (95, 100)
    want = mel_distance(a, b)
    got = enc.roundtrip_mel_distance(wav)
    assert got.dim() == 0 and got.device.type == "cuda" and torch.isfinite(got) and float(got) > 0
    assert torch.equal(got, want) and torch.equal(want, (a - b[:94]).abs().mean())
    # fewer codebooks, and a stereo prompt at another rate: compared at 24 kHz against the converted input
    a2, b2 = fb.extract_batch([wav, enc.decode(enc.encode(wav, 2))])
    assert torch.equal(enc.roundtrip_mel_distance(wav, n_q=2), mel_distance(a2, b2))
    st = (RR.make_noise(48000, 5, channels=2) * 0.1).to(DEV)
    mono = Resampler(48000, 24000).to(DEV)(st)
    a3, b3 = fb.extract_batch([mono, enc.decode(enc.encode(mono))])
    assert torch.equal(enc.roundtrip_mel_distance(st, sr=48000), mel_distance(a3, b3))
    plain = EncodecDecoder(CodecConfig(hidden=geo.hidden, filters=geo.filters, codebook_size=geo.codebook_size,
                                       n_codebooks=geo.n_codebooks), max_frames=256)
    with pytest.raises(RuntimeError, match="encoder=True"):
        plain.to(DEV).roundtrip_mel_distance(wav)
