"""GPU: the EnCodec decoder (csrc/codec_kernels.hpp behind vx_codec_* / vx_op_codec_*) against the fp64 restatement of
tests/encodec_ref.py.

* op level: causal conv rows, transposed conv rows and the LSTM at every shape the decoder uses, single and ragged segments,
  outputs pre-filled with NaN;
* the whole decoder at T = 1, 2, 6, 7, 75, 753, 1505 (weights from the seeded generator) and at the committed narrow fixture;
* a ragged batch against each utterance decoded alone (bitwise), two identical calls (bitwise); a batch whose up-sampling half
  spans several utterance groups; the captured LSTM chain against plain launches (bitwise); a decode on a side stream;
  two handles alive at once, destroyed in interleaved order, against a lone one (bitwise);
* VALLE.inference -> decode end to end.

Tolerance (encodec_ref.TOL_FACTOR = 4): 4 x the fp32 floor, the floor being the same restatement run in torch fp32 on the CPU
against fp64 on the same inputs.  Every comparison prints its figures before it asserts."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encodec_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library(), engine


def _segs(lens):
    s = [0]
    for n in lens:
        s.append(s[-1] + n)
    return (C.c_int32 * len(s))(*s), s


def _report(what, got, ref64, ref32):
    """got (GPU fp32), ref64, ref32 (the CPU fp32 run of the same formula): asserts |got - ref64| <= 4 x |ref32 - ref64|."""
    assert not torch.isnan(got).any(), f"{what}: NaN sentinel left in the output"
    floor = float((ref32.double() - ref64).abs().max())
    err = float((got.double().cpu() - ref64).abs().max())
    scale = float(ref64.abs().max())
    print(f"{what}: scale {scale:.4g} floor {floor:.3e} engine {err:.3e} ratio {err / max(floor, 1e-300):.2f}")
    assert err <= R.tolerance(floor), f"{what}: {err:.3e} > {R.TOL_FACTOR} x floor {floor:.3e} (scale {scale:.4g})"
    return err, floor


def _rows_conv(x, lens, rate, w, b, elu, dtype):
    """Per-segment causal conv on time-major rows (rows, C) -> (rows, O)."""
    outs, o = [], 0
    for n in lens:
        seg = x[o:o + n * rate].to(dtype).T
        outs.append(R.causal_conv(F.elu(seg) if elu else seg, w.to(dtype), b.to(dtype)).T)
        o += n * rate
    return torch.cat(outs)


def _rows_convtr(x, lens, rate, w, b, stride, dtype):
    outs, o = [], 0
    for n in lens:
        seg = x[o:o + n * rate].to(dtype).T
        outs.append(R.up_conv(F.elu(seg), w.to(dtype), b.to(dtype), stride).T)
        o += n * rate
    return torch.cat(outs)


# (c_in, c_out, k, elu, rate): first conv, the four k=3 residual convolutions, the last conv; full then narrow geometry
CONV_SHAPES = [(128, 512, 7, 0, 1), (256, 128, 3, 1, 8), (128, 64, 3, 1, 40), (64, 32, 3, 1, 160), (32, 16, 3, 1, 320), (32, 1, 7, 1, 320),
               (16, 64, 7, 0, 1), (32, 16, 3, 1, 8), (4, 2, 3, 1, 320), (4, 1, 7, 1, 320)]
SEGS = [[37], [1, 2, 6, 7, 21], [5]]


@pytest.mark.parametrize("lens", SEGS, ids=lambda s: "segs" + "_".join(map(str, s)))
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_conv_rows(shape, lens):
    lib, engine = _lib()
    cin, cout, k, elu, rate = shape
    g = torch.Generator().manual_seed(cin * 131 + cout * 7 + k + len(lens))
    rows = sum(lens) * rate
    x = torch.randn(rows, cin, generator=g) * 1.5
    w = torch.randn(cout, cin, k, generator=g) / (cin * k) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    out = torch.full((rows, cout), float("nan"), device=DEV)
    seg, _ = _segs(lens)
    xd = x.to(DEV)
    engine._check(lib.vx_op_codec_conv(xd.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), cin, cout, k, elu, len(lens), seg, rate, None))
    _report(f"conv {shape} {lens}", out, _rows_conv(x, lens, rate, w, b, elu, torch.float64), _rows_conv(x, lens, rate, w, b, elu, torch.float32))


# (c_in, c_out, stride, rate)
CONVTR_SHAPES = [(512, 256, 8, 1), (256, 128, 5, 8), (128, 64, 4, 40), (64, 32, 2, 160), (64, 32, 8, 1), (8, 4, 2, 160)]


@pytest.mark.parametrize("lens", SEGS, ids=lambda s: "segs" + "_".join(map(str, s)))
@pytest.mark.parametrize("shape", CONVTR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_convtr_rows(shape, lens):
    lib, engine = _lib()
    cin, cout, stride, rate = shape
    g = torch.Generator().manual_seed(cin * 17 + stride)
    rows = sum(lens) * rate
    x = torch.randn(rows, cin, generator=g) * 1.5
    w = torch.randn(cin, cout, 2 * stride, generator=g) / (2 * cin) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    out = torch.full((rows * stride, cout), float("nan"), device=DEV)
    seg, _ = _segs(lens)
    xd = x.to(DEV)
    engine._check(lib.vx_op_codec_convtr(xd.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), cin, cout, stride, 1, len(lens), seg, rate, None))
    _report(f"convtr {shape} {lens}", out, _rows_convtr(x, lens, rate, w, b, stride, torch.float64), _rows_convtr(x, lens, rate, w, b, stride, torch.float32))


@pytest.mark.parametrize("lens", [[40], [1, 7, 33, 2], [300]], ids=lambda s: "segs" + "_".join(map(str, s)))
@pytest.mark.parametrize("width,layers", [(512, 2), (64, 2), (128, 2), (256, 2), (512, 1), (64, 1)])
def test_op_lstm(width, layers, lens):
    lib, engine = _lib()
    g = torch.Generator().manual_seed(width + len(lens))
    P = {}
    for l in range(layers):
        P[f"weight_ih_l{l}"] = torch.randn(4 * width, width, generator=g) * (2.0 / width ** 0.5)
        P[f"weight_hh_l{l}"] = torch.randn(4 * width, width, generator=g) * (2.0 / width ** 0.5)
        P[f"bias_ih_l{l}"] = torch.randn(4 * width, generator=g) * 0.1
        P[f"bias_hh_l{l}"] = torch.randn(4 * width, generator=g) * 0.1
    rows = sum(lens)
    x = torch.randn(rows, width, generator=g) * 2.0
    y = torch.full((rows, width), float("nan"), device=DEV)
    seg, _ = _segs(lens)
    arr = lambda n: (C.c_void_p * 2)(*[P[f"{n}_l{l}"].data_ptr() for l in range(layers)])
    xd = x.to(DEV)
    engine._check(lib.vx_op_codec_lstm(xd.data_ptr(), arr("weight_ih"), arr("weight_hh"), arr("bias_ih"), arr("bias_hh"), y.data_ptr(),
                                       width, layers, len(lens), seg, None))

    def ref(dtype):
        Pd = {k: v.to(dtype) for k, v in P.items()}
        outs, o = [], 0
        for n in lens:
            s = x[o:o + n].to(dtype)
            outs.append(R.lstm(s, Pd, "", layers) + s)
            o += n
        return torch.cat(outs)

    _report(f"lstm {width}x{layers} {lens}", y, ref(torch.float64), ref(torch.float32))


# ---- the whole decoder ---------------------------------------------------------------------------------------------------
_DEC = {}


def _decoder(geo, seed, max_frames=1536, max_batch=4, sd=None, lstm_graph=False):
    _lib()
    from valle_amd.codec import CodecConfig, EncodecDecoder

    key = (geo, seed, max_frames, max_batch, lstm_graph)
    if key not in _DEC:
        d = EncodecDecoder(CodecConfig(hidden=geo.hidden, filters=geo.filters, codebook_size=geo.codebook_size,
                                       n_codebooks=geo.n_codebooks), max_frames=max_frames, max_batch=max_batch, lstm_graph=lstm_graph)
        d.load_state_dict(sd if sd is not None else R.make_weights(geo, seed), strict=True)
        _DEC[key] = (d.to(DEV), sd if sd is not None else R.make_weights(geo, seed))
    return _DEC[key]


@pytest.mark.parametrize("T", [1, 2, 6, 7, 75, 753, 1505])
def test_decoder_full_geometry(T):
    dec, sd = _decoder(R.FULL, 3)
    codes = R.make_codes(R.FULL, 8, T, 1)
    ref, floor, scale = R.floor_and_scale(sd, R.FULL, codes)
    wav = dec.decode(codes[None])
    assert wav.shape == (1, 1, 320 * T) and wav.dtype == torch.float32 and wav.is_cuda
    err = float((wav.double().cpu() - ref).abs().max())
    print(f"decoder T={T}: scale {scale:.4g} floor {floor:.3e} ({floor / scale:.2e} rel) engine {err:.3e} ratio {err / floor:.2f}")
    assert torch.isfinite(wav).all()
    assert err <= R.tolerance(floor), f"T={T}: engine {err:.3e} > {R.TOL_FACTOR} x floor {floor:.3e}"


def test_decoder_fewer_codebooks():
    dec, sd = _decoder(R.FULL, 3)
    codes = R.make_codes(R.FULL, 3, 40, 2)
    ref, floor, scale = R.floor_and_scale(sd, R.FULL, codes)
    err = float((dec.decode(codes).double().cpu() - ref).abs().max())
    print(f"decoder n_q=3: floor {floor:.3e} engine {err:.3e}")
    assert err <= R.tolerance(floor)


def test_decoder_narrow_fixture():
    z = np.load(os.path.join(GOLDEN, "codec", "narrow.npz"))
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    dec, _ = _decoder(R.NARROW, -1, max_frames=64, max_batch=1, sd=sd)
    for T in (1, 2, 6, 7, 40):
        codes = torch.from_numpy(z[f"codes_{T}"])
        ref = torch.from_numpy(z[f"wav_{T}"])
        f32 = R.decode(sd, R.NARROW, codes, torch.float32)
        floor = float((f32.double() - ref).abs().max())
        err = float((dec.decode(codes).double().cpu() - ref).abs().max())
        print(f"narrow T={T}: scale {float(ref.abs().max()):.4g} floor {floor:.3e} engine {err:.3e} ratio {err / floor:.2f}")
        assert err <= R.tolerance(floor), f"narrow T={T}: {err:.3e} > {R.TOL_FACTOR} x {floor:.3e}"


def test_ragged_batch_equals_alone_and_repeats_bitwise():
    dec, sd = _decoder(R.FULL, 3)
    lens = [1, 7, 300, 753]
    codes = [R.make_codes(R.FULL, 8, T, 10 + i) for i, T in enumerate(lens)]
    together = [w.clone() for w in dec.decode_batch(codes)]
    again = dec.decode_batch(codes)
    for i, T in enumerate(lens):
        alone = dec.decode(codes[i])
        assert together[i].shape == (1, 1, 320 * T)
        assert torch.equal(together[i], alone), f"utterance {i} (T={T}) differs between the ragged batch and alone"
        assert torch.equal(together[i], again[i]), f"utterance {i}: two identical calls differ"
    ref, floor, _ = R.floor_and_scale(sd, R.FULL, codes[2])
    assert float((together[2].double().cpu() - ref).abs().max()) <= R.tolerance(floor)


def test_batch_spanning_several_groups_equals_alone():
    """The up-sampling half runs over groups of whole utterances of at most max(max_frames, 8192) frames: eight utterances of
    9 500 frames make at least two groups (here 6 + 2), each with its own segment table, offset into the LSTM output and
    copy-out.  Every utterance must be bitwise its alone decode, and one of each group is held against fp64."""
    lens = [1505, 1400, 1, 1536, 1300, 1100, 1358, 1300]
    assert sum(lens) > 8192 and sum(lens[:6]) <= 8192 < sum(lens[:7])
    dec, sd = _decoder(R.FULL, 3, max_frames=1536, max_batch=8)
    codes = [R.make_codes(R.FULL, 8, T, 40 + i) for i, T in enumerate(lens)]
    together = [w.clone() for w in dec.decode_batch(codes)]
    for i, T in enumerate(lens):
        alone = dec.decode(codes[i])
        assert together[i].shape == (1, 1, 320 * T)
        assert torch.equal(together[i], alone), f"utterance {i} (T={T}) differs between the multi-group batch and alone"
    for i in (2, 5, 7):  # first group (the one-frame utterance and a long one) and second group
        ref, floor, _ = R.floor_and_scale(sd, R.FULL, codes[i])
        err = float((together[i].double().cpu() - ref).abs().max())
        print(f"groups utterance {i} T={lens[i]}: floor {floor:.3e} engine {err:.3e} ratio {err / floor:.2f}")
        assert err <= R.tolerance(floor)


def test_captured_chain_equals_plain_launches():
    """The LSTM steps launched one by one (default) and replayed as the captured chain (lstm_graph) are the same kernels on the
    same operands: bitwise equal, for one utterance, lengths around the chain length (64 steps per replay) and a ragged batch."""
    p, sd = _decoder(R.FULL, 3)
    g, _ = _decoder(R.FULL, 3, lstm_graph=True)
    for T in (1, 62, 63, 64, 65, 128, 129, 753):
        codes = R.make_codes(R.FULL, 8, T, 70)
        assert torch.equal(g.decode(codes), p.decode(codes)), T
    codes = [R.make_codes(R.FULL, 8, T, 80 + i) for i, T in enumerate((64, 1, 200, 65))]
    for a, b in zip(g.decode_batch(codes), p.decode_batch(codes)):
        assert torch.equal(a, b)


def test_decode_follows_the_callers_stream():
    """vx_codec_decode orders its work after the caller's stream and the caller's stream after it: a decode issued on a side
    stream right behind the kernel that fills nothing but delays, read back on that stream, equals the default-stream result."""
    dec, _ = _decoder(R.FULL, 3)
    codes = R.make_codes(R.FULL, 8, 75, 90)
    want = dec.decode(codes).cpu()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        junk = torch.randn(4096, 4096, device=DEV) @ torch.randn(4096, 4096, device=DEV)
        got = dec.decode(codes)
        host = got.to("cpu", non_blocking=False)
    side.synchronize()
    assert torch.equal(host, want) and torch.isfinite(junk).all()


def test_two_handles_alive_at_once_decode_as_a_lone_one():
    """Every handle owns its device side as a whole: two narrow handles, one of them with the encoder, are finalised before either
    is used, decode T = 1 and T = 7 in turn (an encode between), and are destroyed in interleaved order with a third made
    in between.  Every decode is bitwise that of a handle that was alone on the device."""
    _lib()
    import encodec_enc_ref as E
    from valle_amd.codec import CodecConfig, EncodecDecoder

    geo = R.NARROW
    sd = E.make_enc_weights(geo, 5)
    dec_sd = {k: v for k, v in sd.items() if not k.startswith("encoder.")}

    def make(encoder):
        d = EncodecDecoder(CodecConfig(hidden=geo.hidden, filters=geo.filters, codebook_size=geo.codebook_size, n_codebooks=geo.n_codebooks),
                           max_frames=8, max_batch=2, encoder=encoder)
        d.load_state_dict(sd if encoder else dec_sd, strict=True)
        d.to(DEV).handle()  # created and finalised here
        return d

    codes = {T: R.make_codes(geo, 8, T, 20 + T) for T in (1, 7)}
    lone = make(False)
    want = {T: lone.decode(c).clone() for T, c in codes.items()}
    lone.close()
    assert all(w.shape == (1, 1, geo.hop * T) and torch.isfinite(w).all() for T, w in want.items())

    a, b = make(False), make(True)
    assert torch.equal(a.decode(codes[1]), want[1]) and torch.equal(b.decode(codes[7]), want[7])
    enc = b.encode_batch([E.make_wave(geo.hop * 7, 3).to(DEV)])
    assert enc[0].shape[-2:] == (geo.n_codebooks, 7)
    assert torch.equal(b.decode(codes[1]), want[1]) and torch.equal(a.decode(codes[7]), want[7])
    a.close()
    assert torch.equal(b.decode(codes[7]), want[7])
    c = make(False)
    assert torch.equal(c.decode(codes[7]), want[7]) and torch.equal(b.decode(codes[1]), want[1])
    b.close()
    assert torch.equal(c.decode(codes[1]), want[1])
    c.close()


def test_inference_to_waveform_end_to_end():
    _lib()
    from valle_amd.codec import AudioTokenizer
    from valle_amd.config import ModelConfig
    from valle_amd.models import VALLE
    from valle_amd.weights import synthetic_inputs, synthetic_state_dict

    cfg = ModelConfig(decoder_dim=256, nhead=4, num_decoder_layers=4, prefix_mode=1)
    x, x_lens, y = synthetic_inputs(4, 30)
    m = VALLE(256, 4, 4, prefix_mode=1, precision="fp32", max_text=64, max_audio=256, print_eos=False)
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    m.to(DEV).eval()
    frames = m.inference(x.to(DEV), x_lens.to(DEV), y.to(DEV), None, top_k=1)  # (1, T, 8)
    dec, _ = _decoder(R.FULL, 3)
    wav = AudioTokenizer(dec).decode([(frames.transpose(2, 1), None)])
    assert wav.shape == (1, 1, 320 * frames.shape[1]) and wav.is_cuda
    assert torch.isfinite(wav).all()
