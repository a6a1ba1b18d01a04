"""CPU: the EnCodec decoder's test-side restatement (tests/encodec_ref.py), its fixtures, the weight layouts and the refusals of
the vx_codec_* entry points (all returned before any HIP call), without a GPU.

The conditions the GPU tests rely on are checked here from the restatement alone: with the generator's weights the waveform
depends on every code, and each deliberately wrong restatement lands at least 100 tolerances from the right one."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import encodec_ref as R
from conftest import GOLDEN, ROOT

CODEC_GOLDEN = os.path.join(GOLDEN, "codec")
LENGTHS = (1, 2, 6, 7, 40)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


def _narrow_cfg():
    from valle_amd.codec import CodecConfig

    return CodecConfig(hidden=16, filters=4, codebook_size=64)


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", [R.FULL, R.NARROW], ids=["full", "narrow"])
def test_restatement_equals_encodec_model_fp64(geo):
    tr = pytest.importorskip("transformers")
    cfg = tr.EncodecConfig(hidden_size=geo.hidden, num_filters=geo.filters, codebook_dim=geo.hidden, codebook_size=geo.codebook_size)
    m = tr.EncodecModel(cfg).double().eval()
    wn = R.to_weight_norm_layout(R.make_weights(geo, 5))
    msd = m.state_dict()
    for k, v in wn.items():
        assert msd[k].shape == v.shape, k
        msd[k] = v.double()
    m.load_state_dict(msd)
    for T in LENGTHS + (5,):
        codes = R.make_codes(geo, 8, T, 2)
        with torch.no_grad():
            want = m.decode(codes[None, None], [None])[0]
        got = R.decode(wn, geo, codes)
        assert got.shape == want.shape == (1, 1, 320 * T)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), T


def test_restatement_reproduces_fixtures():
    z = np.load(os.path.join(CODEC_GOLDEN, "narrow.npz"))
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    assert {k: tuple(v.shape) for k, v in sd.items()} == R.expected_shapes(R.NARROW)
    gen = R.make_weights(R.NARROW, int(z["weight_seed"]))
    assert all(torch.equal(sd[k], gen[k]) for k in gen)  # the committed weights ARE the generator's
    f = np.load(os.path.join(CODEC_GOLDEN, "full.npz"))
    full = R.make_weights(R.FULL, int(f["weight_seed"]))
    for T in LENGTHS:
        for zz, w, geo in ((z, sd, R.NARROW), (f, full, R.FULL)):
            codes = torch.from_numpy(zz[f"codes_{T}"])
            want = torch.from_numpy(zz[f"wav_{T}"])
            assert want.dtype == torch.float64 and want.shape == (1, 1, 320 * T)
            got = R.decode(w, geo, codes)
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (geo, T)


VARIANTS = ("zero_pad", "drop_tap_k7", "drop_tap_k3", "trim_left", "no_skip")


def _check_conditions(sd, geo, T, variants=VARIANTS):
    codes = R.make_codes(geo, 8, T, 1)
    ref, floor, scale = R.floor_and_scale(sd, geo, codes)
    tol = R.tolerance(floor)
    assert floor < 1e-5 * scale
    for t0 in sorted({0, T // 2, T - 1}):
        c2 = codes.clone()
        c2[3, t0] = (c2[3, t0] + 1) % geo.codebook_size
        d = (R.decode(sd, geo, c2) - ref).abs()
        assert float(d[..., 320 * t0:].max()) >= 100 * tol, (T, t0)
        if t0 > 6:  # causal beyond the reflect pad (frames 1..6 are mirrored in front of frame 0)
            assert float(d[..., :320 * t0].max()) == 0.0
    for v in variants:
        d = (R.decode(sd, geo, codes, variant=v) - ref).abs()
        assert float(d.max()) >= 100 * tol, (T, v, float(d.max()) / tol)


@pytest.mark.parametrize("T", [1, 2, 6, 7, 75, 753])
def test_generator_inputs_meet_the_test_conditions(T):
    """At the lengths of the GPU test: one changed code (first, middle, last frame) moves the waveform at or after its frame by
    >= 100 tolerances, and nothing before it once past the reflect pad; every wrong restatement is >= 100 tolerances away."""
    _check_conditions(R.make_weights(R.FULL, 3), R.FULL, T)


def test_generator_inputs_meet_the_test_conditions_20s():
    """T = 1505 (about 25 s of fp64 Python LSTM loop in all): the last-frame code change and the two variants that act far from
    the start, i.e. where the longer recurrence could matter; the others act per sample exactly as at T = 753."""
    sd = R.make_weights(R.FULL, 3)
    T = 1505
    codes = R.make_codes(R.FULL, 8, T, 1)
    ref, floor, scale = R.floor_and_scale(sd, R.FULL, codes)
    tol = R.tolerance(floor)
    c2 = codes.clone()
    c2[3, T - 1] = (c2[3, T - 1] + 1) % 1024
    assert float((R.decode(sd, R.FULL, c2) - ref)[..., 320 * (T - 1):].abs().max()) >= 100 * tol
    for v in ("no_skip", "drop_tap_k3"):
        assert float((R.decode(sd, R.FULL, codes, variant=v) - ref).abs().max()) >= 100 * tol, v


@pytest.mark.parametrize("T", LENGTHS)
def test_narrow_fixture_inputs_meet_the_test_conditions(T):
    z = np.load(os.path.join(CODEC_GOLDEN, "narrow.npz"))
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    _check_conditions(sd, R.NARROW, T)


def test_segment_crossing_is_visible():
    """Two utterances decoded as ONE sequence against the second alone, for lengths of the ragged GPU test: >= 100 tolerances
    when LSTM state and taps are both carried across the boundary, when only the LSTM state is (the convolutions of the second
    utterance computed alone), and when only convolution taps are (the LSTM run per utterance)."""
    import torch.nn.functional as F

    geo = R.FULL
    sd = R.make_weights(geo, 3)
    P = R.fold_weight_norm(sd)
    a, b = R.make_codes(geo, 8, 7, 11), R.make_codes(geo, 8, 300, 12)
    ref, floor, _ = R.floor_and_scale(sd, geo, b)
    tol = R.tolerance(floor)
    joined = R.decode(sd, geo, torch.cat([a, b], dim=1))[..., 320 * 7:]
    assert float((joined - ref).abs().max()) >= 100 * tol

    def tail(x_lstm):  # steps 4 and 5 on a (C, L) LSTM output
        up, res, last = R.layer_index(geo)
        x = x_lstm
        for i, r in enumerate(geo.ratios):
            x = R.up_conv(F.elu(x), P[f"decoder.layers.{up[i]}.conv.weight"], P[f"decoder.layers.{up[i]}.conv.bias"], r)
            p = f"decoder.layers.{res[i]}."
            h = R.causal_conv(F.elu(x), P[p + "block.1.conv.weight"], P[p + "block.1.conv.bias"])
            h = R.causal_conv(F.elu(h), P[p + "block.3.conv.weight"], P[p + "block.3.conv.bias"])
            x = R.causal_conv(x, P[p + "shortcut.conv.weight"], P[p + "shortcut.conv.bias"]) + h
        return R.causal_conv(F.elu(x), P[f"decoder.layers.{last}.conv.weight"], P[f"decoder.layers.{last}.conv.bias"])[None]

    tj, tb, ta = {}, {}, {}
    R.decode(sd, geo, torch.cat([a, b], dim=1), taps=tj)
    R.decode(sd, geo, b, taps=tb)
    R.decode(sd, geo, a, taps=ta)
    assert float((tail(tb["lstm"].T) - ref).abs().max()) == 0.0  # the split restatement is the restatement
    # LSTM state (and the first convolution's taps) carried, every later tap cut at the boundary
    assert float((tail(tj["lstm"][7:].T) - ref).abs().max()) >= 100 * tol
    # only taps carried: per-utterance LSTM outputs joined, then steps 4-5 over the joined rows
    taps_only = tail(torch.cat([ta["lstm"], tb["lstm"]]).T)[..., 320 * 7:]
    assert float((taps_only - ref).abs().max()) >= 100 * tol


# ---- weights ---------------------------------------------------------------------------------------------------------------
def test_key_layouts_pack_to_identical_tensors():
    from valle_amd.codec import EncodecDecoder, expected_keys, pack_state_dict

    cfg = _narrow_cfg()
    sd = R.make_weights(R.NARROW, 4)
    assert {k: tuple(v) for k, v in expected_keys(cfg).items()} == R.expected_shapes(R.NARROW)
    plain, _, _ = pack_state_dict(cfg, sd)
    assert all(torch.equal(plain[k], sd[k]) for k in sd)
    # parametrised layout with g = |v| exactly (fp64): folds back to the same fp32 tensors bit for bit
    wn = {}
    for k, v in sd.items():
        if k.endswith(".conv.weight"):
            base = k[:-len("weight")] + "parametrizations.weight.original"
            wn[base + "0"] = v.double().flatten(1).norm(dim=1).reshape(-1, 1, 1)
            wn[base + "1"] = v.double()
        else:
            wn[k] = v
    folded, missing, unexpected = pack_state_dict(cfg, wn)
    assert not missing and not unexpected
    assert all(torch.equal(folded[k], sd[k]) for k in sd)
    d = EncodecDecoder(cfg)
    r = d.load_state_dict(wn, strict=True)
    assert not r.missing_keys and not r.unexpected_keys and list(d.state_dict()) == list(expected_keys(cfg))


def test_weight_norm_folding():
    from valle_amd.codec import pack_state_dict

    cfg = _narrow_cfg()
    sd = R.make_weights(R.NARROW, 4)
    wn = R.to_weight_norm_layout(sd)  # v scaled per channel, g = |w|: folding must undo the scale
    got, _, _ = pack_state_dict(cfg, wn)
    want = R.fold_weight_norm(wn, torch.float64)
    for k in sd:
        assert float((got[k].double() - want[k]).abs().max()) <= 6e-8 * float(want[k].abs().max()) + 1e-30, k
        assert torch.allclose(got[k], sd[k], rtol=1e-5, atol=1e-6)
    # transposed convolutions: the norm runs over dim 0 = INPUT channels there, as torch's weight_norm(dim=0) does
    k = "decoder.layers.3.conv.parametrizations.weight.original0"
    assert wn[k].shape == (R.NARROW.width, 1, 1)


def test_strict_loading_refuses_missing_unexpected_and_shapes():
    from valle_amd.codec import EncodecDecoder

    cfg = _narrow_cfg()
    sd = R.make_weights(R.NARROW, 4)
    bad = dict(sd)
    bad.pop("decoder.layers.15.conv.bias")
    with pytest.raises(RuntimeError, match="missing"):
        EncodecDecoder(cfg).load_state_dict(bad)
    bad = dict(sd, bogus=torch.zeros(1))
    with pytest.raises(RuntimeError, match="unexpected"):
        EncodecDecoder(cfg).load_state_dict(bad)
    r = EncodecDecoder(cfg).load_state_dict(bad, strict=False)  # e.g. a whole EncodecModel state_dict: encoder keys ignored
    assert r.unexpected_keys == ["bogus"]
    bad = dict(sd)
    bad["decoder.layers.0.conv.weight"] = torch.zeros(64, 16, 5)
    with pytest.raises(RuntimeError, match="size mismatch"):
        EncodecDecoder(cfg).load_state_dict(bad)


def test_no_cpu_fallback():
    from valle_amd.codec import AudioTokenizer, EncodecDecoder

    d = EncodecDecoder(_narrow_cfg(), max_frames=8)
    d.load_state_dict(R.make_weights(R.NARROW, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.decode(R.make_codes(R.NARROW, 8, 4, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AudioTokenizer(d).decode([(R.make_codes(R.NARROW, 8, 4, 0)[None], None)])


# ---- C ABI -----------------------------------------------------------------------------------------------------------------
def _cfg_struct(**kw):
    from valle_amd.engine import VxCodecConfig

    c = VxCodecConfig()
    c.struct_size = C.sizeof(VxCodecConfig)
    c.hidden, c.filters, c.kernel, c.last_kernel, c.res_kernel = 16, 4, 7, 7, 3
    for i, r in enumerate((8, 5, 4, 2)):
        c.ratios[i] = r
    c.n_codebooks, c.codebook_size, c.codebook_dim, c.lstm_layers, c.max_frames, c.max_batch, c.device = 8, 64, 16, 2, 64, 2, 0
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_symbols_and_struct_size(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = set(re.findall(r"\b(vx_[a-z0-9_]+)\s*\(", hdr))
    names = {"vx_codec_create", "vx_codec_destroy", "vx_codec_set_weight", "vx_codec_finalize", "vx_codec_decode",
             "vx_op_codec_conv", "vx_op_codec_convtr", "vx_op_codec_lstm"}
    assert names <= declared and names <= set(engine.declared_symbols())
    assert all(hasattr(lib, n) for n in names)
    assert C.sizeof(engine.VxCodecConfig) == 18 * 4
    assert "int32_t ratios[4];" in hdr
    assert C.sizeof(engine.VxConfig) == 64 and C.sizeof(engine.VxDecodeParams) == 56  # the existing structs did not move


def test_create_refusals(lib):
    h = C.c_void_p()
    for kw, code, word in ((dict(struct_size=0), 1, b"struct_size"), (dict(filters=5), 5, b"LSTM width"), (dict(lstm_layers=3), 5, b"lstm_layers"),
                           (dict(codebook_dim=8), 5, b"codebook_dim"), (dict(max_batch=65), 5, b"max_batch"), (dict(max_frames=0), 1, b"positive"),
                           (dict(n_codebooks=33), 5, b"n_codebooks")):
        c = _cfg_struct(**kw)
        assert lib.vx_codec_create(C.byref(c), C.byref(h)) == code, kw
        assert word in lib.vx_last_error(), (kw, lib.vx_last_error())
    for filters in (4, 32):  # both test geometries are served
        assert lib.vx_codec_create(C.byref(_cfg_struct(filters=filters)), C.byref(h)) == 0
        lib.vx_codec_destroy(h)


def test_weight_refusals(lib):
    h = C.c_void_p()
    assert lib.vx_codec_create(C.byref(_cfg_struct()), C.byref(h)) == 0
    w = torch.zeros(64, 16, 7)
    shp = lambda *s: (C.c_int64 * len(s))(*s)
    assert lib.vx_codec_set_weight(h, b"decoder.layers.0.conv.weight", w.data_ptr(), shp(64, 16, 7), 3) == 0
    assert lib.vx_codec_set_weight(h, b"decoder.layers.0.conv.weight", w.data_ptr(), shp(64, 16, 5), 3) == 6
    assert lib.vx_codec_set_weight(h, b"decoder.layers.0.conv.weight", w.data_ptr(), shp(64, 112), 2) == 6
    assert lib.vx_codec_set_weight(h, b"decoder.layers.0.conv.weight_g", w.data_ptr(), shp(64, 16, 7), 3) == 6
    assert b"unknown key" in lib.vx_last_error()
    assert lib.vx_codec_set_weight(h, b"quantizer.layers.8.codebook.embed", w.data_ptr(), shp(64, 16), 2) == 6  # only 8 loaded
    assert lib.vx_codec_finalize(h) == 6  # tensors missing: refused before any device work
    assert b"missing tensor" in lib.vx_last_error()
    lib.vx_codec_destroy(h)


@pytest.mark.parametrize("geo", [R.FULL, R.NARROW], ids=["full", "narrow"])
def test_c_key_table_matches_python(lib, geo):
    """The C side's key / shape table against codec.expected_keys: every key is accepted with its shape, and finalize then gets
    past the 'missing tensor' check (without a GPU it stops at the first HIP call instead)."""
    from valle_amd.codec import CodecConfig, expected_keys

    cfg = CodecConfig(hidden=geo.hidden, filters=geo.filters, codebook_size=geo.codebook_size)
    h = C.c_void_p()
    assert lib.vx_codec_create(C.byref(_cfg_struct(hidden=geo.hidden, filters=geo.filters, codebook_dim=geo.hidden,
                                                   codebook_size=geo.codebook_size)), C.byref(h)) == 0
    keys = expected_keys(cfg)
    assert {k: tuple(v) for k, v in keys.items()} == R.expected_shapes(geo)
    for k, shp in keys.items():
        t = torch.zeros(shp)
        assert lib.vx_codec_set_weight(h, k.encode(), t.data_ptr(), (C.c_int64 * len(shp))(*shp), len(shp)) == 0, k
    rc = lib.vx_codec_finalize(h)
    assert rc in (0, 2) and b"missing tensor" not in lib.vx_last_error()
    if rc == 2:  # no GPU here: the handle whose finalize stopped half way refuses further use instead of claiming to be ready
        assert lib.vx_codec_finalize(h) == 3
        codes = torch.zeros(8, 4, dtype=torch.int64)
        cp, T, op = (C.c_void_p * 1)(codes.data_ptr()), (C.c_int32 * 1)(4), (C.c_void_p * 1)(8)
        assert lib.vx_codec_decode(h, 1, cp, T, 8, op, None) == 3
    lib.vx_codec_destroy(h)


def test_decode_refusals_before_any_hip_call(lib):
    from valle_amd.codec import EncodecDecoder
    from valle_amd.engine import VxError

    d = EncodecDecoder(_narrow_cfg(), max_frames=64, max_batch=2)
    d.load_state_dict(R.make_weights(R.NARROW, 4))
    ok = R.make_codes(R.NARROW, 8, 5, 0)

    def code_of(cs):
        with pytest.raises(VxError) as e:
            d._decode_raw(cs, [8] * len(cs), finalize=False)  # never finalised: no device is touched
        return e.value.code

    hi, lo = ok.clone(), ok.clone()
    hi[7, 4] = 64
    lo[0, 0] = -1
    assert code_of([hi]) == 1 and code_of([lo]) == 1                     # id outside [0, codebook_size)
    assert code_of([torch.zeros(0, 5, dtype=torch.int64)]) == 1          # n_q < 1
    assert code_of([torch.zeros(9, 5, dtype=torch.int64)]) == 1          # n_q > loaded
    assert code_of([torch.zeros(8, 0, dtype=torch.int64)]) == 1          # T < 1
    assert code_of([R.make_codes(R.NARROW, 8, 65, 0)]) == 4              # T > max_frames
    assert code_of([ok, ok, ok]) == 4                                    # n > max_batch
    assert code_of([ok, hi]) == 1                                        # every utterance of a batch is checked
    assert code_of([ok]) == 3                                            # valid arguments: only then the state is looked at
    d.close()
