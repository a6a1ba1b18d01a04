"""CPU: the speaker encoder's definition, inputs and packaging (valle_amd.spk, vx_spk_*), no GPU needed.

1. the restatement tests/spk_ref.py equals transformers' WavLMForXVector and Wav2Vec2ForXVector in fp64 at 1e-10 relative
   (embeddings and logits; skipped without the package);
2. the bucket rule equals WavLM's `_relative_positions_bucket` for every |r| <= 2000 at (320, 800) and (32, 40), against a table
   recorded from the package (tests/golden/spk/buckets.npz) and, where it is installed, against the package itself;
3. every mutation of spk_ref.MUTATIONS moves the embedding by more than 100 x the GPU test's bound at 33 frames on the GPU test's
   own inputs: the condition under which that bound can tell a wrong implementation from the definition;
4. ABI and packaging: header <=> ctypes <=> exports, struct sizes, every refusal before any HIP call, load_state_dict."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import spk_cases as SC
import spk_ref as R
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


# ---- 1. the restatement against the canonical classes -----------------------------------------------------------------------------
@pytest.mark.parametrize("frames", (16, 17, 61))
@pytest.mark.parametrize("wls", (True, False))
@pytest.mark.parametrize("attention", ("wavlm", "plain"))
def test_restatement_matches_transformers(attention, wls, frames):
    tf = pytest.importorskip("transformers")
    from valle_amd.spk import SpeakerConfig, synthetic_state_dict

    fields = dict(SC._TINY, use_weighted_layer_sum=wls)
    cfg_cls, model_cls = (tf.WavLMConfig, tf.WavLMForXVector) if attention == "wavlm" else (tf.Wav2Vec2Config, tf.Wav2Vec2ForXVector)
    hf_cfg = cfg_cls(**fields)
    cfg = SpeakerConfig.from_any(hf_cfg)  # any object with the attributes
    assert cfg == SpeakerConfig(**fields)
    sd = synthetic_state_dict(cfg, 1, attention)
    model = model_cls(hf_cfg).double().eval()
    res = model.load_state_dict({k: v.double() for k, v in sd.items()}, strict=False)
    assert res.missing_keys == ["objective.weight"] and not res.unexpected_keys
    L = R.samples_for_frames(cfg, frames) + 3
    wav = 0.5 * torch.randn(L, generator=torch.Generator().manual_seed(frames)).double()
    with torch.no_grad():
        want = model(wav[None])
    got = R.forward(SC.ref_state_dict(sd), cfg, wav, torch.float64, attention)
    assert got["hidden"][0].shape[0] == frames
    for name, a, b in (("embeddings", want.embeddings[0], got["embedding"]), ("logits", want.logits[0], got["logits"])):
        rel = float((a - b).abs().max() / a.abs().max())
        print(f"{attention} wls={wls} frames={frames} {name}: {rel:.2e} relative")
        assert rel <= 1e-10, (name, rel)


# ---- 2. the bucket table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,md", ((320, 800), (32, 40)))
def test_bucket_table(nb, md):
    from valle_amd.spk import relative_position_buckets

    r = torch.arange(-2000, 2001)
    want = torch.from_numpy(np.load(os.path.join(GOLDEN, "spk", "buckets.npz"))[f"b{nb}_{md}"].astype(np.int64))
    assert torch.equal(relative_position_buckets(r, nb, md), want)
    assert torch.equal(R.relative_position_buckets(r, nb, md), want)
    # the three regimes occur: exact, logarithmic, saturated
    half = nb // 2
    assert int(want[2000 + half // 2 - 1]) == half + half // 2 - 1 and int(want.max()) == nb - 1 and int(want[0]) == half - 1
    try:
        from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    except ImportError:
        return
    att = WavLMAttention(embed_dim=16, num_heads=1, num_buckets=nb, max_distance=md)
    assert torch.equal(att._relative_positions_bucket(r), want)


def test_regimes_within_60_frames():
    b = R.relative_position_buckets(torch.arange(0, 60), 32, 40)
    assert int(b[7]) == 16 + 7 and int(b[8]) == 16 + 8 and len(set(b[8:40].tolist())) > 2 and int(b[41]) == int(b[59]) == 31


# ---- 3. every mutation moves the output ------------------------------------------------------------------------------------------
def test_every_mutation_moves_the_output():
    name, frames = "tiny_wavlm", 33
    r64 = SC.reference(name, frames, torch.float64)
    bound = SC.TOL_FACTOR * SC.floors(name, frames)["embedding"]
    sd, cfg, wav = SC.ref_state_dict(SC.state_dict(name)), SC.config(name), SC.wave(name, frames)
    small = []
    for m in R.MUTATIONS:
        moved = float((R.forward(sd, cfg, wav, torch.float64, "wavlm", mutation=m)["embedding"] - r64["embedding"]).abs().max())
        print(f"{m:22s} moves the embedding by {moved:.3e} = {moved / bound:8.1f} x the bound {bound:.3e}")
        if not moved > 100 * bound:
            small.append((m, moved / bound))
    assert not small, f"mutations within 100 x the bound: {small}"


# ---- 4. ABI and packaging -------------------------------------------------------------------------------------------------------
def test_header_ctypes_exports(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = sorted(set(re.findall(r"\b(vx_spk_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ["vx_spk_create", "vx_spk_destroy", "vx_spk_embed", "vx_spk_finalize", "vx_spk_frames", "vx_spk_get_timings",
                        "vx_spk_min_samples", "vx_spk_read", "vx_spk_set_buckets", "vx_spk_set_weight", "vx_spk_similarity"]
    assert declared == [s for s in engine.declared_symbols() if s.startswith("vx_spk_")]
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in vallex.h but not exported"


def test_struct_sizes():
    from valle_amd import engine as e

    assert C.sizeof(e.VxSpkConfig) == 280  # 70 four-byte fields, as the header lays them out
    sizes = {"VxConfig": 64, "VxDecodeParams": 56, "VxCodecConfig": 72, "VxFbankConfig": 36, "VxVocoderConfig": 40, "VxGanConfig": 188,
             "VxDtwConfig": 20, "VxPitchConfig": 28, "VxStftConfig": 72, "VxMelConfig": 48}
    for name, size in sizes.items():  # the existing structs are untouched
        assert C.sizeof(getattr(e, name)) == size, name


def _struct(**over):
    from valle_amd.spk import SpeakerEncoder

    enc = SpeakerEncoder(SC.config("tiny_wavlm"), max_batch=2, max_seconds=1.0)
    s = enc._config_struct()
    enc.close()
    for k, v in over.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("over,code,match", (
    (dict(struct_size=0), 1, b"struct_size"),
    (dict(feat_extract_norm=1), 5, b"feat_extract_norm"),
    (dict(do_stable_layer_norm=1), 5, b"do_stable_layer_norm"),
    (dict(add_adapter=1), 5, b"add_adapter"),
    (dict(activation=1), 5, b"activation"),
    (dict(heads=8), 5, b"head_dim = 8"),
    (dict(hidden=96, heads=2, pos_groups=4), 5, b"head_dim = 48"),
    (dict(max_batch=65), 5, b"max_batch"),
    (dict(max_samples=5199), 1, b"5200"),
))
def test_create_refusals_without_gpu(lib, over, code, match):
    s = _struct(**over)
    if "max_samples" in over:  # the default strides and TDNN kernels: the limit is derived from the configuration
        s.n_conv = 7
        for i, (k, st) in enumerate(zip((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2))):
            s.conv_kernel[i], s.conv_stride[i] = k, st
    h = C.c_void_p()
    assert lib.vx_spk_create(C.byref(s), C.byref(h)) == code
    assert match in lib.vx_last_error(), lib.vx_last_error()
    assert not h.value


def test_python_refusals():
    from valle_amd.spk import SpeakerConfig, SpeakerEncoder

    tiny = SC.GEOMETRIES["tiny_wavlm"][1]
    for over in (dict(feat_extract_norm="layer"), dict(do_stable_layer_norm=True), dict(add_adapter=True), dict(hidden_act="relu"),
                 dict(feat_extract_activation="relu"), dict(num_attention_heads=8)):
        with pytest.raises(NotImplementedError):
            SpeakerEncoder(SpeakerConfig(**dict(tiny, **over)))
    with pytest.raises(ValueError):
        SpeakerEncoder(SpeakerConfig(**tiny), attention="gated")
    for hd_heads in (4, 2, 1):  # head_dim 16, 32, 64
        SpeakerEncoder(SpeakerConfig(**dict(tiny, num_attention_heads=hd_heads)), max_batch=1, max_seconds=1.0).close()


def test_default_geometry_and_lengths(lib):
    from valle_amd.spk import PRESETS, SpeakerConfig, SpeakerEncoder

    assert PRESETS["wavlm_base_plus_sv"] == SpeakerConfig(use_weighted_layer_sum=True)
    enc = SpeakerEncoder(max_batch=1, max_seconds=1.0)
    assert enc.min_samples == 5200 == R.min_samples(enc.config)
    assert enc.num_frames(16000) == 49 == R.conv_frames(enc.config, 16000) and enc.num_frames(5200) == 16 and enc.num_frames(9) == 0
    assert enc.workspace_bytes() > 0
    enc.close()
    tiny = SpeakerEncoder(SC.config("tiny_wavlm"), max_batch=1, max_seconds=1.0)
    for L in (5200, 5201, 5519, 5520, 16000):
        assert tiny.num_frames(L) == R.conv_frames(tiny.config, L)
    tiny.close()


def test_embed_checks_before_any_hip_call(lib):
    from valle_amd import engine as e
    from valle_amd.spk import SpeakerEncoder

    name = "tiny_wavlm"
    enc = SpeakerEncoder(SC.config(name), max_batch=2, max_seconds=1.0)
    with pytest.raises(RuntimeError, match="no weights|no CPU fallback"):
        enc.embed(torch.zeros(8000))
    enc.load_state_dict(SC.state_dict(name))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.embed(torch.zeros(8000), sr=16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.cosine(torch.zeros(1, 24), torch.zeros(1, 24))
    fake = 4096  # never dereferenced: the checks come first
    with pytest.raises(e.VxError, match="5199 samples, the shortest served is 5200") as ei:
        enc._embed_raw([fake], [5199], False, fake, None)
    assert ei.value.code == 1
    with pytest.raises(e.VxError, match="16001 samples > max_samples 16000") as ei:
        enc._embed_raw([fake], [16001], False, fake, None)
    assert ei.value.code == 4
    with pytest.raises(e.VxError, match="max_batch 2") as ei:
        enc._embed_raw([fake] * 3, [8000] * 3, False, fake, None)
    assert ei.value.code == 4
    with pytest.raises(e.VxError, match="null pointer"):
        enc._embed_raw([0], [8000], False, fake, None)
    assert lib.vx_spk_embed(enc._h, 1, (C.c_void_p * 1)(fake), (C.c_int32 * 1)(8000), 2, fake, None, None) == 1  # unknown flag
    out = torch.zeros(4)
    assert lib.vx_spk_read(enc._h, b"pooled", 0, out.data_ptr(), 4) == 3  # no call yet
    enc.close()
    fresh = SpeakerEncoder(SC.config(name), max_batch=2, max_seconds=1.0)
    assert lib.vx_spk_embed(fresh._h, 1, (C.c_void_p * 1)(fake), (C.c_int32 * 1)(8000), 0, fake, None, None) == 3  # not finalized
    bad = (C.c_int32 * 3)(0, 1, 99)
    assert lib.vx_spk_set_buckets(fresh._h, bad, 3) == 1 and b"expected 2 x" in lib.vx_last_error()
    fresh.close()


def test_load_state_dict_is_strict_and_takes_both_weight_norm_layouts():
    from valle_amd.spk import SpeakerEncoder, canonical_state_dict, fold_pos_conv_weight_norm

    name = "tiny_wavlm"
    sd = SC.state_dict(name)
    enc = SpeakerEncoder(SC.config(name), max_batch=1, max_seconds=1.0)
    enc.load_state_dict(sd)  # parametrizations.weight.original0 / original1, the prefix, masked_spec_embed ignored
    g0, v0 = "wavlm.encoder.pos_conv_embed.conv.parametrizations.weight.original0", "wavlm.encoder.pos_conv_embed.conv.parametrizations.weight.original1"
    legacy = {k: v for k, v in sd.items() if k not in (g0, v0)}
    legacy["wavlm.encoder.pos_conv_embed.conv.weight_g"], legacy["wavlm.encoder.pos_conv_embed.conv.weight_v"] = sd[g0], sd[v0]
    legacy["objective.weight"] = torch.zeros(3, 24)
    a, b = canonical_state_dict(sd), canonical_state_dict(legacy)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    w = a["encoder.pos_conv_embed.conv.weight"]
    v64 = sd[v0].double()
    want = sd[g0].double() * v64 / v64.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()  # per tap, over (out, in)
    assert torch.equal(w, want.float()) and torch.equal(w, fold_pos_conv_weight_norm(sd[g0], sd[v0]))
    enc.load_state_dict(legacy)
    with pytest.raises(KeyError, match="unexpected keys \\['encoder.layers.0.attention.extra'\\]"):
        enc.load_state_dict(dict(sd, **{"wavlm.encoder.layers.0.attention.extra": torch.zeros(1)}))
    with pytest.raises(KeyError, match="missing keys \\['projector.bias'\\]"):
        enc.load_state_dict({k: v for k, v in sd.items() if k != "projector.bias"})
    with pytest.raises(KeyError, match="weight norm needs both"):
        enc.load_state_dict({k: v for k, v in sd.items() if k != g0})
    with pytest.raises(ValueError, match="tdnn.0.kernel.weight is"):
        enc.load_state_dict(dict(sd, **{"tdnn.0.kernel.weight": torch.zeros(32, 5, 32)}))
    plain = SpeakerEncoder(SC.config("tiny_plain"), attention="plain", max_batch=1, max_seconds=1.0)
    plain.load_state_dict(SC.state_dict("tiny_plain"))
    with pytest.raises(KeyError, match="gru_rel_pos"):
        plain.load_state_dict(sd)  # the wavlm-only tensors are unexpected in the plain mode
    enc.close(), plain.close()


def test_package_exports():
    import valle_amd

    for name in ("SpeakerEncoder", "SpeakerConfig", "speaker_similarity"):
        assert name in valle_amd.__all__ and getattr(valle_amd, name) is not None
    from valle_amd.codec import EncodecDecoder

    assert callable(EncodecDecoder.roundtrip_speaker_similarity)
