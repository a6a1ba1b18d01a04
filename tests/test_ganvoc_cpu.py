"""No GPU: the HiFi-GAN / BigVGAN generator's restatement (tests/ganvoc_ref.py), the host side of the C ABI (vx_gan_*) and the
Python surface of valle_amd.ganvoc.

* the leaky-ReLU mode of the restatement equals `transformers.SpeechT5HifiGan` in fp64 within 1e-10, and that model's state dict
  (weight norm applied) loads through `GanVocoder.load_state_dict`;
* the anti-aliased activation: the 12 taps are the Kaiser-sinc formula's and the C side's, the fused polyphase form the kernel uses
  equals the pad / conv_transpose / crop / act / pad / strided-conv composition, an identity activation passes a slow sinusoid;
* every deliberately wrong restatement moves the output by far more than the GPU test's bound (the inputs tell them apart);
* weight-norm folding, the loader's accepted forms and refusals, the C ABI's names, struct size and refusals in their order."""
import ctypes as C
import os
import re

import pytest
import torch

import ganvoc_ref as GR
from conftest import ROOT

NAMES = {"vx_gan_create", "vx_gan_destroy", "vx_gan_set_weight", "vx_gan_set_filter", "vx_gan_get_filter", "vx_gan_finalize",
         "vx_gan_samples", "vx_gan_synthesize"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


# ---- 1. the restatement against an independent implementation ----------------------------------------------------------------
def _speecht5(rates, kernels, C0, rks, dils, normalize_before, seed):
    tf = pytest.importorskip("transformers")
    cfg = tf.SpeechT5HifiGanConfig(model_in_dim=100, upsample_initial_channel=C0, upsample_rates=list(rates),
                                   upsample_kernel_sizes=list(kernels), resblock_kernel_sizes=list(rks),
                                   resblock_dilation_sizes=[list(d) for d in dils], leaky_relu_slope=0.1,
                                   normalize_before=normalize_before)
    torch.manual_seed(seed)
    m = tf.SpeechT5HifiGan(cfg).double().eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():  # the default initialisation (std 0.01) gives an almost constant output: a poor test signal
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.1)
            else:
                fan = p.shape[1] * p.shape[2] if "upsampler" not in name else p.shape[0] * 2
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) / fan ** 0.5)
        m.mean.copy_(torch.randn(100, generator=g, dtype=torch.float64) - 4.0)
        m.scale.copy_(torch.rand(100, generator=g, dtype=torch.float64) + 1.5)
    m.apply_weight_norm()
    with torch.no_grad():  # a gain that is not the direction's norm, so that the fold is not the identity
        for name, p in m.named_parameters():
            if name.endswith("weight_g") or name.endswith("original0"):
                p.mul_(torch.rand(p.shape, generator=g, dtype=torch.float64) + 0.5)
    ours = dict(n_mels=100, rates=tuple(rates), kernels=tuple(kernels), initial_channels=C0, resblock_kernels=tuple(rks),
                dilations=tuple(tuple(d) for d in dils), activation="lrelu", alpha_logscale=False, lrelu_slope=0.1)
    return m, ours


@pytest.mark.parametrize("normalize_before", (False, True))
@pytest.mark.parametrize("rates,kernels,C0", (((4, 2), (8, 4), 32), ((8, 2), (16, 4), 16)))
def test_lrelu_mode_equals_speecht5_hifigan(rates, kernels, C0, normalize_before):
    from valle_amd.ganvoc import GanVocoder, canonical_state_dict

    m, cfg = _speecht5(rates, kernels, C0, (3, 7), ((1, 3, 5), (1, 2, 4)), normalize_before, seed=5)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    w, taps = canonical_state_dict(sd, None)
    assert taps is None
    # the fold in fp64, before its rounding to fp32, is what the model computes
    w64 = {}
    for k, v in sd.items():
        k2 = re.sub(r"^upsampler\.", "ups.", k)
        if k2.endswith("weight_g") or k2.endswith("original0"):
            base = re.sub(r"\.(weight_g|parametrizations\.weight\.original0)$", "", k2)
            vv = sd[k.replace("weight_g", "weight_v").replace("original0", "original1")]
            w64[base + ".weight"] = v * vv / vv.reshape(vv.shape[0], -1).norm(dim=1).reshape(-1, 1, 1)
        elif not (k2.endswith("weight_v") or k2.endswith("original1")):
            w64[k2] = v
    if not normalize_before:  # the buffers exist but the model does not apply them
        w64.pop("mean"), w64.pop("scale")
    assert set(w) - {"mean", "scale"} == set(w64) - {"mean", "scale"}
    for T in (1, 2, 9):
        mel = GR.logmel(T).double()
        with torch.no_grad():
            want = m(mel)
        got = GR.forward(w64, cfg, mel, torch.float64)
        assert want.shape == got.shape == (T * GR.hop(cfg),)
        assert float((want - got).abs().max()) <= 1e-10, (T, float((want - got).abs().max()))
    for k in w64:  # the loader's fold, rounded to fp32 once
        assert torch.equal(w[k], w64[k].float()), k
    # the model's own config carries normalize_before: its buffers are applied exactly when the model applies them
    v = GanVocoder(m.config)
    assert v.config.normalize_before is normalize_before and v.config.lrelu_slope == 0.1 and tuple(v.config.rates) == tuple(rates)
    assert v.load_state_dict(sd) is v and set(v._weights) == set(w64) and ("mean" in v._weights) is normalize_before
    v.close()
    v = GanVocoder(cfg)  # a dict without the flag: mean / scale are applied when they are there
    assert v.load_state_dict(sd) is v and "mean" in v._weights and "scale" in v._weights
    v.close()


# ---- 2. the anti-aliased activation -----------------------------------------------------------------------------------------
def test_filter_is_the_formula_and_the_c_sides(lib):
    from valle_amd.ganvoc import GanVocoder

    f = GR.kaiser_sinc_filter()
    assert f.shape == (12,) and abs(float(f.sum()) - 1.0) < 1e-15 and float((f - f.flip(0)).abs().max()) < 1e-16
    # written out: I0 by its series, beta from the attenuation formula
    import math

    A = 2.285 * 5 * math.pi * 1.2 + 7.95
    assert A > 50.0  # 51.02: the first branch of the attenuation rule
    beta = 0.1102 * (A - 8.7)

    def i0(x):
        s, t = 1.0, 1.0
        for k in range(1, 60):
            t *= (x / (2 * k)) ** 2
            s += t
        return s

    g = []
    for n in range(12):
        r = 2.0 * n / 11 - 1.0
        t = 0.5 * (n - 6 + 0.5)
        g.append(0.5 * i0(beta * math.sqrt(1 - r * r)) / i0(beta) * math.sin(math.pi * t) / (math.pi * t))
    g = torch.tensor(g, dtype=torch.float64)
    assert float((g / g.sum() - f).abs().max()) < 1e-14
    v = GanVocoder(GR.GEOMETRIES["g1_snakebeta"])
    assert torch.equal(v.filter, f.float())  # fp64 on both sides, rounded once
    v.close()


@pytest.mark.parametrize("L", list(range(1, 14)) + [40])
def test_polyphase_form_equals_the_composition(L):
    g = torch.Generator().manual_seed(L)
    x = torch.randn((5, L), generator=g, dtype=torch.float64) * 2.0
    a = torch.rand(5, generator=g, dtype=torch.float64) + 0.5
    b = torch.rand(5, generator=g, dtype=torch.float64) + 0.5
    f = GR.kaiser_sinc_filter()
    for aa, bb in ((a, b), (a, a), (None, None)):
        d = float((GR.aa_act(x, f, aa, bb) - GR.aa_act_polyphase(x, f, aa, bb)).abs().max())
        assert d <= 1e-12, (L, d)
    # the wrong restatements differ from it (at L = 1 the shifted crop and a replicate pad of a constant cannot show)
    for variant in ("zero_pad", "drop_tap") + (("crop_shift",) if L > 1 else ()):
        assert float((GR.aa_act(x, f, a, b, variant) - GR.aa_act(x, f, a, b)).abs().max()) > 1e-4, variant


def test_identity_activation_passes_a_slow_sinusoid():
    """Up by 2 and down by 2 through the same low-pass: a sinusoid far below the cutoff (0.01 cycles per sample against 0.25 of the
    2x rate) comes back within the filter's pass-band ripple, away from the replicate-padded ends."""
    f = GR.kaiser_sinc_filter()
    n = torch.arange(400, dtype=torch.float64)
    x = torch.sin(2 * torch.pi * 0.01 * n)[None]
    y = GR.aa_act(x, f, None, None)
    H = lambda w: float((f * torch.cos(w * (torch.arange(12, dtype=torch.float64) - 5.5))).sum())  # the symmetric filter's gain
    gain = H(2 * torch.pi * 0.005) ** 2  # at the 2x rate the tone sits at 0.005; its image at 0.495 is in the stop band
    assert abs(gain - 1.0) < 2e-3
    assert float((y - x)[0, 12:-12].abs().max()) < 3e-3
    assert float((y - gain * x)[0, 12:-12].abs().max()) < 2e-3


# ---- 3. the test inputs tell the wrong restatements apart -------------------------------------------------------------------
APPLIES = {"g1_snakebeta": GR.VARIANTS,
           "g2_snake": ("zero_pad", "drop_tap", "crop_shift", "dilation_1", "p_off_by_one", "no_mean"),
           "g3_lrelu": ("dilation_1", "p_off_by_one", "no_mean")}


@pytest.mark.parametrize("name", sorted(GR.GEOMETRIES))
def test_every_mutation_moves_the_output(name):
    """At T = 33 every wrong restatement that applies to the geometry (all eight on g1; no beta, no exp on g2; no anti-aliased
    activation on g3) moves the fp64 output by at least 100 x the GPU test's bound, 4 x the fp32 floor.  None is left out."""
    cfg = GR.GEOMETRIES[name]
    w, mel = GR.make_weights(cfg, 1), GR.logmel(33)
    y64 = GR.forward(w, cfg, mel, torch.float64)
    floor = float((GR.forward(w, cfg, mel, torch.float32).double() - y64).abs().max())
    peak = float(GR.pre_tanh(w, cfg, mel).abs().max())
    assert 1.0 < peak < 2.0 and 0.0 < floor < 1e-5
    short = []
    for v in GR.VARIANTS:
        d = float((GR.forward(w, cfg, mel, torch.float64, variant=v) - y64).abs().max())
        print(f"{name} {v}: moves {d:.3e} = {d / GR.tolerance(floor):.0f} x the bound")
        if v in APPLIES[name]:
            if d < 100 * GR.tolerance(floor):
                short.append((v, d))
        else:
            assert d == 0.0, v
    assert not short, short


# ---- 4. weight norm and the loader -------------------------------------------------------------------------------------------
def test_weight_norm_fold_matches_torch():
    from valle_amd.ganvoc import fold_weight_norm

    torch.manual_seed(2)
    for mod in (torch.nn.Conv1d(6, 10, 7), torch.nn.ConvTranspose1d(8, 4, 16, stride=8)):
        m = torch.nn.utils.parametrizations.weight_norm(mod.double())
        with torch.no_grad():
            m.parametrizations.weight.original0.mul_(1.7)
        want = m.weight.detach()
        got = fold_weight_norm(m.parametrizations.weight.original0, m.parametrizations.weight.original1)
        assert got.dtype == torch.float32 and got.shape == want.shape
        # one rounding to fp32 of a value that agrees with torch's fold to fp64 accuracy
        assert bool(((got.double() - want).abs() <= 2.0 ** -24 * 1.0001 * want.abs()).all())


def _bigvgan_style(cfg, w, form):
    """The canonical weights under BigVGAN's key layout, weight norm as `form`."""
    sd = {}
    for k, t in w.items():
        k2 = re.sub(r"^ups\.(\d+)\.", r"ups.\1.0.", k)
        k2 = re.sub(r"\.(alpha|beta)$", r".act.\1", k2)
        if k2.endswith(".weight") and form != "plain":
            v = t.double() * 3.0
            g = t.double().reshape(t.shape[0], -1).norm(dim=1).reshape(-1, 1, 1)
            gk, vk = ("weight_g", "weight_v") if form == "gv" else ("parametrizations.weight.original0",
                                                                      "parametrizations.weight.original1")
            sd[k2[:-6] + gk], sd[k2[:-6] + vk] = g, v
        else:
            sd[k2] = t.clone()
    return sd


@pytest.mark.parametrize("form", ("plain", "gv", "param"))
def test_loader_accepts_the_three_weight_forms(form):
    from valle_amd.ganvoc import BigVGAN

    cfg = GR.GEOMETRIES["g1_snakebeta"]
    w = GR.make_weights(cfg, 1)
    sd = _bigvgan_style(cfg, w, form)
    f = GR.kaiser_sinc_filter().float()
    sd["resblocks.0.activations.0.upsample.filter"] = f.reshape(1, 1, 12).clone()
    sd["resblocks.0.activations.0.downsample.lowpass.filter"] = f.reshape(1, 1, 12).clone()
    v = BigVGAN(cfg, state_dict={"generator": sd})  # the checkpoint wrapper is unwrapped
    assert set(v._weights) == set(w)
    for k in w:
        if form == "plain" or not k.endswith(".weight"):
            assert torch.equal(v._weights[k], w[k]), k
        else:  # g v / |v| in fp64 returns the weight within an fp32 rounding
            assert float((v._weights[k] - w[k]).abs().max()) <= 1.2e-7 * float(w[k].abs().max()), k
    assert torch.equal(v._taps, f) and torch.equal(v.filter, f)
    v.close()


def test_loader_refusals():
    from valle_amd.ganvoc import BigVGAN, GanVocoder

    cfg = GR.GEOMETRIES["g1_snakebeta"]
    w = GR.make_weights(cfg, 1)
    v = GanVocoder(cfg)
    sd = _bigvgan_style(cfg, w, "plain")
    gone = dict(sd)
    gone.pop("resblocks.1.convs2.0.bias"), gone.pop("activation_post.act.beta")
    with pytest.raises(KeyError, match=r"missing keys \['activation_post.beta', 'resblocks.1.convs2.0.bias'\]"):
        v.load_state_dict(gone)
    with pytest.raises(KeyError, match=r"unexpected keys \['resblocks.9.convs1.0.weight'\]"):
        v.load_state_dict(dict(sd, **{"resblocks.9.convs1.0.weight": torch.zeros(1)}))
    with pytest.raises(ValueError, match="conv_pre.weight is"):
        v.load_state_dict(dict(sd, **{"conv_pre.weight": torch.zeros(24, 100, 5)}))
    with pytest.raises(KeyError, match="weight norm needs both"):
        v.load_state_dict(dict(sd, **{"conv_pre.weight_g": torch.zeros(24, 1, 1)}))
    f = GR.kaiser_sinc_filter().float().reshape(1, 1, 12)
    with pytest.raises(ValueError, match="differ from one another"):
        v.load_state_dict(dict(sd, **{"resblocks.0.activations.0.upsample.filter": f,
                                      "resblocks.0.activations.1.downsample.lowpass.filter": f * 1.001}))
    with pytest.raises(ValueError, match="taps"):
        v.load_state_dict(dict(sd, **{"activation_post.upsample.filter": torch.ones(1, 1, 8) / 8}))
    with pytest.raises(KeyError, match="mean and scale"):
        v.load_state_dict(dict(sd, mean=torch.zeros(100)))
    assert v._weights is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.load_state_dict(sd)(GR.logmel(2))
    v.close()
    with pytest.raises(ValueError, match="unknown preset"):
        GanVocoder("bigvgan_v9")
    with pytest.raises(ValueError, match="leaky-ReLU"):
        BigVGAN("hifigan_v1_256")
    with pytest.raises(ValueError, match="activation"):
        GanVocoder(dict(cfg, activation="gelu"))


def test_presets_and_config_json():
    from valle_amd.ganvoc import PRESETS, BigVGAN, GanConfig, GanVocoder

    assert set(PRESETS) == {"bigvgan_24khz_100band", "bigvgan_base_24khz_100band", "hifigan_v1_256"}
    for name, hopv, C0, act in (("bigvgan_24khz_100band", 256, 1536, "snakebeta"), ("bigvgan_base_24khz_100band", 256, 512, "snakebeta"),
                                ("hifigan_v1_256", 256, 512, "lrelu")):
        v = GanVocoder(name)
        assert (v.hop, v.config.initial_channels, v.config.activation, v.config.n_mels) == (hopv, C0, act, 100)
        assert v.num_samples(7) == 7 * 256 and v.num_samples(0) == 0
        v.close()
    # a checkpoint's own config.json overrides the presets: the generator's field names are understood
    js = {"num_mels": 80, "upsample_rates": [5, 4], "upsample_kernel_sizes": [11, 8], "upsample_initial_channel": 64,
          "resblock_kernel_sizes": [3, 5], "resblock_dilation_sizes": [[1, 2], [2, 6]], "activation": "snake", "snake_logscale": False,
          "resblock": "1", "sampling_rate": 24000}
    v = BigVGAN(js)
    assert isinstance(v.config, GanConfig) and (v.hop, v.config.n_mels, v.config.activation, v.config.alpha_logscale) == (20, 80, "snake", False)
    v.close()
    js.pop("activation"), js.pop("snake_logscale")
    v = BigVGAN(js)
    assert (v.config.activation, v.config.alpha_logscale) == ("snakebeta", True)
    v.close()


# ---- 5. the C ABI -------------------------------------------------------------------------------------------------------------
def _config(kw=None):
    from valle_amd.engine import VxGanConfig

    kw = kw or {}
    c = VxGanConfig()
    c.struct_size = C.sizeof(VxGanConfig)
    c.n_mels, c.n_stages, c.initial_channels, c.n_resblocks, c.n_dilations = 100, 2, 24, 2, 2
    c.rates[0], c.rates[1], c.kernels[0], c.kernels[1] = 2, 2, 4, 4
    c.resblock_kernels[0], c.resblock_kernels[1] = 3, 7
    for r in range(2):
        c.dilations[r][0], c.dilations[r][1] = 1, 3
    c.activation, c.alpha_logscale, c.lrelu_slope, c.max_batch, c.max_total_frames = 2, 1, 0.1, 4, 100
    for k, v in kw.items():
        if isinstance(k, tuple):
            arr = getattr(c, k[0])
            if len(k) == 3:
                arr[k[1]][k[2]] = v
            else:
                arr[k[1]] = v
        else:
            setattr(c, k, v)
    return c


def test_symbols_and_struct_size(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = set(re.findall(r"\b(vx_[a-z0-9_]+)\s*\(", hdr))
    assert {n for n in declared if n.startswith("vx_gan_")} == NAMES
    assert {n for n in engine.declared_symbols() if n.startswith("vx_gan_")} == NAMES
    assert all(hasattr(lib, n) for n in NAMES)
    assert C.sizeof(engine.VxGanConfig) == 188  # 47 four-byte fields, as the header declares them
    assert [f[0] for f in engine.VxGanConfig._fields_] == [
        "struct_size", "n_mels", "n_stages", "rates", "kernels", "initial_channels", "n_resblocks", "resblock_kernels", "n_dilations",
        "dilations", "activation", "alpha_logscale", "lrelu_slope", "max_batch", "max_total_frames"]
    body = re.search(r"typedef struct vx_gan_config \{(.*?)\} vx_gan_config;", hdr, re.S).group(1)
    fields = re.findall(r"(?:int32_t|float)\s+([a-z_]+)((?:\[\d+\])*);", body)
    assert [f[0] for f in fields] == [f[0] for f in engine.VxGanConfig._fields_]
    n = 0
    for _, dims in fields:
        k = 1
        for d in re.findall(r"\[(\d+)\]", dims):
            k *= int(d)
        n += k
    assert 4 * n == 188


def test_create_refusals(lib):
    h = C.c_void_p()
    assert lib.vx_gan_create(C.byref(_config()), None) == 1
    assert lib.vx_gan_create(None, C.byref(h)) == 1
    cases = (({"struct_size": 0}, 1), ({"struct_size": 184}, 1), ({"max_batch": 0}, 1), ({"max_total_frames": 0}, 1), ({"n_mels": 0}, 1),
             ({"n_stages": 0}, 1), ({"n_stages": 9}, 1), ({"n_resblocks": 0}, 1), ({"n_resblocks": 5}, 1), ({"n_dilations": 0}, 1),
             ({"n_dilations": 5}, 1), ({("rates", 1): 0}, 1), ({("kernels", 0): 0}, 1), ({("resblock_kernels", 1): 0}, 1),
             ({("dilations", 1, 1): 0}, 1), ({"initial_channels": 0}, 1), ({"activation": 3}, 1), ({"activation": -1}, 1),
             ({"alpha_logscale": 2}, 1), ({"lrelu_slope": float("nan")}, 1), ({"lrelu_slope": float("inf")}, 1),
             # well-formed, not built
             ({("kernels", 0): 1}, 5),            # k < u
             ({("kernels", 1): 5}, 5),            # k - u odd: no symmetric padding
             ({("resblock_kernels", 0): 4}, 5),   # an even resblock kernel
             ({"initial_channels": 26}, 5),       # no multiple of 2^2
             ({"max_batch": 65}, 5), ({"max_total_frames": 2 ** 21 + 1}, 5),
             ({"n_stages": 8, **{("rates", i): 4 for i in range(8)}, **{("kernels", i): 8 for i in range(8)}, "initial_channels": 512}, 5),
             # in order: an argument error is reported before what is unsupported
             ({("kernels", 0): 1, "max_batch": 0}, 1))
    for kw, code in cases:
        assert lib.vx_gan_create(C.byref(_config(kw)), C.byref(h)) == code, kw
        assert lib.vx_last_error()
    for kw in ({}, {"activation": 0}, {"activation": 1, "alpha_logscale": 0}, {("kernels", 0): 2}, {("kernels", 1): 6}, {"max_batch": 64}):
        assert lib.vx_gan_create(C.byref(_config(kw)), C.byref(h)) == 0, kw
        lib.vx_gan_destroy(h)
    lib.vx_gan_destroy(None)


def test_weights_filter_and_samples(lib):
    h = C.c_void_p()
    assert lib.vx_gan_create(C.byref(_config()), C.byref(h)) == 0
    assert lib.vx_gan_samples(h, 7) == 28 and lib.vx_gan_samples(h, 0) == 0 and lib.vx_gan_samples(h, -2) == 0
    assert lib.vx_gan_samples(None, 7) == 0 and lib.vx_gan_samples(h, 2 ** 40) == 2 ** 42
    buf = torch.zeros(24 * 100 * 7)

    def put(key, shape):
        s = (C.c_int64 * len(shape))(*shape)
        return lib.vx_gan_set_weight(h, key, buf.data_ptr(), s, len(shape))

    assert put(b"conv_pre.weight", (24, 100, 7)) == 0
    assert put(b"conv_pre.weight", (24, 100, 5)) == 6 and b"expected (24, 100, 7)" in lib.vx_last_error()
    assert put(b"conv_pre.weight", (24, 700)) == 6
    assert put(b"vocoder.weight", (1,)) == 6 and b"unknown key" in lib.vx_last_error()
    assert lib.vx_gan_set_weight(h, None, buf.data_ptr(), (C.c_int64 * 1)(1), 1) == 1
    assert lib.vx_gan_set_filter(h, buf.data_ptr(), 8) == 5 and lib.vx_gan_set_filter(h, None, 12) == 1
    assert lib.vx_gan_finalize(h) == 6 and b"missing tensor" in lib.vx_last_error()
    one = (C.c_void_p * 1)(8)
    T = (C.c_int32 * 1)(4)
    assert lib.vx_gan_synthesize(h, 1, one, T, one, None) == 3  # not finalized
    lib.vx_gan_destroy(h)


def test_synthesize_refusals_before_any_hip_call(lib):
    """A handle that never saw a device: every refusal comes back in the header's order without a HIP call; valid arguments then
    fail at the first HIP call when there is no GPU, and leave the handle usable."""
    from valle_amd.engine import VxError
    from valle_amd.ganvoc import GanVocoder

    cfg = GR.GEOMETRIES["g1_snakebeta"]
    v = GanVocoder(cfg, state_dict=GR.make_weights(cfg, 1), max_batch=2, max_total_frames=50)

    def code_of(mels, T, wavs=None):
        with pytest.raises(VxError) as e:
            v._synthesize_raw(mels, T, wavs or [8] * len(mels))
        return e.value.code

    assert code_of([8], [-1]) == 1                 # a negative frame count
    assert code_of([0], [4]) == 1                  # null input
    assert code_of([8], [4], wavs=[0]) == 1        # null output
    assert code_of([8, 8, 8], [4] * 3) == 4        # n > max_batch
    assert code_of([8, 8], [4, -1]) == 1           # every utterance is checked
    assert code_of([8, 8], [30, 21]) == 4          # 51 frames > max_total_frames
    assert code_of([8], [51]) == 4
    assert code_of([8, 0], [51, 4]) == 4           # in order: the capacity of utterance 0 before the null of utterance 1
    h = v._h
    assert lib.vx_gan_synthesize(h, 0, None, None, None, None) == 1
    assert lib.vx_gan_synthesize(None, 1, None, None, None, None) == 1
    one, T = (C.c_void_p * 1)(8), (C.c_int32 * 1)(4)
    assert lib.vx_gan_synthesize(h, 0, one, T, one, None) == 1
    v._synthesize_raw([0, 0], [0, 0], [0, 0])      # no frame at all: nothing to do, no pointer looked at
    buf = torch.zeros(4)
    assert lib.vx_gan_set_weight(h, b"conv_pre.bias", buf.data_ptr(), (C.c_int64 * 1)(24), 1) == 3  # after finalize
    assert lib.vx_gan_set_filter(h, buf.data_ptr(), 12) == 3
    if not torch.cuda.is_available():
        for _ in range(2):  # the first HIP call fails; the handle is as before and fails the same way again
            assert code_of([8], [4]) == 2
        assert code_of([8], [-1]) == 1
    v.close()


def test_exports():
    import valle_amd

    for n in ("GanVocoder", "BigVGAN"):
        assert n in valle_amd.__all__ and callable(getattr(valle_amd, n))
    from valle_amd.ganvoc import GanVocoder

    assert valle_amd.GanVocoder is GanVocoder
