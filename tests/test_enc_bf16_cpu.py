"""CPU: the restatement of the recognisers' bf16 encoder mode (enc_bf16_ref) and the cases the GPU tests compare on
(enc_bf16_cases), vetted on the host alone; and everything of the mode that is decided before any HIP call.

1. the rounding restatement is the unrounded one when nothing is rounded, and in fp32 it is the same function as in fp64 (their
   distance is far below the rounding's own effect);
2. the floors (rounding restatement in fp32 against the unrounded fp64) are printed per case and tap;
3. the conditions on the cases: at least 70 % of the Whisper steps and 60 % of the CTC frames are decided under the bf16 bound, every
   case has a decided one, at least six Whisper cases are decided at every step;
4. which of whisper_ref's and asr_ref's deliberate mistakes still exceed the bf16 bound (recorded; the tanh GELU does not - the fp32
   mode keeps pinning the semantics);
5. the refusals, without a GPU: flags, flavours, head dimensions, widths, `precision=`; the plan shrinks and the weights halve."""
import ctypes as C

import pytest
import torch

import asr_cases as AC
import asr_ref
import enc_bf16_cases as EC
import enc_bf16_ref as ER
import whisper_cases as WC
import whisper_ref


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from valle_amd import engine

    ge.build()
    return engine.load_library()


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------
def test_without_roundings_it_is_the_unrounded_restatement(monkeypatch):
    monkeypatch.setattr(ER, "rb", lambda x: x)
    cid = "C_0"
    name = WC.CASES[cid][0]
    base = WC.encoded(cid, torch.float64)
    got = ER.whisper_encode(WC.state_dict(name), WC.config(name), base, torch.float64)
    for k in ("enc1", "encoder"):
        assert float((got[k] - base[k]).abs().max()) <= 1e-12, k
    name, frames = "hd64_layer", 65
    base = AC.reference(name, frames, torch.float64)
    got = ER.asr_forward(AC.ref_state_dict(AC.state_dict(name)), AC.config(name), base, torch.float64)
    assert float((got["logits"] - base["logits"]).abs().max()) <= 1e-11
    for a, b in zip(got["hidden"], base["hidden"]):
        assert float((a - b).abs().max()) <= 1e-11


def test_rounding_is_nearest_even():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0e38], dtype=torch.float64)
    assert ER.rb(x).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, float(torch.tensor(-3.0e38).to(torch.bfloat16))]


# ---- 2. / 3. floors and decisions -----------------------------------------------------------------------------------------------------
def test_whisper_floors_and_decided_share():
    steps = decided = 0
    full = []
    for cid in WC.CASES:
        f16, f32 = EC.wsp_floors(cid), WC.floors(cid)
        dec = EC.wsp_decided(cid)
        steps, decided = steps + len(dec), decided + sum(dec)
        print(f"{cid}: encoder floor bf16 {f16['encoder']:.2e} (fp32 {f32['encoder']:.2e}), logits floor bf16 {f16['logits']:.2e} "
              f"(fp32 {f32['logits']:.2e}), {sum(dec)} of {len(dec)} steps decided")
        assert f16["logits"] > 100 * f32["logits"], "the roundings are what the floor measures"
        assert any(dec), f"{cid} has no decided step"
        if all(dec):
            full.append(cid)
        # the roundings are in the encoder layers and nowhere else
        for tap in ("logmel", "conv1", "features", "enc0"):
            assert f16[tap] == f32[tap], tap
    print(f"{decided} of {steps} steps decided ({decided / steps:.0%}); fully decided: {full}")
    assert decided >= EC.WHISPER_DECIDED_SHARE * steps
    assert len(full) >= EC.FULLY_DECIDED_CASES, full


def test_fully_decided_cases_decode_alike_in_the_restatement():
    """What the GPU test asks of the engine on the fully decided cases, asked of the rounding restatement in fp32 first."""
    for cid in WC.CASES:
        if not all(EC.wsp_decided(cid)):
            continue
        name = WC.CASES[cid][0]
        g, s = WC.generation(name), WC.special(name)
        got = whisper_ref.greedy(WC.state_dict(name), WC.config(name), EC.wsp_encoded(cid, torch.float32), WC.case_prompt(cid), WC.case_max_new(cid),
                                 g["suppress_tokens"], g["begin_suppress_tokens"], s["eos"], torch.float32)
        want = WC.generated(cid)
        assert got["tokens"] == want["tokens"] and got["stop"] == want["stop"], cid


def test_whisper_teacher_forced_run_floors():
    f16, f32 = EC.wsp_tf_floors(), WC.tf_floors()
    print(f"D_tf260: encoder floor bf16 {f16['encoder']:.2e} (fp32 {f32['encoder']:.2e}), logits floor bf16 {f16['logits']:.2e} (fp32 {f32['logits']:.2e})")
    assert f16["logits"] > 100 * f32["logits"]


def test_ctc_floors_and_decided_share():
    frames = decided = 0
    for name, T in EC.ASR_CASES:
        f16, f32 = EC.asr_floors(name, T), AC.floors(name, T)
        want, dec = EC.asr_decided_frames(name, T)
        frames, decided = frames + T, decided + int(dec.sum())
        print(f"{name} x {T}: logits floor bf16 {f16['logits']:.2e} (fp32 {f32['logits']:.2e}), {int(dec.sum())} of {T} frames decided")
        assert f16["logits"] > 100 * f32["logits"]
        assert bool(dec.any()), f"{name} x {T} has no decided frame"
        for tap in ("conv0", "features", "hidden0"):
            assert f16[tap] == f32[tap], tap
        got = EC.asr_reference(name, T, torch.float32)["logits"].argmax(1)
        assert torch.equal(got[dec], want[dec]), "the rounding restatement in fp32 decides the decided frames as fp64 does"
    print(f"{decided} of {frames} frames decided ({decided / frames:.0%})")
    assert decided >= EC.CTC_DECIDED_SHARE * frames


# ---- 4. the deliberate mistakes under the bf16 bound ----------------------------------------------------------------------------------
def test_which_mistakes_the_bf16_bound_still_sees():
    cid = "A_len16000"
    bound = EC.TOL_FACTOR * EC.wsp_floors(cid)["logits"]
    base = WC.forced(cid, torch.float64)
    seen = {}
    for mut in whisper_ref.MUTATIONS:
        try:
            moved = float((WC.forced(cid, torch.float64, (mut,)) - base).abs().max())
        except RuntimeError:  # a mistake that changes the step count has no teacher-forced rows to compare
            continue
        seen[mut] = moved / bound
        print(f"whisper {mut}: moves the logits by {seen[mut]:.2f} x the bf16 bound")
    assert seen["tanh_gelu"] < 1.0 < max(seen.values())
    name, T = "hd64_layer", 65
    bound = EC.TOL_FACTOR * EC.asr_floors(name, T)["logits"]
    base = AC.reference(name, T, torch.float64)["logits"]
    sd, cfg, wav = AC.ref_state_dict(AC.state_dict(name)), AC.config(name), AC.wave(name, T)
    seen = {}
    for mut in asr_ref.MUTATIONS:
        seen[mut] = float((asr_ref.forward(sd, cfg, wav, torch.float64, mutation=mut)["logits"] - base).abs().max()) / bound
        print(f"ctc {mut}: moves the logits by {seen[mut]:.2f} x the bf16 bound")
    assert seen["gelu_tanh"] < 1.0 < max(seen.values())


# ---- 5. before any HIP call -----------------------------------------------------------------------------------------------------------
def _wsp_struct(name="A", **over):
    from valle_amd.whisper import WhisperRecognizer

    rec = WhisperRecognizer(WC.config(name), max_batch=2, precision="bf16")
    s = rec._config_struct()
    rec.close()
    for k, v in over.items():
        setattr(s, k, v)
    return s


def _asr_struct(name, **over):
    from valle_amd.asr import SpeechRecognizer

    rec = SpeechRecognizer(AC.config(name), AC.vocab(name), max_batch=2, max_seconds=1.0)
    s = rec._config_struct()
    rec.close()
    for k, v in over.items():
        setattr(s, k, v)
    return s


def test_flags_and_constants(lib):
    from valle_amd import engine as e

    assert (e.VX_WSP_KEEP_TAPS, e.VX_WSP_ENC_BF16, e.VX_ASR_KEEP_TAPS, e.VX_ASR_ENC_BF16) == (1, 2, 1, 2)
    assert _wsp_struct().flags == e.VX_WSP_ENC_BF16
    assert C.sizeof(e.VxWspConfig) == 68 and C.sizeof(e.VxAsrConfig) == 180  # no struct changed its size
    for name in ("vx_op_enc16_gemm", "vx_op_enc16_add_ln", "vx_op_enc16_attn"):
        assert hasattr(lib, name) and name in e.declared_symbols()


@pytest.mark.parametrize("over,code,match", (
    (dict(flags=4), 1, b"flags = 4"),
    (dict(flags=7), 1, b"flags = 7"),
    (dict(enc_ffn=272), 5, b"encoder_ffn_dim"),   # a multiple of 16, which the fp32 mode serves, and no multiple of 64
    (dict(enc_heads=4), 5, b"encoder head_dim = 128 / 4"),
))
def test_whisper_create_refusals(lib, over, code, match):
    s = _wsp_struct(**over)
    h = C.c_void_p()
    assert lib.vx_wsp_create(C.byref(s), C.byref(h)) == code
    assert match in lib.vx_last_error(), lib.vx_last_error()
    assert not h.value
    if "enc_ffn" in over:  # the fp32 mode still serves it
        s.flags = 0
        assert lib.vx_wsp_create(C.byref(s), C.byref(h)) == 0
        lib.vx_wsp_destroy(h)


@pytest.mark.parametrize("name,over,code,match", (
    ("hd64_layer", dict(flags=4), 1, b"flags = 4"),
    ("hd64_group", dict(flags=2), 5, b"do_stable_layer_norm"),   # group / post-norm
    ("base2", dict(flags=2), 5, b"do_stable_layer_norm"),        # wav2vec2-base's flavour
    ("tiny_layer", dict(flags=2), 5, b"head_dim 64, not hidden / heads = 64 / 4"),        # head_dim 16
    ("tiny_layer", dict(flags=2, heads=2), 5, b"head_dim 64, not hidden / heads = 64 / 2"),  # head_dim 32
    ("hd64_layer", dict(flags=2, ffn=160), 5, b"ffn in multiples of 64, not 160"),
))
def test_ctc_create_refusals(lib, name, over, code, match):
    s = _asr_struct(name, **over)
    h = C.c_void_p()
    assert lib.vx_asr_create(C.byref(s), C.byref(h)) == code
    assert match in lib.vx_last_error(), lib.vx_last_error()
    assert not h.value


def test_python_precision_argument():
    from valle_amd.asr import SpeechRecognizer
    from valle_amd.engine import VxError
    from valle_amd.whisper import WhisperRecognizer

    for bad in ("fp16", "bf16 ", None, "fp8"):
        with pytest.raises(ValueError, match="precision"):
            WhisperRecognizer(WC.config("A"), precision=bad)
        with pytest.raises(ValueError, match="precision"):
            SpeechRecognizer(AC.config("hd64_layer"), AC.vocab("hd64_layer"), precision=bad)
    assert WhisperRecognizer(WC.config("A")).precision == "fp32" and SpeechRecognizer(AC.config("hd64_layer"), AC.vocab("hd64_layer")).precision == "fp32"
    with pytest.raises(VxError, match="do_stable_layer_norm") as ei:
        SpeechRecognizer(AC.config("hd64_group"), AC.vocab("hd64_group"), precision="bf16")
    assert ei.value.code == 5
    with pytest.raises(VxError, match="head_dim 64") as ei:
        SpeechRecognizer(AC.config("tiny_layer"), AC.vocab("tiny_layer"), precision="bf16")
    assert ei.value.code == 5
    for name in WC.GEOMETRIES:  # every test geometry is served, B's d = 192 included
        WhisperRecognizer(WC.config(name), WC.vocab(name), WC.generation(name), max_batch=1, precision="bf16").close()
    for name in ("hd64_layer", "large2"):
        SpeechRecognizer(AC.config(name), AC.vocab(name), max_batch=1, max_seconds=1.0, precision="bf16").close()


def test_workspace_and_weight_bytes_follow_the_mode():
    """Host only: the plan is made at create and the packing at finalize.  The mode's rows (LN output, q | k | v, attention output, FFN
    inner) take half the bytes, and so do the four matrices of every encoder layer."""
    from valle_amd import engine as e
    from valle_amd.whisper import WhisperRecognizer

    out = {}
    for prec in ("fp32", "bf16"):
        rec = WhisperRecognizer(WC.config("C"), WC.vocab("C"), WC.generation("C"), max_batch=2, state_dict=WC.state_dict("C"), precision=prec)
        t = (C.c_double * 4)()
        e._check(e.load_library().vx_wsp_get_timings(rec._handle(), t, 4))
        out[prec] = (int(t[1]), int(t[2]))
        rec.close()
    g = WC.GEOMETRIES["C"]
    d, ffn, P, L = g["d_model"], g["encoder_ffn_dim"], g["max_source_positions"], g["encoder_layers"]
    rows = 2 * P * (d + 3 * d + d + ffn)   # elements of the four row buffers at max_batch 2
    mats = L * (4 * d * d + 2 * d * ffn)   # elements of the four matrices
    print(f"workspace {out['fp32'][0]} -> {out['bf16'][0]} bytes, weights {out['fp32'][1]} -> {out['bf16'][1]} bytes")
    assert out["fp32"][0] - out["bf16"][0] == 2 * rows
    assert abs((out["fp32"][1] - out["bf16"][1]) - 2 * mats) <= 64 * L  # alignment padding of the packed blocks
