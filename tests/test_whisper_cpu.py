"""No GPU: what the Whisper recogniser's GPU tests stand on.

1. the restatement (whisper_ref.py) in fp64 against `transformers`: the mel table, WhisperFeatureExtractor's features, the encoder's
   last_hidden_state, teacher-forced logits and generate(do_sample=False) ids with both suppress lists set, on geometries A, B, C
   and D, relative bound 1e-10, the measured figures printed.  Measured here: mel table 4.5e-16, encoder 1e-15 .. 1e-14, logits 1e-15 ..
   1e-14, ids equal.  The features equal the extractor's own lines (its spectrogram asked for fp64 output) to 3.6e-15 once the
   restatement takes the one step in which the extractor differs from the definition: transformers.audio_utils.spectrogram stores the
   STFT as complex64 between its fp64 FFT and its fp64 power (whisper_ref.logmel(stft_complex64=True)).  Without that step, which is
   the yardstick the GPU tests use, the two differ by 8.8e-9 .. 9.8e-9: an fp32-grade rounding of the STFT and nothing else.  The
   extractor's fp32 output agrees to 1.3e-6.  The model comparisons feed the restatement's own features to both sides.
2. deliberate mistakes: each of whisper_ref.MUTATIONS moves the teacher-forced logits of a GPU case by at least 10 x the GPU bound,
   so that no engine inside the bound can carry one.  Measured ratios (movement / bound, the smaller of cases A_len321 and B_1):
   k_bias 4.2e4, q_unscaled 2.3e5, post_norm 3.4e5, tanh_gelu 5.9e1, no_decoder_positions 2.7e5, conv2_shifted 2.3e4, natural_log
   8.5e4, no_clamp 6.8e4, drop_first_frame 2.3e4, cross_before_final_norm 3.1e5, no_causal_mask 1.7e5, begin_suppress_always inf
   (an entry of the processed row goes to -inf).  `k_bias` is the form in which a bias lands on k in an engine that stacks q | k | v
   into one GEMM: the checkpoint's two bias vectors laid onto the first two projections, k taking v's and v left without.  A bias
   added to k and nothing else cannot be seen by any test (q . b is the same for every key and softmax is invariant to it: 4.1e-10 x
   the bound, rounding), which test_a_bias_on_k_alone_is_invisible records.
3. the cases of the GPU test: stops, distinct tokens, decided steps (none excused), asserted of the fp32 restatement alone.
4. the byte decoder, the prefix, the C ABI and every refusal before any HIP call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import whisper_cases as WC
import whisper_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-10
HF_CASES = ("A_len16000", "A_prompt1", "A_len201", "B_1", "B_3", "C_0", "C_1", "D_0", "D_1")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from valle_amd import engine

    ge.build()
    return engine.load_library()


# ---- 1. the restatement against transformers --------------------------------------------------------------------------------------
_HF = {}


def _hf_model(name):
    tf = pytest.importorskip("transformers")
    if name not in _HF:
        s = WC.special(name)
        cfg = tf.WhisperConfig(**WC.GEOMETRIES[name], eos_token_id=s["eos"], decoder_start_token_id=s["start"], pad_token_id=s["eos"],
                               bos_token_id=s["eos"], suppress_tokens=None, begin_suppress_tokens=None)
        m = tf.WhisperForConditionalGeneration(cfg).double().eval()
        m.load_state_dict({k: v.double() for k, v in WC.state_dict(name).items()}, strict=True)
        _HF[name] = m
    return _HF[name]


def _extractor(name):
    tf = pytest.importorskip("transformers")
    fe = tf.WhisperFeatureExtractor(feature_size=WC.GEOMETRIES[name]["num_mel_bins"], sampling_rate=16000, hop_length=160, chunk_length=1, n_fft=400)
    fe.n_samples = WC.chunk(name)  # the chunk of 320 P samples
    fe.nb_max_frames = fe.n_samples // 160
    return fe


@pytest.mark.parametrize("name", list(WC.GEOMETRIES))
def test_mel_table_is_transformers(name):
    au = pytest.importorskip("transformers.audio_utils")
    n = WC.GEOMETRIES[name]["num_mel_bins"]
    want = au.mel_filter_bank(201, n, 0.0, 8000.0, 16000, norm="slaney", mel_scale="slaney").T
    err = float(np.abs(WC.mel(name).numpy() - want).max() / np.abs(want).max())
    print(f"mel table {n}: relative error {err:.3e}")
    assert err <= REL
    assert np.array_equal(_extractor(name).mel_filters.T, want)


def test_features_match_the_feature_extractor():
    au = pytest.importorskip("transformers.audio_utils")
    worst, worst_pure = 0.0, 0.0
    for cid in HF_CASES:
        name = WC.CASES[cid][0]
        fe, wav = _extractor(name), WC.case_wave(cid)
        P = WC.GEOMETRIES[name]["max_source_positions"]
        pure = WC.encoded(cid, torch.float64)["logmel"]
        as_extractor = R.logmel(wav, P, WC.mel(name), torch.float64, stft_complex64=True)
        f32 = fe(wav.numpy(), sampling_rate=16000, return_tensors="pt").input_features[0].T
        # the extractor's own lines (_np_extract_fbank_features) with its spectrogram asked for fp64 output
        x = np.zeros(fe.n_samples)
        x[:wav.numel()] = wav.double().numpy()
        ls = au.spectrogram(x, au.window_function(fe.n_fft, "hann"), frame_length=fe.n_fft, hop_length=fe.hop_length, power=2.0,
                            mel_filters=fe.mel_filters, log_mel="log10", dtype=np.float64)[:, :-1]
        ls = torch.from_numpy((np.maximum(ls, ls.max() - 8.0) + 4.0) / 4.0).T
        e64 = float((ls - as_extractor).abs().max() / ls.abs().max())
        e_pure = float((ls - pure).abs().max() / ls.abs().max())
        e32 = float((f32.double() - as_extractor).abs().max() / ls.abs().max())
        print(f"{cid} features: relative error {e64:.3e} with the extractor's complex64 STFT, {e_pure:.3e} without it (the yardstick), "
              f"{e32:.3e} against the extractor's fp32 output")
        assert f32.shape == pure.shape and e32 <= 4e-6  # its output: the last lines in fp32 on values up to 10 (ulp 9.5e-7), a few roundings
        worst, worst_pure = max(worst, e64), max(worst_pure, e_pure)
    assert worst <= REL
    assert worst_pure <= 1e-7  # the complex64 step is an fp32-grade rounding of the STFT and nothing more


@pytest.mark.parametrize("cid", HF_CASES)
def test_restatement_matches_transformers(cid):
    tf = pytest.importorskip("transformers")
    name = WC.CASES[cid][0]
    m, g, s = _hf_model(name), WC.generation(name), WC.special(name)
    e, want, prompt = WC.encoded(cid, torch.float64), WC.generated(cid), WC.case_prompt(cid)
    feats = e["logmel"].T[None]
    with torch.no_grad():
        enc = m.model.encoder(input_features=feats).last_hidden_state[0]
        e_enc = float((enc - e["encoder"]).abs().max() / e["encoder"].abs().max())
        ids = prompt + want["tokens"][:-1]
        lg = m(input_features=feats, decoder_input_ids=torch.tensor([ids])).logits[0][len(prompt) - 1:]
        mine = WC.forced(cid, torch.float64)
        e_lg = float((lg - mine).abs().max() / mine.abs().max())
        k = min(WC.case_max_new(cid), WC.GEOMETRIES[name]["max_target_positions"] - len(prompt))
        out = tf.generation.GenerationMixin.generate(m, feats, decoder_input_ids=torch.tensor([prompt]), do_sample=False, max_new_tokens=k,
                                                     suppress_tokens=g["suppress_tokens"], begin_suppress_tokens=g["begin_suppress_tokens"],
                                                     eos_token_id=s["eos"], pad_token_id=s["eos"])[0].tolist()
    print(f"{cid}: encoder {e_enc:.3e}, teacher-forced logits {e_lg:.3e}, {len(want['tokens'])} generated ids")
    assert e_enc <= REL and e_lg <= REL
    assert out == prompt + want["tokens"]


# ---- 2. deliberate mistakes ----------------------------------------------------------------------------------------------------------
MUT_CASES = ("A_len321", "B_1")  # audio shorter than the chunk: the clamp binds on the padded frames


def _mutation_ratio(cid, mut):
    name = WC.CASES[cid][0]
    bound = WC.TOL_FACTOR * WC.floors(cid)["logits"]
    base = WC.forced(cid, torch.float64)
    if mut == "begin_suppress_always":  # a mistake of the processed row: the raw logits do not move, the rows the argmax reads do
        g = WC.generation(name)
        rows = [(R.process_row(r, i, g["suppress_tokens"], g["begin_suppress_tokens"]),
                 R.process_row(r, i, g["suppress_tokens"], g["begin_suppress_tokens"], mut=(mut,))) for i, r in enumerate(base)]
        moved = max(float("inf") if bool((torch.isinf(a) != torch.isinf(b)).any()) else 0.0 for a, b in rows[1:])
    else:
        moved = float((WC.forced(cid, torch.float64, (mut,)) - base).abs().max())
    return moved / bound


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mistake_moves_the_logits(mut):
    for cid in MUT_CASES:
        ratio = _mutation_ratio(cid, mut)
        print(f"{mut} on {cid}: moves the teacher-forced logits by {ratio:.3e} x the GPU bound")
        assert ratio >= 10.0


def test_a_bias_on_k_alone_is_invisible():
    """Why `k_bias` is modelled as the packing slip (k takes v's bias, v loses it): a bias added to k and nothing else adds q . b to
    every score of a query, the same number for every key, and softmax is invariant to it, so no test of any output can see it."""
    for cid in MUT_CASES:
        ratio = _mutation_ratio(cid, "k_bias_only")
        print(f"k_bias_only on {cid}: moves the teacher-forced logits by {ratio:.3e} x the GPU bound")
        assert ratio <= 1e-6


# ---- 3. the GPU test's cases -----------------------------------------------------------------------------------------------------------
def test_case_selection():
    gens = {cid: WC.generated(cid) for cid in WC.CASES}
    eos_steps = {len(g["tokens"]) for g in gens.values() if g["stop"] == R.STOP_EOS}
    stops = [g["stop"] for g in gens.values()]
    distinct = set(t for g in gens.values() for t in g["tokens"])
    print(f"eos at steps {sorted(eos_steps)}, {stops.count(R.STOP_MAX_NEW)} on the cap, {stops.count(R.STOP_MAX_TARGET)} on max_target_positions, "
          f"{len(distinct)} distinct tokens")
    assert len(eos_steps) >= 3 and stops.count(R.STOP_MAX_NEW) >= 1 and stops.count(R.STOP_MAX_TARGET) >= 1 and len(distinct) >= 8
    for name in ("A", "B"):  # every prompt length, and on B a cache that runs past 65 positions
        assert {WC.CASES[c][3] for c in WC.CASES if WC.CASES[c][0] == name} >= {1, 2, 4}
    assert max(len(WC.case_prompt(c)) + len(gens[c]["tokens"]) for c in WC.CASES if WC.CASES[c][0] == "B") == 72
    for cid, g in gens.items():  # the eos of a run is its last token and nowhere else; the suppressed tokens never appear
        name = WC.CASES[cid][0]
        gc, eos = WC.generation(name), WC.special(name)["eos"]
        assert eos not in g["tokens"][:-1] and (g["tokens"][-1] == eos) == (g["stop"] == R.STOP_EOS)
        assert not set(g["tokens"]) & set(gc["suppress_tokens"]) and g["tokens"][0] not in gc["begin_suppress_tokens"]


def test_margins_decide_every_step():
    excused = []
    for cid in WC.CASES:
        dec, g64 = WC.decided(cid), WC.generated(cid)
        floor = WC.floors(cid)["logits"]
        print(f"{cid}: smallest margin {min(g64['margins']):.3e}, logits floor {floor:.3e}, {dec.count(False)} undecided steps")
        if False in dec:
            excused.append(cid)
            continue
        g32 = WC.generated(cid, torch.float32)  # the fp32 restatement alone satisfies what the GPU test asks of the engine
        assert g32["tokens"] == g64["tokens"] and g32["stop"] == g64["stop"]
    assert len(excused) <= WC.EXCUSED_SHARE * len(WC.CASES), excused


# ---- 4. text, prefix, ABI --------------------------------------------------------------------------------------------------------------
def test_byte_decoder_inverts_bytes_to_unicode():
    from valle_amd.whisper import bytes_to_unicode, decode_tokens

    mine = bytes_to_unicode()
    try:
        from transformers.models.gpt2.tokenization_gpt2 import bytes_to_unicode as theirs
        assert mine == theirs()
    except ImportError:
        pass
    assert len(mine) == 256 == len(set(mine.values()))
    for text in ("hello world", " naïve café", "日本語", "a\nb\tc", "🙂"):
        s = "".join(mine[b] for b in text.encode("utf-8"))
        toks = {i: ch for i, ch in enumerate(s)}  # one token per byte
        assert decode_tokens(list(range(len(s))), toks, len(s)) == text
    inv = {0: mine[0xE6], 1: mine[0x97] + mine[0xA5], 2: "x", 3: "<|endoftext|>"}
    assert decode_tokens([0, 1, 2, 3], inv, 3) == "日x"          # a character split over two tokens; the special id dropped
    assert decode_tokens([0, 2], inv, 3) == "�x"            # a torn character decodes with errors="replace"
    v = WC.vocab("A")
    assert decode_tokens([0, 1, 2, v["<|endoftext|>"]], {i: t for t, i in v.items()}, WC.special("A")["eos"]) == " the cat sat"


def test_prefix_construction():
    from valle_amd.whisper import WhisperRecognizer

    s = WC.special("A")
    multi = WhisperRecognizer(WC.config("A"), None, WC.generation("A"))
    assert multi.prompt_prefix("en", "transcribe") == [s["start"], s["lang"], s["transcribe"], s["notimestamps"]] == WC.prompt("A", 4)
    assert multi.prompt_prefix("<|en|>") == WC.prompt("A", 4)
    with pytest.raises(ValueError, match="language"):
        multi.prompt_prefix("xx")
    with pytest.raises(ValueError, match="task"):
        multi.prompt_prefix("en", "translate")
    en_only = {k: v for k, v in WC.generation("A").items() if k not in ("lang_to_id", "task_to_id")}
    assert WhisperRecognizer(WC.config("A"), None, en_only).prompt_prefix() == [s["start"], s["notimestamps"]] == WC.prompt("A", 2)
    assert WhisperRecognizer(WC.config("A")).prompt_prefix() == [s["start"]]


NAMES = ["vx_wsp_create", "vx_wsp_destroy", "vx_wsp_finalize", "vx_wsp_get_timings", "vx_wsp_read", "vx_wsp_recognize", "vx_wsp_set_suppress",
         "vx_wsp_set_weight"]
OP_NAMES = ["vx_op_wsp_decode_attn", "vx_op_wsp_embed", "vx_op_wsp_gemm", "vx_op_wsp_head"]


def test_header_ctypes_exports(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = sorted(set(re.findall(r"\b(vx_wsp_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == NAMES
    assert declared == [s for s in engine.declared_symbols() if s.startswith("vx_wsp_")]
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in vallex.h but not exported"
    assert C.sizeof(engine.VxWspConfig) == 68  # 17 four-byte fields, as the header lays them out
    ops = sorted(set(re.findall(r"\b(vx_op_wsp_[a-z0-9_]+)\s*\(", hdr)))  # the token loop's kernels on caller data
    assert ops == OP_NAMES == [s for s in engine.declared_symbols() if s.startswith("vx_op_wsp_")]
    for name in ops:
        assert hasattr(lib, name), f"{name} declared in vallex.h but not exported"


def _struct(**over):
    from valle_amd.whisper import WhisperRecognizer

    rec = WhisperRecognizer(WC.config("A"), max_batch=2)
    s = rec._config_struct()
    rec.close()
    for k, v in over.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("over,code,match", (
    (dict(struct_size=0), 1, b"struct_size"),
    (dict(eos_token_id=101), 1, b"eos_token_id 101"),
    (dict(max_target_positions=1), 1, b"max_target_positions 1"),
    (dict(activation=1), 5, b"activation_function"),
    (dict(enc_heads=4), 5, b"encoder head_dim = 128 / 4"),
    (dict(dec_heads=1), 5, b"decoder head_dim = 128 / 1"),
    (dict(n_mels=81), 5, b"num_mel_bins = 81"),
    (dict(max_batch=65), 5, b"max_batch"),
    (dict(max_source_positions=5000), 5, b"max_source_positions 5000"),
))
def test_create_refusals_without_gpu(lib, over, code, match):
    s = _struct(**over)
    h = C.c_void_p()
    assert lib.vx_wsp_create(C.byref(s), C.byref(h)) == code
    assert match in lib.vx_last_error(), lib.vx_last_error()
    assert not h.value


def test_python_refusals_name_the_field():
    from valle_amd.whisper import WhisperConfig, WhisperRecognizer

    a = dict(WC.GEOMETRIES["A"], eos_token_id=96, decoder_start_token_id=97)
    for over, field in ((dict(activation_function="relu"), "activation_function"), (dict(encoder_attention_heads=4), "encoder head_dim"),
                        (dict(decoder_attention_heads=1), "decoder head_dim")):
        with pytest.raises(NotImplementedError, match=field):
            WhisperRecognizer(WhisperConfig(**dict(a, **over)))
    with pytest.raises(ValueError, match="mel_basis"):
        WhisperRecognizer(WC.config("A"), mel_basis=torch.zeros(80, 200))
    for name in WC.GEOMETRIES:
        WhisperRecognizer(WC.config(name), WC.vocab(name), WC.generation(name), max_batch=1).close()


def test_lengths_and_checks_before_any_hip_call(lib, tmp_path):
    import json

    from valle_amd import engine as e
    from valle_amd.whisper import WhisperConfig, WhisperRecognizer

    path, gpath = tmp_path / "config.json", tmp_path / "generation_config.json"
    s = WC.special("A")
    path.write_text(json.dumps(dict(WC.GEOMETRIES["A"], eos_token_id=s["eos"], decoder_start_token_id=s["start"], model_type="whisper")))
    gpath.write_text(json.dumps(WC.generation("A")))
    assert WhisperConfig.from_any(str(path)) == WC.config("A")
    rec = WhisperRecognizer(str(path), WC.vocab("A"), str(gpath), max_batch=2)
    assert rec.config.chunk_samples == 16000 and rec.workspace_bytes() > 0 and rec.eos_token_id == s["eos"]
    with pytest.raises(RuntimeError, match="no weights|no CPU fallback"):
        rec.recognize(torch.zeros(8000))
    rec.load_state_dict(WC.state_dict("A"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rec.recognize(torch.zeros(8000), sr=16000)
    fake = 4096  # never dereferenced: the checks come first
    p4 = WC.prompt("A", 4)

    def raw(lengths, prompts, max_new, forced=None, stride=8):
        rec._recognize_raw([fake] * len(lengths), lengths, prompts, max_new, forced, stride, fake, fake, fake, fake)

    for args, code, match in (
            (([16001], [p4], [4]), 4, "n_samples = 16001 > the chunk of 16000 samples"),
            (([-1], [p4], [4]), 1, "n_samples = -1"),
            (([100], [[]], [4]), 1, "empty prompt_ids"),
            (([100], [[s["start"]] * 40], [4]), 4, "prompt_ids of 40 tokens leave no room under max_target_positions = 40"),
            (([100], [[101]], [4]), 1, r"prompt_ids\[0\] = 101"),
            (([100], [p4], [0]), 1, "max_new_tokens = 0"),
            (([100], [p4], [9]), 1, "max_new_tokens = 9 outside \\[1, out_stride = 8\\]"),
            (([100] * 3, [p4] * 3, [4] * 3), 4, "max_batch 2"),
            (([100], [p4], [2], [[5, 101]]), 1, "forced token 1 is id 101"),
            (([100], [p4 * 9], [8], [[5] * 8]), 4, "8 forced tokens after a prompt of 36 exceed max_target_positions = 40"),
    ):
        with pytest.raises(e.VxError, match=match) as ei:
            raw(*args)
        assert ei.value.code == code, args
    out = torch.zeros(4)
    assert lib.vx_wsp_read(rec._h, b"logmel", 0, out.data_ptr(), 4) == 3  # no call yet
    with pytest.raises(KeyError, match="missing keys \\['model.encoder.conv1.bias'\\]"):
        rec.load_state_dict({k: v for k, v in WC.state_dict("A").items() if k != "model.encoder.conv1.bias"})
    with pytest.raises(KeyError, match="unexpected keys \\['model.encoder.layers.0.self_attn.k_proj.bias'\\]"):
        rec.load_state_dict(WC.state_dict("A") | {"model.encoder.layers.0.self_attn.k_proj.bias": torch.zeros(128)})
    with pytest.raises(ValueError, match="model.decoder.embed_positions.weight is \\(41, 128\\)"):
        rec.load_state_dict(WC.state_dict("A") | {"model.decoder.embed_positions.weight": torch.zeros(41, 128)})
    with pytest.raises(KeyError, match="missing keys \\['proj_out.weight'\\]"):  # an untied checkpoint needs its own head
        WhisperRecognizer(WC.config("B")).load_state_dict({k: v for k, v in WC.state_dict("B").items() if k != "proj_out.weight"})
    assert lib.vx_wsp_set_suppress(rec._h, (C.c_int32 * 1)(5), 1, None, 0) == 3  # finalized
    rec.close()
    with pytest.raises(e.VxError, match="begin_suppress_tokens\\[0\\] = 101"):
        WhisperRecognizer(WC.config("A"), None, dict(WC.generation("A"), begin_suppress_tokens=[101]))


def test_package_exports():
    import valle_amd

    for name in ("WhisperRecognizer", "WhisperConfig", "WhisperTranscript"):
        assert name in valle_amd.__all__ and getattr(valle_amd, name) is not None
    from valle_amd.whisper import synthetic_state_dict

    sd = synthetic_state_dict(WC.config("B"), 3)
    assert "proj_out.weight" in sd and sd["proj_out.weight"].data_ptr() != sd["model.decoder.embed_tokens.weight"].data_ptr()
