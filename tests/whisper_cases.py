"""The Whisper recogniser's test cases, shared by test_whisper_cpu.py and test_gpu_whisper.py: geometries, seeded weights and
waveforms, the restatement's results (computed once per case and left unchanged) and the bounds.

Bound: the project's standing rule, engine max-abs error <= TOL_FACTOR x floor, the floor being the restatement (whisper_ref) in
torch fp32 on the host against itself in fp64, per tap and per utterance.  A generated step is decided when the fp64 top-two margin
of its processed row exceeds 2 x TOL_FACTOR x the case's logits floor (both logits may move by the bound, in opposite directions);
at most EXCUSED_SHARE of the cases may contain an undecided step."""
import torch

import whisper_ref as R

TOL_FACTOR = 4.0
EXCUSED_SHARE = 0.10
WEIGHT_SEED = 0

_A = dict(num_mel_bins=80, d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, encoder_layers=2, decoder_layers=2,
          encoder_ffn_dim=256, decoder_ffn_dim=256, vocab_size=101, max_source_positions=50, max_target_positions=40)
GEOMETRIES = {
    "A": _A,
    # P = 75 crosses the encoder attention's 32-key tile twice, 72 targets take the cache across 64; proj_out is a key of its own
    "B": dict(_A, num_mel_bins=128, d_model=192, encoder_attention_heads=3, decoder_attention_heads=3, encoder_ffn_dim=384, decoder_ffn_dim=384,
              vocab_size=160, max_source_positions=75, max_target_positions=72, tie_word_embeddings=False),
    # whisper-tiny's widths, one layer each
    "C": dict(_A, d_model=384, encoder_attention_heads=6, decoder_attention_heads=6, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=1536,
              decoder_ffn_dim=1536, vocab_size=120),
    # the token loop's launcher rules through the recogniser: an FFN of 2064 is two K chunks of the skinny GEMM (2048 + 16), 300 words are
    # more than one logit a thread of the head and no multiple of 8, 260 cross keys and 264 targets take both attentions past 256 keys
    "D": dict(_A, encoder_layers=1, decoder_layers=1, decoder_ffn_dim=2064, vocab_size=300, max_source_positions=260, max_target_positions=264),
}


def special(name):
    """The ids of the special tokens: the last five of the vocabulary, as in the released ones (eos first)."""
    V = GEOMETRIES[name]["vocab_size"]
    return dict(eos=V - 5, start=V - 4, lang=V - 3, transcribe=V - 2, notimestamps=V - 1)


def config(name):
    from valle_amd.whisper import WhisperConfig

    s = special(name)
    return WhisperConfig(**dict(GEOMETRIES[name], eos_token_id=s["eos"], decoder_start_token_id=s["start"]))


def generation(name):
    """A multilingual checkpoint's generation_config.json, both suppress lists set."""
    s = special(name)
    return dict(decoder_start_token_id=s["start"], eos_token_id=s["eos"], no_timestamps_token_id=s["notimestamps"],
                lang_to_id={"<|en|>": s["lang"]}, task_to_id={"transcribe": s["transcribe"]},
                suppress_tokens=[1, 2, 7, 11, s["start"], s["lang"], s["transcribe"], s["notimestamps"]],
                begin_suppress_tokens=[3, s["eos"]])


def prompt(name, length=4):
    s = special(name)
    return {1: [s["start"]], 2: [s["start"], s["notimestamps"]], 4: [s["start"], s["lang"], s["transcribe"], s["notimestamps"]]}[length]


def vocab(name):
    """A toy byte-level vocab.json: token string -> id, the specials as <|...|>."""
    from valle_amd.whisper import bytes_to_unicode

    b2u = bytes_to_unicode()
    s = special(name)
    words = [b2u[ord(" ")] + w for w in ("the", "cat", "sat", "on", "mat", "a", "dog")] + list("abcdefghijklmnopqrstuvwxyz") + [b2u[ord(" ")], ".", ","]
    toks = {}
    for i in range(s["eos"]):
        toks[words[i] if i < len(words) else f"{b2u[ord(' ')]}w{i}"] = i
    toks.update({"<|endoftext|>": s["eos"], "<|startoftranscript|>": s["start"], "<|en|>": s["lang"], "<|transcribe|>": s["transcribe"],
                 "<|notimestamps|>": s["notimestamps"]})
    assert len(toks) == GEOMETRIES[name]["vocab_size"]
    return toks


_SD, _MEL = {}, {}


def state_dict(name, seed=WEIGHT_SEED):
    from valle_amd.whisper import synthetic_state_dict

    if (name, seed) not in _SD:
        _SD[(name, seed)] = synthetic_state_dict(config(name), seed)
    return _SD[(name, seed)]


def mel(name):
    from valle_amd.whisper import mel_filters

    n = GEOMETRIES[name]["num_mel_bins"]
    if n not in _MEL:
        _MEL[n] = mel_filters(n)
    return _MEL[n]


def chunk(name):
    return 320 * GEOMETRIES[name]["max_source_positions"]


def wave(samples, seed):
    """A seeded 16 kHz waveform of `samples` samples."""
    g = torch.Generator().manual_seed(3000 + seed)
    t = torch.arange(samples) / 16000.0
    return 0.3 * torch.randn(samples, generator=g) + 0.2 * torch.sin(2 * torch.pi * (110.0 + 7.0 * seed) * t) + 0.05


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# id -> (geometry, samples, wave seed, prompt length, max_new_tokens or None for no cap)
def _cases():
    c = {}
    ch = chunk("A")
    for i, L in enumerate((1, 199, 200, 201, 319, 320, 321, ch - 1, ch)):  # the audio lengths
        c[f"A_len{L}"] = ("A", L, i, 4, None)
    c["A_cap3"] = ("A", 9000, 20, 4, 3)          # stops on the cap
    c["A_prompt1"] = ("A", 7000, 21, 1, None)    # prompt lengths 1 and 2
    c["A_prompt2"] = ("A", 12000, 22, 2, None)
    for i in range(4):                            # B: the cache passes 31 / 32 / 33 and 63 / 64 / 65 when the utterance runs on
        c[f"B_{i}"] = ("B", (5000, 13000, 24000, 17001)[i], 30 + i, (4, 1, 2, 4)[i], None)
    c["C_0"] = ("C", 11000, 40, 4, None)
    c["C_1"] = ("C", 16000, 41, 4, 12)
    c["D_0"] = ("D", 30000, 50, 4, None)
    c["D_1"] = ("D", 83200, 51, 4, 24)
    return c


CASES = _cases()
_ENC, _GEN, _FORCED = {}, {}, {}


def case_wave(cid):
    name, L, seed, _, _ = CASES[cid]
    return wave(L, seed)


def case_prompt(cid):
    return prompt(CASES[cid][0], CASES[cid][3])


def case_max_new(cid):
    name, _, _, pl, mn = CASES[cid]
    return GEOMETRIES[name]["max_target_positions"] if mn is None else mn  # no cap: more than the positions leave


def encoded(cid, dtype, mut=()):
    key = (cid, dtype, tuple(mut))
    if key not in _ENC:
        name = CASES[cid][0]
        _ENC[key] = R.encode(state_dict(name), config(name), case_wave(cid), mel(name), dtype, mut)
    return _ENC[key]


def generated(cid, dtype=torch.float64):
    """whisper_ref.greedy of the case."""
    key = (cid, dtype)
    if key not in _GEN:
        name = CASES[cid][0]
        g, s = generation(name), special(name)
        _GEN[key] = R.greedy(state_dict(name), config(name), encoded(cid, dtype), case_prompt(cid), case_max_new(cid), g["suppress_tokens"],
                             g["begin_suppress_tokens"], s["eos"], dtype)
    return _GEN[key]


def forced(cid, dtype, mut=()):
    """The teacher-forced raw logits (count, vocab) of fp64's greedy tokens, at `dtype` (mutated, when asked)."""
    key = (cid, dtype, tuple(mut))
    if key not in _FORCED:
        name = CASES[cid][0]
        _FORCED[key] = R.forced_logits(state_dict(name), config(name), encoded(cid, dtype, mut), case_prompt(cid), generated(cid)["tokens"], dtype,
                                       mut)
    return _FORCED[key]


TAPS = ("logmel", "conv1", "features", "encoder")


def tap_names(name):
    return TAPS + tuple(f"enc{l}" for l in range(GEOMETRIES[name]["encoder_layers"] + 1)) + ("logits",)


def named_taps(cid, dtype):
    name = CASES[cid][0]
    e = encoded(cid, dtype)
    out = {k: e[k] for k in tap_names(name) if k != "logits"}
    out["logits"] = forced(cid, dtype)
    return out


def floors(cid):
    """tap name -> max-abs error of the fp32 restatement against the fp64 one."""
    r64, r32 = named_taps(cid, torch.float64), named_taps(cid, torch.float32)
    return {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64}


def decided(cid):
    """Per generated step of fp64's greedy run: the margin of the processed row exceeds 2 x TOL_FACTOR x the case's logits floor."""
    bound = 2 * TOL_FACTOR * floors(cid)["logits"]
    return [m > bound for m in generated(cid)["margins"]]


# ---- a teacher-forced run that takes the self-attention cache across 256 keys --------------------------------------------------------
# geometry, samples, wave seed, prompt length, forced tokens, token seed: 4 + 260 tokens fill D's 264 positions
TF_CASE = ("D", 40000, 60, 4, 260, 7)
_TF = {}


def tf_wave():
    return wave(TF_CASE[1], TF_CASE[2])


def tf_prompt():
    return prompt(TF_CASE[0], TF_CASE[3])


def tf_tokens():
    """Seeded tokens that are neither suppressed (either list) nor eos."""
    name, count, seed = TF_CASE[0], TF_CASE[4], TF_CASE[5]
    g = generation(name)
    ok = [t for t in range(GEOMETRIES[name]["vocab_size"]) if t not in g["suppress_tokens"] and t not in g["begin_suppress_tokens"]
          and t != special(name)["eos"]]
    pick = torch.randint(0, len(ok), (count,), generator=torch.Generator().manual_seed(seed)).tolist()
    return [ok[i] for i in pick]


def tf_taps(dtype):
    """The taps of the run at `dtype`, "logits" being the 260 raw rows teacher forcing reads."""
    if dtype not in _TF:
        name = TF_CASE[0]
        e = R.encode(state_dict(name), config(name), tf_wave(), mel(name), dtype)
        out = {k: e[k] for k in tap_names(name) if k != "logits"}
        out["logits"] = R.forced_logits(state_dict(name), config(name), e, tf_prompt(), tf_tokens(), dtype)
        _TF[dtype] = out
    return _TF[dtype]


def tf_floors():
    r64, r32 = tf_taps(torch.float64), tf_taps(torch.float32)
    return {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64}
