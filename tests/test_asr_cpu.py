"""CPU: the CTC recogniser's definition, inputs and packaging (valle_amd.asr, vx_asr_*, vx_ctc_greedy, vx_edit_distance), no GPU.

1. the restatement tests/asr_ref.py equals transformers' Wav2Vec2ForCTC and HubertForCTC in fp64 at 1e-10 relative, both flavours,
   at 1, 17 and 61 frames (skipped without the package);
2. every mutation of asr_ref.MUTATIONS moves the logits by more than 100 x the GPU test's bound at 33 frames on the GPU test's own
   inputs: the condition under which that bound can tell a wrong implementation from the definition;
3. the numpy restatements of the greedy decode and of the edit distance with S / D / I against hand-worked cases, and the edit
   distance against a full-matrix backtrace with the same preference on 300 seeded random pairs;
4. the text normalisation rule and the error rates' arithmetic;
5. the condition the GPU test relies on: in every case at most asr_cases.EXCUSED_SHARE of the frames have an fp64 top-two margin
   within 2 x TOL_FACTOR x the logits floor, and the fp32 host restatement gets the argmax of every other frame right;
6. ABI and packaging: header <=> ctypes <=> exports, the struct size, every refusal before any HIP call, load_state_dict."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import asr_cases as AC
import asr_ref as R
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


# ---- 1. the restatement against the canonical classes -----------------------------------------------------------------------------
@pytest.mark.parametrize("frames", (1, 17, 61))
@pytest.mark.parametrize("family,flavour", (("wav2vec2", "tiny_group"), ("wav2vec2", "tiny_layer"), ("hubert", "tiny_group"),
                                            ("hubert", "tiny_layer"), ("hubert", "tiny_layer_nofpn")))  # Wav2Vec2 always norms the projection's input
def test_restatement_matches_transformers(family, flavour, frames):
    tf = pytest.importorskip("transformers")
    from valle_amd.asr import RecognizerConfig, synthetic_state_dict

    fields = dict(AC.GEOMETRIES[flavour], pad_token_id=0)
    if family == "wav2vec2":
        hf_cfg, model_cls = tf.Wav2Vec2Config(**fields), tf.Wav2Vec2ForCTC
    else:
        hf_cfg, model_cls = tf.HubertConfig(**fields), tf.HubertForCTC
    cfg = RecognizerConfig.from_any(hf_cfg)  # any object with the attributes
    assert cfg == RecognizerConfig(**fields)
    sd = synthetic_state_dict(cfg, 1, prefix=family + ".")
    model = model_cls(hf_cfg).double().eval()
    res = model.load_state_dict({k: v.double() for k, v in sd.items()}, strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res
    L = R.samples_for_frames(cfg, frames) + 3
    wav = 0.5 * torch.randn(L, generator=torch.Generator().manual_seed(frames)).double()
    with torch.no_grad():
        want = model(wav[None], output_hidden_states=True)
    got = R.forward(AC.ref_state_dict(sd), cfg, wav, torch.float64)
    assert got["logits"].shape == (frames, 32)
    pairs = [("logits", want.logits[0], got["logits"])] + [(f"hidden{i}", a[0], b) for i, (a, b) in enumerate(zip(want.hidden_states, got["hidden"]))]
    assert len(want.hidden_states) == len(got["hidden"]) == 3
    for name, a, b in pairs:
        rel = float((a - b).abs().max() / a.abs().max())
        print(f"{family} {flavour} frames={frames} {name}: {rel:.2e} relative")
        assert rel <= 1e-10, (name, rel)


# ---- 2. every mutation moves the logits ------------------------------------------------------------------------------------------
def test_every_mutation_moves_the_logits():
    name, frames = "tiny_layer", 33
    r64 = AC.reference(name, frames, torch.float64)
    bound = AC.TOL_FACTOR * AC.floors(name, frames)["logits"]
    sd, cfg, wav = AC.ref_state_dict(AC.state_dict(name)), AC.config(name), AC.wave(name, frames)
    small = []
    for m in R.MUTATIONS:
        moved = float((R.forward(sd, cfg, wav, torch.float64, mutation=m)["logits"] - r64["logits"]).abs().max())
        print(f"{m:22s} moves the logits by {moved:.3e} = {moved / bound:8.1f} x the bound {bound:.3e}")
        if not moved > 100 * bound:
            small.append((m, moved / bound))
    assert not small, f"mutations within 100 x the bound: {small}"


def test_group_flavour_mutations_move_the_logits():
    name, frames = "tiny_group", 33
    r64 = AC.reference(name, frames, torch.float64)
    bound = AC.TOL_FACTOR * AC.floors(name, frames)["logits"]
    sd, cfg, wav = AC.ref_state_dict(AC.state_dict(name)), AC.config(name), AC.wave(name, frames)
    for m in ("proj_norm_skipped", "gelu_tanh"):
        moved = float((R.forward(sd, cfg, wav, torch.float64, mutation=m)["logits"] - r64["logits"]).abs().max())
        assert moved > 100 * bound, (m, moved / bound)


# ---- 3. greedy CTC and the edit distance -----------------------------------------------------------------------------------------
def _onehot(ids, V=5, hi=3.0):
    x = np.zeros((len(ids), V))
    for t, i in enumerate(ids):
        x[t, i] = hi
    return x


@pytest.mark.parametrize("ids,want,at", (
    ([1, 1, 0, 1], [1, 1], [0, 3]),              # A A _ A -> A A: repeats merged first, blanks removed second
    ([1, 1, 1], [1], [0]),                       # a run
    ([0, 0, 2, 2, 0, 0], [2], [2]),              # leading and trailing blanks
    ([0, 0, 0], [], []),                         # all blank
    ([3], [3], [0]),                             # one frame
    ([0], [], []),
    ([1, 2, 1, 2], [1, 2, 1, 2], [0, 1, 2, 3]),
    ([2, 0, 2, 2, 0, 0, 2], [2, 2, 2], [0, 2, 6]),
))
def test_ctc_greedy_by_hand(ids, want, at):
    got, frames, mean, lp = R.ctc_greedy(_onehot(ids), blank=0)
    assert got == want and frames == at
    each = 3.0 - math.log(math.exp(3.0) + 4.0)
    assert abs(mean - each) < 1e-12 and np.allclose(lp, each, atol=1e-12)


def test_ctc_greedy_ties_take_the_lowest_index():
    x = np.zeros((3, 4))
    x[0, [1, 3]] = 2.0   # a tie between 1 and 3 -> 1
    x[1, :] = 1.0        # all equal -> 0, the blank
    x[2, [2, 3]] = 5.0   # -> 2
    got, frames, _, lp = R.ctc_greedy(x, blank=0)
    assert got == [1, 2] and frames == [0, 2]
    assert abs(lp[1] + math.log(4.0)) < 1e-12
    assert R.ctc_greedy(np.zeros((0, 4)))[:3] == ([], [], 0.0)


@pytest.mark.parametrize("ref,hyp,want", (
    ("", "", (0, 0, 0, 0)),
    ("abc", "", (3, 0, 3, 0)),
    ("", "ab", (2, 0, 0, 2)),
    ("abc", "abc", (0, 0, 0, 0)),
    ("abc", "xyz", (3, 3, 0, 0)),
    ("kitten", "sitting", (3, 2, 0, 1)),
    ("ab", "b", (1, 0, 1, 0)),
    ("b", "ab", (1, 0, 0, 1)),
    ("abcd", "acd", (1, 0, 1, 0)),
    ("aa", "a", (1, 0, 1, 0)),
    ("ab", "ba", (2, 2, 0, 0)),        # two substitutions are preferred to a deletion and an insertion of the same cost
    ("abc", "ca", (3, 2, 1, 0)),
))
def test_edit_distance_by_hand(ref, hyp, want):
    assert R.edit_distance(list(ref), list(hyp)) == want


def _backtrace(ref, hyp):
    """The full matrix, then a walk back from (R, H) that prefers the diagonal, then the deletion, then the insertion."""
    Rn, Hn = len(ref), len(hyp)
    D = np.zeros((Rn + 1, Hn + 1), dtype=np.int64)
    D[:, 0], D[0, :] = np.arange(Rn + 1), np.arange(Hn + 1)
    for i in range(1, Rn + 1):
        for j in range(1, Hn + 1):
            D[i, j] = min(D[i - 1, j - 1] + (ref[i - 1] != hyp[j - 1]), D[i - 1, j] + 1, D[i, j - 1] + 1)
    i, j, s, d, n = Rn, Hn, 0, 0, 0
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + (ref[i - 1] != hyp[j - 1]):
            s += int(ref[i - 1] != hyp[j - 1]); i -= 1; j -= 1
        elif i > 0 and D[i, j] == D[i - 1, j] + 1:
            d += 1; i -= 1
        else:
            n += 1; j -= 1
    return int(D[Rn, Hn]), s, d, n


def test_edit_distance_equals_a_backtrace_on_random_pairs():
    rng = np.random.default_rng(5)
    for _ in range(300):
        a = rng.integers(0, int(rng.integers(1, 5)), int(rng.integers(0, 24))).tolist()
        b = rng.integers(0, int(rng.integers(1, 5)), int(rng.integers(0, 24))).tolist()
        got = R.edit_distance(a, b)
        assert got == _backtrace(a, b), (a, b)
        assert got[0] == got[1] + got[2] + got[3] and len(a) - got[2] + got[3] == len(b)
        assert R.edit_distance_fast(a, b) == got
    a, b = rng.integers(0, 3, 300).tolist(), rng.integers(0, 3, 257).tolist()
    assert R.edit_distance_fast(a, b) == R.edit_distance(a, b) == _backtrace(a, b)


# ---- 4. text --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,want", (
    ("Hello, world!", "HELLO WORLD"),
    ("  it's   9 o'clock -- really?  ", "IT'S 9 O'CLOCK REALLY"),
    ("", ""),
    ("...", ""),
    ("tab\tand\nnewline", "TAB AND NEWLINE"),
    ("MR. O'NEIL'S 2ND", "MR O'NEIL'S 2ND"),
))
def test_normalize_text(text, want):
    from valle_amd.asr import normalize_text

    assert normalize_text(text) == want == R.normalize_text(text)


def test_error_rate_arithmetic():
    rate, rows = R.error_rate([["A", "B", "C"], [], ["A"]], [["A", "C"], ["X"], ["A"]])
    assert rows == [(1, 0, 1, 0, 3), (1, 0, 0, 1, 0), (0, 0, 0, 0, 1)] and rate == 2 / 4
    assert math.isnan(R.error_rate([[]], [["X"]])[0])
    from valle_amd.asr import PairErrors, ids_to_text

    assert math.isnan(PairErrors(1, 0, 0, 1, 0).rate) and PairErrors(1, 0, 1, 0, 4).rate == 0.25
    v = AC.vocab("tiny_group")
    inv = {i: t for t, i in v.items()}
    ids = [v[ch] for ch in "|HI||THERE|"] + [v["<unk>"]]
    assert ids_to_text(ids, inv, "|", ("<pad>", "<s>", "</s>", "<unk>")) == "HI THERE"


# ---- 5. the GPU test's condition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frames", AC.all_cases())
def test_margins_decide_nearly_every_frame(name, frames):
    ids64, decided = AC.decided_frames(name, frames)
    excused = int((~decided).sum())
    print(f"{name}_T{frames}: {excused} of {frames} frames excused, logits floor {AC.floors(name, frames)['logits']:.3e}")
    assert excused <= AC.EXCUSED_SHARE * frames
    ids32 = AC.reference(name, frames, torch.float32)["logits"].argmax(1)
    assert torch.equal(ids32[decided], ids64[decided])


# ---- 6. ABI and packaging -------------------------------------------------------------------------------------------------------
NAMES = ["vx_asr_create", "vx_asr_destroy", "vx_asr_finalize", "vx_asr_frames", "vx_asr_get_timings", "vx_asr_min_samples", "vx_asr_read",
         "vx_asr_recognize", "vx_asr_set_weight", "vx_ctc_greedy", "vx_edit_distance"]


def test_header_ctypes_exports(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = sorted(set(re.findall(r"\b(vx_(?:asr|ctc|edit)_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == NAMES
    assert declared == [s for s in engine.declared_symbols() if s.startswith(("vx_asr_", "vx_ctc_", "vx_edit_"))]
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in vallex.h but not exported"
    from valle_amd import engine as e

    assert C.sizeof(e.VxAsrConfig) == 180  # 45 four-byte fields, as the header lays them out


def _struct(name="tiny_group", **over):
    from valle_amd.asr import SpeechRecognizer

    rec = SpeechRecognizer(AC.config(name), AC.vocab(name), max_batch=2, max_seconds=1.0)
    s = rec._config_struct()
    rec.close()
    for k, v in over.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("over,code,match", (
    (dict(struct_size=0), 1, b"struct_size"),
    (dict(blank=32), 1, b"blank 32"),
    (dict(add_adapter=1), 5, b"add_adapter"),
    (dict(conv_pos_batch_norm=1), 5, b"conv_pos_batch_norm"),
    (dict(activation=1), 5, b"activation"),
    (dict(feat_extract_norm=1), 5, b"feat_extract_norm = 1 with do_stable_layer_norm = 0"),
    (dict(do_stable_layer_norm=1), 5, b"feat_extract_norm = 0 with do_stable_layer_norm = 1"),
    (dict(feat_extract_norm=1, do_stable_layer_norm=1), 5, b"conv_bias"),
    (dict(heads=8), 5, b"head_dim = 8"),
    (dict(max_batch=65), 5, b"max_batch"),
    (dict(max_samples=399), 1, b"400"),
))
def test_create_refusals_without_gpu(lib, over, code, match):
    s = _struct(**over)
    h = C.c_void_p()
    assert lib.vx_asr_create(C.byref(s), C.byref(h)) == code
    assert match in lib.vx_last_error(), lib.vx_last_error()
    assert not h.value


def test_python_refusals_name_the_field():
    from valle_amd.asr import RecognizerConfig, SpeechRecognizer

    tiny, v = AC.GEOMETRIES["tiny_group"], AC.vocab("tiny_group")
    for over, field in ((dict(add_adapter=True), "add_adapter"), (dict(conv_pos_batch_norm=True), "conv_pos_batch_norm"),
                        (dict(hidden_act="relu"), "hidden_act"), (dict(feat_extract_activation="relu"), "feat_extract_activation"),
                        (dict(num_attention_heads=8), "head_dim"), (dict(feat_extract_norm="layer"), "do_stable_layer_norm"),
                        (dict(do_stable_layer_norm=True), "feat_extract_norm")):
        with pytest.raises(NotImplementedError, match=field):
            SpeechRecognizer(RecognizerConfig(**dict(tiny, **over)), v)
    with pytest.raises(ValueError, match="blank"):
        SpeechRecognizer(RecognizerConfig(**tiny), {"A": 0})
    for name in ("tiny_group", "tiny_layer", "tiny_layer_nofpn", "hd64_layer"):
        SpeechRecognizer(AC.config(name), AC.vocab(name), max_batch=1, max_seconds=1.0).close()


def test_lengths_and_checks_before_any_hip_call(lib, tmp_path):
    import json

    from valle_amd import engine as e
    from valle_amd.asr import RecognizerConfig, SpeechRecognizer

    path = tmp_path / "config.json"
    path.write_text(json.dumps(dict(AC.GEOMETRIES["tiny_layer"], model_type="hubert", architectures=["HubertForCTC"])))
    assert RecognizerConfig.from_any(str(path)) == AC.config("tiny_layer")
    rec = SpeechRecognizer(str(path), AC.vocab("tiny_layer"), max_batch=2, max_seconds=1.0)
    assert rec.min_samples == 400 == R.samples_for_frames(rec.config, 1) and rec.blank_id == 0
    for L in (399, 400, 719, 720, 16000):
        assert rec.num_frames(L) == R.conv_frames(rec.config, L)
    assert rec.num_frames(16000) == 49 and rec.workspace_bytes() > 0
    with pytest.raises(RuntimeError, match="no weights|no CPU fallback"):
        rec.recognize(torch.zeros(8000))
    rec.load_state_dict(AC.state_dict("tiny_layer"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rec.recognize(torch.zeros(8000), sr=16000)
    fake = 4096  # never dereferenced: the checks come first
    with pytest.raises(e.VxError, match="399 samples, the shortest served is 400") as ei:
        rec._recognize_raw([fake], [399], False, fake, fake, fake, fake, None)
    assert ei.value.code == 1
    with pytest.raises(e.VxError, match="16001 samples > max_samples 16000") as ei:
        rec._recognize_raw([fake], [16001], False, fake, fake, fake, fake, None)
    assert ei.value.code == 4
    with pytest.raises(e.VxError, match="max_batch 2") as ei:
        rec._recognize_raw([fake] * 3, [8000] * 3, False, fake, fake, fake, fake, None)
    assert ei.value.code == 4
    out = torch.zeros(4)
    assert lib.vx_asr_read(rec._h, b"logits", 0, out.data_ptr(), 4) == 3  # no call yet
    with pytest.raises(KeyError, match="missing keys \\['lm_head.bias'\\]"):
        rec.load_state_dict({k: v for k, v in AC.state_dict("tiny_layer").items() if k != "lm_head.bias"})
    with pytest.raises(KeyError, match="unexpected keys"):
        rec.load_state_dict(AC.state_dict("tiny_layer_nofpn") | {"wav2vec2.feature_projection.layer_norm.extra": torch.zeros(1)})
    rec.close()
    # the decode and the distance refuse before any HIP call too
    one = (C.c_int32 * 1)
    assert lib.vx_ctc_greedy(fake, 4, 4, 1, one(3), fake, fake, fake, fake, None, None) == 1 and b"blank 4" in lib.vx_last_error()
    assert lib.vx_ctc_greedy(fake, 4, 0, 1, one(-1), fake, fake, fake, fake, None, None) == 1
    assert lib.vx_edit_distance(1, fake, one(2049), fake, one(1), fake, None) == 1 and b"up to 2048 tokens" in lib.vx_last_error()
    assert lib.vx_edit_distance(1, fake, one(1), fake, one(-1), fake, None) == 1
    assert lib.vx_edit_distance(0, fake, one(1), fake, one(1), fake, None) == 1


def test_package_exports():
    import valle_amd

    for name in ("SpeechRecognizer", "RecognizerConfig", "edit_distance", "word_error_rate", "char_error_rate", "recognition_error"):
        assert name in valle_amd.__all__ and getattr(valle_amd, name) is not None
    from valle_amd.codec import EncodecDecoder

    assert callable(EncodecDecoder.roundtrip_wer)
