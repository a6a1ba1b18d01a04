"""CTC speech recogniser on the GPU: `transformers`' `Wav2Vec2ForCTC` / `HubertForCTC` behind `vx_asr_*` (include/vallex.h,
csrc/asr_kernels.hpp on top of the speaker encoder's kernels), its greedy decode, and the word / character error rate of a
transcript against the text that was to be said, with the edit distance on the device; there is no CPU fallback.

    from valle_amd import SpeechRecognizer, recognition_error
    rec = SpeechRecognizer("ckpt/config.json", json.load(open("ckpt/vocab.json")), state_dict=torch.load("ckpt/pytorch_model.bin")).to("cuda")
    hyp = rec.recognize([synth_wav], sr=24000)[0]          # .text, .tokens, .frames (x 20 ms), .logprob
    wer = recognition_error(text, synth_wav, rec, sr=24000)  # ErrorRate: .rate, .pairs[0].substitutions / .deletions / .insertions

Two flavours, chosen by the checkpoint's config: group / post-norm (`wav2vec2-base-960h`, HuBERT base) and layer / stable
(`hubert-large-ls960-ft`, `wav2vec2-large-960h-lv60-self`).  The definition is stated in include/vallex.h and restated in fp64 in
tests/asr_ref.py, which tests/test_asr_cpu.py pins against the two `transformers` classes.  Nothing has been recognised on trained
weights: no checkpoint is available where this is built, and on synthetic weights the error rate means nothing.  The S / D / I
counts are those of the stated tie-break (match or substitution, then deletion, then insertion); only their sum, the distance,
is independent of it, so parity with another aligner's counts (jiwer's, say) is by definition only.

A text that is already known is scored and placed against the same logits (`vx_falign`, csrc/falign_kernels.hpp): the CTC
likelihood `-log p(text | audio)` by the forward algorithm, and per character and word the frames of the best path
(`torchaudio.functional.forced_align`'s rule; that package is not a dependency, so parity with its tie-break is by definition only):

    al = rec.align([synth_wav], [text], sr=24000)[0]         # TextAlignment: .words[i] = (word, start_s, end_s, score), .chars, .nll
    nll = text_likelihood(text, synth_wav, rec)[0].nll_per_char"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import re
from typing import Dict, List, NamedTuple, Optional, Sequence, Union

import torch

from . import engine as _e
from ._speech_handle import SAMPLE_RATE, W2vHandle, config_from_any, w2v_backbone_keys, w2v_synthetic_state_dict
from .spk import canonical_state_dict as _canonical

HEAD_DIMS = (16, 32, 64)
EDIT_MAX_LEN = 2048  # tokens per side of a pair (csrc/asr_kernels.hpp)
FALIGN_MAX_TARGETS = 1000  # target tokens per utterance of an alignment (csrc/falign_kernels.hpp)


@dataclasses.dataclass
class RecognizerConfig:
    """The fields of `Wav2Vec2Config` / `HubertConfig` the network reads, under their names and with `Wav2Vec2Config()`'s defaults."""
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    conv_dim: Sequence[int] = (512, 512, 512, 512, 512, 512, 512)
    conv_kernel: Sequence[int] = (10, 3, 3, 3, 3, 2, 2)
    conv_stride: Sequence[int] = (5, 2, 2, 2, 2, 2, 2)
    conv_bias: bool = False
    num_conv_pos_embeddings: int = 128
    num_conv_pos_embedding_groups: int = 16
    vocab_size: int = 32
    pad_token_id: int = 0
    layer_norm_eps: float = 1e-5
    feat_extract_norm: str = "group"
    feat_extract_activation: str = "gelu"
    hidden_act: str = "gelu"
    do_stable_layer_norm: bool = False
    feat_proj_layer_norm: bool = True
    add_adapter: bool = False
    conv_pos_batch_norm: bool = False

    def __post_init__(self):  # a config.json gives lists
        self.conv_dim, self.conv_kernel, self.conv_stride = tuple(self.conv_dim), tuple(self.conv_kernel), tuple(self.conv_stride)

    @classmethod
    def from_any(cls, cfg) -> "RecognizerConfig":
        """A dict (a checkpoint's `config.json`), a path to one, or any object with the attributes."""
        return config_from_any(cls, cfg)


def expected_keys(c: RecognizerConfig) -> Dict[str, tuple]:
    """canonical key -> shape, as vx_asr_create lays them out."""
    keys = w2v_backbone_keys(c, c.feat_extract_norm == "layer")
    keys["lm_head.weight"], keys["lm_head.bias"] = (int(c.vocab_size), int(c.hidden_size)), (int(c.vocab_size),)
    return keys


def canonical_state_dict(sd: dict) -> Dict[str, torch.Tensor]:
    """A `Wav2Vec2ForCTC` / `HubertForCTC` state dict -> {canonical key: fp32 CPU tensor}: the `wav2vec2.` / `hubert.` prefix dropped,
    the positional convolution's weight norm folded, `masked_spec_embed` ignored."""
    return _canonical({re.sub(r"^hubert\.", "wav2vec2.", k): v for k, v in sd.items()})


def synthetic_state_dict(config, seed: int = 0, prefix: str = "wav2vec2.", head_scale: float = 4.0) -> Dict[str, torch.Tensor]:
    """Seeded weights in the `transformers` layout (prefix `wav2vec2.` / `hubert.`, weight norm unfolded) for the tests.  The scales
    keep every stage alive and make every part of the definition matter (norm gains and biases away from 1 and 0, convolution gains
    that put the GELUs in their curved range); `head_scale` spreads the logits so that the argmax of nearly every frame is decided by
    far more than fp32 rounding."""
    c = RecognizerConfig.from_any(config)
    own = {"lm_head.weight": (0.0, head_scale / math.sqrt(int(c.hidden_size)))}
    return w2v_synthetic_state_dict(expected_keys(c), seed, prefix, lambda k: k.startswith("lm_head"), own, int(c.hidden_size))


@dataclasses.dataclass
class Transcript:
    text: str
    tokens: List[int]      # the kept ids, repeats merged and blanks removed
    frames: List[int]      # the encoder frame of every kept id (x 20 ms at the default strides: the character's time)
    logprob: float         # mean over ALL frames of the log-probability of the frame's argmax


def ids_to_text(ids: Sequence[int], id_to_token: Dict[int, str], word_delimiter: str = "|", special=()) -> str:
    """The tokenizer's rule for already collapsed ids: the word delimiter is a space, special tokens are dropped."""
    out = []
    for i in ids:
        tok = id_to_token.get(int(i), "")
        if tok in special:
            continue
        out.append(" " if tok == word_delimiter else tok)
    return " ".join("".join(out).split())


class SpeechRecognizer(W2vHandle):
    """`SpeechRecognizer(config, vocab, max_batch=32, max_seconds=20.0, state_dict=None)`: `config` is a `RecognizerConfig`, a dict or
    path of the checkpoint's `config.json`, or any object with the `Wav2Vec2Config` / `HubertConfig` attributes; `vocab` is the
    checkpoint's `vocab.json` mapping token -> id, with `|` as the word delimiter and `<pad>` as the CTC blank unless `blank` names
    another token.  A call serves up to `max_batch` (<= 64) utterances of up to `max_seconds` at 16 kHz each.  Adapters,
    `conv_pos_batch_norm`, activations other than GELU, head dimensions other than 16 / 32 / 64 and a feature encoder norm that does
    not go with the encoder (`group` with post-norm, `layer` with stable) raise NotImplementedError naming the field.
    `precision="bf16"` runs the encoder layers of the layer / stable flavour at head_dim 64 on the bf16 matrix cores (include/vallex.h:
    the bf16 encoder mode); the other flavour and head dimensions are refused by name.  Any other precision raises ValueError."""
    _PREFIX, _NAME = "vx_asr", "SpeechRecognizer"

    def __init__(self, config, vocab: Dict[str, int], max_batch: int = 32, max_seconds: float = 20.0, state_dict: Optional[dict] = None,
                 keep_taps: bool = False, blank: str = "<pad>", word_delimiter: str = "|", precision: str = "fp32"):
        if precision not in _e.ENC_PRECISIONS:
            raise ValueError(f"precision = {precision!r}: one of {_e.ENC_PRECISIONS}")
        self.precision = precision
        c = self.config = RecognizerConfig.from_any(config)
        if c.add_adapter:
            raise NotImplementedError("add_adapter: adapters are not served")
        if c.conv_pos_batch_norm:
            raise NotImplementedError("conv_pos_batch_norm: the weight-normed positional convolution is served")
        if c.feat_extract_activation != "gelu" or c.hidden_act != "gelu":
            raise NotImplementedError(f"feat_extract_activation / hidden_act = {c.feat_extract_activation!r} / {c.hidden_act!r}: gelu is served")
        if c.feat_extract_norm not in ("group", "layer"):
            raise ValueError(f"feat_extract_norm = {c.feat_extract_norm!r}")
        if (c.feat_extract_norm == "layer") != bool(c.do_stable_layer_norm):
            raise NotImplementedError(f"feat_extract_norm = {c.feat_extract_norm!r} with do_stable_layer_norm = {bool(c.do_stable_layer_norm)}: "
                                      "group / post-norm and layer / stable are served")
        if int(c.hidden_size) % int(c.num_attention_heads) or int(c.hidden_size) // int(c.num_attention_heads) not in HEAD_DIMS:
            raise NotImplementedError(f"head_dim = {c.hidden_size} / {c.num_attention_heads}: {HEAD_DIMS} are served")
        if not (len(c.conv_dim) == len(c.conv_kernel) == len(c.conv_stride)) or not 1 <= len(c.conv_dim) <= 8:
            raise ValueError("conv_dim, conv_kernel and conv_stride have one entry per layer, 1..8 layers")
        self.vocab = {str(k): int(v) for k, v in vocab.items()}
        if blank not in self.vocab:
            raise ValueError(f"vocab has no blank token {blank!r}")
        if max(self.vocab.values()) >= int(c.vocab_size) or min(self.vocab.values()) < 0:
            raise ValueError(f"vocab ids outside [0, vocab_size = {c.vocab_size})")
        self.blank_id, self.word_delimiter = self.vocab[blank], word_delimiter
        self.id_to_token = {v: k for k, v in self.vocab.items()}
        self.special = tuple(t for t in self.vocab if re.fullmatch(r"<.*>", t))
        self.max_batch, self.max_samples = int(max_batch), int(round(float(max_seconds) * SAMPLE_RATE))
        self.keep_taps = bool(keep_taps)
        self._init_handle()
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # ---- handle -------------------------------------------------------------------------------------
    def _config_struct(self) -> "_e.VxAsrConfig":
        s, c = _e.VxAsrConfig(), self.config
        s.struct_size = C.sizeof(_e.VxAsrConfig)
        self._fill_backbone(s)
        s.vocab, s.blank = int(c.vocab_size), self.blank_id
        s.feat_extract_norm = int(c.feat_extract_norm == "layer")
        s.do_stable_layer_norm = int(bool(c.do_stable_layer_norm))
        s.feat_proj_layer_norm = int(bool(c.feat_proj_layer_norm))
        s.add_adapter, s.conv_pos_batch_norm = int(bool(c.add_adapter)), int(bool(c.conv_pos_batch_norm))
        s.activation = 0
        s.flags = (_e.VX_ASR_KEEP_TAPS if self.keep_taps else 0) | (_e.VX_ASR_ENC_BF16 if self.precision == "bf16" else 0)
        return s

    @property
    def min_samples(self) -> int:
        """The shortest utterance served (one encoder frame): 400 samples at the default kernels and strides."""
        return super().min_samples

    def load_state_dict(self, sd: dict):
        """Takes the `transformers` key layout (see `canonical_state_dict`); missing and unexpected keys and wrong shapes raise by
        name.  Returns self."""
        return self._check_state_dict(expected_keys(self.config), canonical_state_dict(sd))

    # ---- recognition --------------------------------------------------------------------------------
    def _recognize_raw(self, wav_ptrs, lengths, normalize, tokens_ptr, frames_ptr, counts_ptr, logprob_ptr, logits_ptr):
        """vx_asr_recognize on raw pointers (the argument checks run before any device work)."""
        self._call("recognize", wav_ptrs, lengths, _e.VX_ASR_NORMALIZE if normalize else 0, tokens_ptr, frames_ptr, counts_ptr, logprob_ptr,
                   logits_ptr)

    @torch.no_grad()
    def _run(self, wavs, sr, normalize, want_logits, after_chunk=None):
        ws = self._prepare(wavs, sr)
        results, logits = [], []
        V = int(self.config.vocab_size)
        for i in range(0, len(ws), self.max_batch):
            chunk = ws[i:i + self.max_batch]
            T = [self.num_frames(w.numel()) for w in chunk]
            total = max(sum(T), 1)
            tok = torch.full((total,), -1, dtype=torch.int32, device=self.device)
            frm = torch.full((total,), -1, dtype=torch.int32, device=self.device)
            cnt = torch.zeros(len(chunk), dtype=torch.int32, device=self.device)
            lp = torch.zeros(len(chunk), dtype=torch.float32, device=self.device)
            lg = torch.empty((total, V), dtype=torch.float32, device=self.device) if want_logits else None
            with torch.cuda.device(self.device):
                self._recognize_raw([w.data_ptr() for w in chunk], [w.numel() for w in chunk], normalize, tok.data_ptr(), frm.data_ptr(),
                                    cnt.data_ptr(), lp.data_ptr(), None if lg is None else lg.data_ptr())
                if after_chunk is not None:  # the call's logits are still the handle's
                    after_chunk(i, T)
            tok, frm, cnt, lp = tok.cpu(), frm.cpu(), cnt.cpu().tolist(), lp.cpu().tolist()
            o = 0
            for u, t in enumerate(T):
                ids = tok[o:o + cnt[u]].tolist()
                results.append(Transcript(ids_to_text(ids, self.id_to_token, self.word_delimiter, self.special), ids,
                                          frm[o:o + cnt[u]].tolist(), float(lp[u])))
                if want_logits:
                    logits.append(lg[o:o + t])
                o += t
        return results, logits

    def recognize(self, wavs: Union[torch.Tensor, Sequence[torch.Tensor]], sr: int = 24000, normalize: bool = False) -> List[Transcript]:
        """One waveform or a list of ragged ones, float32 (L,), (1, L) or (1, 1, L) at `sr` -> one `Transcript` per utterance.  Audio
        at another rate than 16 kHz goes through the GPU `Resampler` first.  `normalize=True` applies the feature extractor's
        zero-mean unit-variance rule per utterance: the checkpoint's `preprocessor_config.json` (`do_normalize`) says which it
        wants.  More than `max_batch` utterances are served in several calls; every utterance is bitwise what it is alone.  The ids
        become text on the host: `|` is a space, `<...>` tokens are dropped."""
        return self._run(wavs, sr, normalize, False)[0]

    def logits(self, wavs, sr: int = 24000, normalize: bool = False) -> List[torch.Tensor]:
        """Per utterance the (frames, vocab) float32 logits on the device."""
        return self._run(wavs, sr, normalize, True)[1]

    # ---- a known text against the audio -------------------------------------------------------------
    @property
    def seconds_per_frame(self) -> float:
        """The hop of the encoder's frames: the product of the convolution strides over 16 kHz (20 ms at the default strides)."""
        return math.prod(int(s) for s in self.config.conv_stride) / SAMPLE_RATE

    def text_to_ids(self, text: str) -> List[int]:
        """`normalize_text`, then one id per character, a space becoming the word delimiter.  A character the vocabulary lacks
        raises ValueError naming it: nothing is dropped silently."""
        ids = []
        for pos, ch in enumerate(normalize_text(text)):
            tok = self.word_delimiter if ch == " " else ch
            if tok not in self.vocab or self.vocab[tok] == self.blank_id:
                raise ValueError(f"character {ch!r} (position {pos} of {normalize_text(text)!r}) is not in the recogniser's vocabulary")
            ids.append(self.vocab[tok])
        return ids

    def _falign_raw(self, targets: Sequence[Sequence[int]], nll_ptr, plp_ptr, ftok_ptr, start_ptr, end_ptr, score_ptr, feas_ptr):
        """vx_falign_asr on raw pointers: the logits are those of the last `recognize` (the argument checks run before any device
        work)."""
        n = len(targets)
        flat = [int(t) for y in targets for t in y]
        self._invoke(_e.load_library().vx_falign_asr, n, (C.c_int32 * max(len(flat), 1))(*flat),
                     (C.c_int32 * max(n, 1))(*[len(y) for y in targets]), nll_ptr, plp_ptr, ftok_ptr, start_ptr, end_ptr, score_ptr, feas_ptr)

    @torch.no_grad()
    def _align_ids(self, wavs, targets: Sequence[Sequence[int]], sr, normalize, path: bool):
        """Recognises, then aligns every chunk on the logits the call left on the device -> (transcripts, raw alignments)."""
        raws: List[CTCAlignment] = []

        def after_chunk(first, T):
            ys = targets[first:first + len(T)]
            out = _FalignOut(len(T), sum(T), sum(len(y) for y in ys), self.device, path)
            self._falign_raw(ys, *out.pointers())
            raws.extend(out.split(T, [len(y) for y in ys]))

        ws = [wavs] if isinstance(wavs, torch.Tensor) else list(wavs)
        assert len(ws) == len(targets), "one text per waveform"
        return self._run(ws, sr, normalize, False, after_chunk)[0], raws

    def align(self, wavs, texts: Union[str, Sequence[str]], sr: int = 24000, normalize: bool = False) -> List["TextAlignment"]:
        """Where in each waveform the characters and words of its known text are, and how likely the text is: one `TextAlignment`
        per utterance.  One pass of the network serves the transcript and the alignment; the logits never leave the device.  The
        times are frames x `seconds_per_frame`; an infeasible pair (more characters than frames) has `feasible = False`,
        `nll = inf` and no spans.  Nothing is validated on trained weights."""
        texts = [texts] if isinstance(texts, str) else list(texts)
        ids = [self.text_to_ids(t) for t in texts]
        hyps, raws = self._align_ids(wavs, ids, sr, normalize, True)
        inv, spf = self.id_to_token, self.seconds_per_frame
        out = []
        for text, y, hyp, r in zip(texts, ids, hyps, raws):
            chars = []
            if r.feasible:
                for k, t in enumerate(y):
                    tok = inv[t]
                    chars.append(CharSpan(" " if tok == self.word_delimiter else tok, r.starts[k] * spf, r.ends[k] * spf, r.scores[k]))
            out.append(TextAlignment(normalize_text(text), hyp, chars, group_words(chars), r.nll, r.nll / max(len(y), 1), r.path_logprob,
                                     r.feasible, r.frame_tokens))
        return out

    def score_text(self, wavs, texts: Union[str, Sequence[str]], sr: int = 24000, normalize: bool = False) -> List["TextScore"]:
        """The likelihoods only: per utterance `-log p(text | audio)` under CTC, its mean per character and whether the pair is
        feasible (the best path is not computed)."""
        texts = [texts] if isinstance(texts, str) else list(texts)
        ids = [self.text_to_ids(t) for t in texts]
        _, raws = self._align_ids(wavs, ids, sr, normalize, False)
        return [TextScore(r.nll, r.nll / max(len(y), 1), r.feasible, len(y)) for y, r in zip(ids, raws)]


# ---- greedy CTC on given logits -----------------------------------------------------------------------
@torch.no_grad()
def ctc_greedy(logits: torch.Tensor, frames: Sequence[int], blank: int = 0):
    """`vx_ctc_greedy`: logits (sum frames, vocab) float32 on the device, the utterances' rows concatenated -> (tokens, token_frames)
    as lists of int lists, mean log-probabilities (n,) and per-frame log-probabilities (sum frames,) on the host."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
    n, total = len(frames), int(sum(frames))
    assert logits.shape[0] == total
    dev = logits.device
    tok = torch.full((total + 1,), -1, dtype=torch.int32, device=dev)
    frm = torch.full((total + 1,), -1, dtype=torch.int32, device=dev)
    cnt = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    mean = torch.full((n + 1,), float("nan"), dtype=torch.float32, device=dev)
    flp = torch.full((total + 1,), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _e._check(_e.load_library().vx_ctc_greedy(logits.data_ptr(), logits.shape[1], int(blank), n, (C.c_int32 * n)(*[int(f) for f in frames]),
                                                  tok.data_ptr(), frm.data_ptr(), cnt.data_ptr(), mean.data_ptr(), flp.data_ptr(),
                                                  _e.current_stream_ptr(dev)))
    assert int(tok[-1]) == -1 and int(frm[-1]) == -1 and int(cnt[-1]) == -1 and bool(torch.isnan(mean[-1])) and bool(torch.isnan(flp[-1])), \
        "a write outside an output"
    tok, frm, cnt = tok.cpu(), frm.cpu(), cnt[:-1].cpu().tolist()
    ids, at, o = [], [], 0
    for u, t in enumerate(frames):
        ids.append(tok[o:o + cnt[u]].tolist())
        at.append(frm[o:o + cnt[u]].tolist())
        o += int(t)
    return ids, at, mean[:-1].cpu(), flp[:-1].cpu()


# ---- forced alignment and likelihood on given logits -------------------------------------------------------
@dataclasses.dataclass
class CTCAlignment:
    """One utterance of `ctc_forced_align`, in frames and target positions."""
    nll: float                 # -log p(targets | logits); inf when infeasible
    path_logprob: Optional[float]  # the log-probability of the best path; -inf when infeasible
    feasible: bool
    frame_tokens: List[int]    # per frame the index of the target it emits, -1 for blank
    starts: List[int]          # per target its frames [start, end)
    ends: List[int]
    scores: List[float]        # per target the mean log-probability over its frames


class CharSpan(NamedTuple):
    char: str
    start_s: float
    end_s: float
    score: float


class WordSpan(NamedTuple):
    word: str
    start_s: float
    end_s: float
    score: float               # the mean of its characters' scores


@dataclasses.dataclass
class TextAlignment:
    text: str                  # the normalised text that was aligned
    transcript: Transcript     # what the recogniser heard in the same pass
    chars: List[CharSpan]      # one per character of `text`, a space for the word delimiter
    words: List[WordSpan]
    nll: float
    nll_per_char: float        # nll / max(L, 1)
    path_logprob: float
    feasible: bool
    frame_tokens: List[int]


@dataclasses.dataclass
class TextScore:
    nll: float
    nll_per_char: float
    feasible: bool
    n_chars: int


def group_words(chars: Sequence[CharSpan]) -> List[WordSpan]:
    """The characters between word delimiters (spaces): a word runs from its first character's start to its last one's end, and
    its score is the mean of its characters' scores."""
    words, cur = [], []
    for c in list(chars) + [CharSpan(" ", 0.0, 0.0, 0.0)]:
        if c.char != " ":
            cur.append(c)
        elif cur:
            words.append(WordSpan("".join(x.char for x in cur), cur[0].start_s, cur[-1].end_s, sum(x.score for x in cur) / len(cur)))
            cur = []
    return words


class _FalignOut:
    """The device outputs of one vx_falign / vx_falign_asr call, each with a guard entry behind it."""

    def __init__(self, n: int, frames: int, toks: int, dev, path: bool):
        mk = lambda m, dt, fill: torch.full((m + 1,), fill, dtype=dt, device=dev)  # noqa: E731
        self.n, self.path = n, path
        self.nll = mk(n, torch.float64, float("nan"))
        self.feas = mk(n, torch.int32, -7)
        self.plp = mk(n, torch.float64, float("nan")) if path else None
        self.ftok = mk(frames, torch.int32, -7) if path else None
        self.start = mk(toks, torch.int32, -7) if path else None
        self.end = mk(toks, torch.int32, -7) if path else None
        self.score = mk(toks, torch.float32, float("nan")) if path else None

    def pointers(self):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return p(self.nll), p(self.plp), p(self.ftok), p(self.start), p(self.end), p(self.score), p(self.feas)

    def split(self, frames: Sequence[int], lens: Sequence[int]) -> List[CTCAlignment]:
        for t in (self.nll, self.plp, self.score):
            assert t is None or bool(torch.isnan(t[-1])), "a write outside an output"
        for t in (self.feas, self.ftok, self.start, self.end):
            assert t is None or int(t[-1]) == -7, "a write outside an output"
        host = lambda t: None if t is None else t[:-1].cpu().tolist()  # noqa: E731
        nll, feas, plp, ftok, start, end, score = (host(t) for t in (self.nll, self.feas, self.plp, self.ftok, self.start, self.end, self.score))
        out, fo, to = [], 0, 0
        for u, (T, L) in enumerate(zip(frames, lens)):
            T, L = int(T), int(L)
            if self.path:
                out.append(CTCAlignment(nll[u], plp[u], bool(feas[u]), ftok[fo:fo + T], start[to:to + L], end[to:to + L], score[to:to + L]))
            else:
                out.append(CTCAlignment(nll[u], None, bool(feas[u]), [], [], [], []))
            fo, to = fo + T, to + L
        return out


@torch.no_grad()
def _falign(logits: torch.Tensor, frames: Sequence[int], targets: Sequence[Sequence[int]], blank: int, path: bool) -> List[CTCAlignment]:
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
    n, total = len(frames), int(sum(frames))
    assert logits.shape[0] == total and len(targets) == n, "one row per frame and one target list per utterance"
    flat = [int(t) for y in targets for t in y]
    lens = [len(y) for y in targets]
    out = _FalignOut(n, total, len(flat), logits.device, path)
    if total == 0:  # no frame at all: a pointer that is not null, never read
        logits = logits.new_zeros((1, logits.shape[1]))
    with torch.cuda.device(logits.device):
        _e._check(_e.load_library().vx_falign(logits.data_ptr(), logits.shape[1], int(blank), n, (C.c_int32 * n)(*[int(f) for f in frames]),
                                              (C.c_int32 * max(len(flat), 1))(*flat), (C.c_int32 * n)(*lens), *out.pointers(),
                                              _e.current_stream_ptr(logits.device)))
    return out.split(frames, lens)


def ctc_forced_align(logits: torch.Tensor, frames: Sequence[int], targets: Sequence[Sequence[int]], blank: int = 0) -> List[CTCAlignment]:
    """`vx_falign`: logits (sum frames, vocab) float32 on the device, the utterances' rows concatenated, and per utterance the
    target ids (none equal to `blank`) -> one `CTCAlignment` per utterance: the likelihood, the best path's log-probability, per
    frame the target it emits, per target its frames [start, end) and mean log-probability.  Up to 1000 targets an utterance."""
    return _falign(logits, frames, targets, blank, True)


def ctc_nll(logits: torch.Tensor, frames: Sequence[int], targets: Sequence[Sequence[int]], blank: int = 0) -> torch.Tensor:
    """`vx_falign`'s likelihood half alone: `-log p(targets | logits)` per utterance, (n,) float64 on the host, `inf` where the
    targets do not fit the frames.  `F.ctc_loss(reduction="none")` on a ragged batch, in fp64."""
    return torch.tensor([r.nll for r in _falign(logits, frames, targets, blank, False)], dtype=torch.float64)


# ---- edit distance and error rates ------------------------------------------------------------------------
@dataclasses.dataclass
class PairErrors:
    distance: int
    substitutions: int
    deletions: int
    insertions: int
    ref_len: int

    @property
    def rate(self) -> float:
        return self.distance / self.ref_len if self.ref_len else float("nan")


@dataclasses.dataclass
class ErrorRate:
    rate: float               # (sum S + sum D + sum I) / sum N over the corpus; nan when sum N = 0
    pairs: List[PairErrors]


@torch.no_grad()
def edit_distance(refs: Sequence[Sequence[int]], hyps: Sequence[Sequence[int]], device="cuda") -> torch.Tensor:
    """`vx_edit_distance`: per pair (distance, substitutions, deletions, insertions) turning refs[p] into hyps[p], an (n, 4) int32
    tensor on the host.  Unit costs; among equal costs a match or substitution is preferred, then a deletion, then an insertion.
    Up to 2048 tokens a side; a zero-length side is legal."""
    assert len(refs) == len(hyps) and len(refs) >= 1, "one hypothesis per reference"
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("valle_amd.asr.edit_distance runs only on an MI355X (no CPU fallback)")
    n = len(refs)
    rl, hl = [len(r) for r in refs], [len(h) for h in hyps]
    flat_r = torch.tensor([int(t) for r in refs for t in r] or [0], dtype=torch.int32).to(dev)
    flat_h = torch.tensor([int(t) for h in hyps for t in h] or [0], dtype=torch.int32).to(dev)
    out = torch.full((n * 4 + 1,), -1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _e._check(_e.load_library().vx_edit_distance(n, flat_r.data_ptr(), (C.c_int32 * n)(*rl), flat_h.data_ptr(), (C.c_int32 * n)(*hl),
                                                     out.data_ptr(), _e.current_stream_ptr(dev)))
    assert int(out[-1]) == -1, "a write outside the output"
    return out[:-1].reshape(n, 4).cpu()


def normalize_text(text: str) -> str:
    """The rule both sides of an error rate go through: upper-case; letters, digits and apostrophes are kept; everything else
    becomes a space; runs of spaces collapse and the ends are trimmed."""
    return " ".join("".join(ch if (ch.isalnum() or ch == "'") else " " for ch in str(text).upper()).split())


def _error_rate(ref_units: List[list], hyp_units: List[list], device) -> ErrorRate:
    table: Dict[object, int] = {}
    enc = lambda seq: [table.setdefault(u, len(table)) for u in seq]  # noqa: E731  ids over the union of both sides
    refs, hyps = [enc(r) for r in ref_units], [enc(h) for h in hyp_units]
    pairs: List[PairErrors] = []
    for i in range(0, len(refs), 64):
        for (dist, s, d, ins), r in zip(edit_distance(refs[i:i + 64], hyps[i:i + 64], device).tolist(), refs[i:i + 64]):
            pairs.append(PairErrors(dist, s, d, ins, len(r)))
    total = sum(p.ref_len for p in pairs)
    return ErrorRate(sum(p.distance for p in pairs) / total if total else float("nan"), pairs)


def word_error_rate(ref_texts: Sequence[str], hyp_texts: Sequence[str], device="cuda") -> ErrorRate:
    """WER of hypotheses against references (a string each, or equally long lists): both sides through `normalize_text`, split at
    spaces, words mapped to ids over the union of both sides, the distance on the device.  Per pair S / D / I / N and the rate
    (S + D + I) / N (`nan` when N = 0); the corpus rate is (sum S + sum D + sum I) / sum N, a pair with N = 0 counted in the sums."""
    ref_texts = [ref_texts] if isinstance(ref_texts, str) else list(ref_texts)
    hyp_texts = [hyp_texts] if isinstance(hyp_texts, str) else list(hyp_texts)
    return _error_rate([normalize_text(t).split() for t in ref_texts], [normalize_text(t).split() for t in hyp_texts], device)


def char_error_rate(ref_texts: Sequence[str], hyp_texts: Sequence[str], device="cuda") -> ErrorRate:
    """CER: as `word_error_rate` over the characters of the normalised texts, the single spaces between words included."""
    ref_texts = [ref_texts] if isinstance(ref_texts, str) else list(ref_texts)
    hyp_texts = [hyp_texts] if isinstance(hyp_texts, str) else list(hyp_texts)
    return _error_rate([list(normalize_text(t)) for t in ref_texts], [list(normalize_text(t)) for t in hyp_texts], device)


def recognition_error(text, wav, recognizer: SpeechRecognizer, sr: int = 24000, normalize: bool = False, unit: str = "word") -> ErrorRate:
    """The WER (`unit="word"`) or CER (`unit="char"`) of synthesised utterance(s) against the text they were given: `wav` goes
    through `recognizer.recognize`, the transcript and `text` through the error rate.  On synthetic weights the number means
    nothing."""
    texts = [text] if isinstance(text, str) else list(text)
    hyps = [t.text for t in recognizer.recognize(wav, sr=sr, normalize=normalize)]
    assert len(hyps) == len(texts), "one text per waveform"
    fn = {"word": word_error_rate, "char": char_error_rate}[unit]
    return fn(texts, hyps, recognizer.device)


def text_likelihood(text, wav, recognizer: SpeechRecognizer, sr: int = 24000, normalize: bool = False) -> List[TextScore]:
    """How likely the text(s) an utterance was given are under its audio: per utterance a `TextScore` with the CTC likelihood
    `-log p(text | audio)` and its mean per character.  A continuous companion of `recognition_error`: it still separates two
    candidates with the same error rate, and needs no decoding decision.  On synthetic weights the number means nothing."""
    return recognizer.score_text(wav, [text] if isinstance(text, str) else list(text), sr=sr, normalize=normalize)
