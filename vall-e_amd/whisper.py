"""Whisper recogniser on the GPU: `transformers`' `WhisperForConditionalGeneration` with greedy decoding behind `vx_wsp_*`
(include/vallex.h, csrc/whisper_kernels.hpp on top of the speaker encoder's kernels); there is no CPU fallback and `transformers` is
not needed at run time.

    from valle_amd import WhisperRecognizer, recognition_error
    rec = WhisperRecognizer("ckpt/config.json", json.load(open("ckpt/vocab.json")), "ckpt/generation_config.json",
                            state_dict=torch.load("ckpt/pytorch_model.bin")).to("cuda")
    hyp = rec.recognize([synth_wav], sr=24000)[0]           # .text, .tokens, .token_logprobs, .logprob, .stop_reason
    wer = recognition_error(text, synth_wav, rec, sr=24000)   # the CTC recogniser's function, unchanged
    nll = rec.score_tokens([synth_wav], [token_ids]).nll      # teacher forcing

The definition is stated in include/vallex.h and restated in fp64 in tests/whisper_ref.py, which tests/test_whisper_cpu.py pins
against `transformers`.  One chunk (30 s at the released shapes) per utterance; beam search, temperature fallback, timestamps,
language detection, long-form transcription and a bf16 token loop are not built (`precision="bf16"` is the encoder's).  Nothing has been recognised on trained weights: no checkpoint
is available where this is built, and on synthetic weights the transcript means nothing.  Parity with `openai-whisper` and with the
tokenizer's encode direction is not pinned: text comes from `vocab.json` by the byte-level decode rule only."""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Union

import torch

from . import engine as _e
from ._speech_handle import SAMPLE_RATE, SpeechHandle, config_from_any

N_FFT, HOP, BINS = 400, 160, 201
STOP_REASONS = {0: "none", 1: "eos", 2: "max_new_tokens", 3: "max_target_positions"}


@dataclasses.dataclass
class WhisperConfig:
    """The fields of `transformers.WhisperConfig` the network reads, under their names and with its defaults."""
    vocab_size: int = 51865
    num_mel_bins: int = 80
    encoder_layers: int = 4
    encoder_attention_heads: int = 6
    decoder_layers: int = 4
    decoder_attention_heads: int = 6
    decoder_ffn_dim: int = 1536
    encoder_ffn_dim: int = 1536
    d_model: int = 384
    activation_function: str = "gelu"
    max_source_positions: int = 1500
    max_target_positions: int = 448
    eos_token_id: int = 50256
    decoder_start_token_id: int = 50257
    tie_word_embeddings: bool = True

    @classmethod
    def from_any(cls, cfg) -> "WhisperConfig":
        """A dict (a checkpoint's `config.json`), a path to one, or any object with the attributes."""
        return config_from_any(cls, cfg)

    @property
    def chunk_samples(self) -> int:
        return 320 * int(self.max_source_positions)


@dataclasses.dataclass
class WhisperGeneration:
    """The fields of the checkpoint's `generation_config.json` greedy decoding reads."""
    decoder_start_token_id: Optional[int] = None
    eos_token_id: Optional[int] = None
    no_timestamps_token_id: Optional[int] = None
    lang_to_id: Optional[Dict[str, int]] = None
    task_to_id: Optional[Dict[str, int]] = None
    suppress_tokens: Sequence[int] = ()
    begin_suppress_tokens: Sequence[int] = ()
    max_length: Optional[int] = None

    @classmethod
    def from_any(cls, cfg) -> "WhisperGeneration":
        if cfg is None:
            return cls()
        if isinstance(cfg, cls):
            return cfg
        out = config_from_any(cls, cfg)
        if isinstance(out.eos_token_id, (list, tuple)):
            out.eos_token_id = int(out.eos_token_id[0])
        return out


def mel_filters(n_mels: int) -> torch.Tensor:
    """(n_mels, 201) float64: Whisper's mel table, Slaney scale and norm over 0 .. 8000 Hz at n_fft 400 / 16 kHz, computed in fp64
    (`transformers.audio_utils.mel_filter_bank(201, n_mels, 0, 8000, 16000, "slaney", "slaney")`, transposed)."""
    from .fbank import slaney_mel_basis_f64

    return torch.from_numpy(slaney_mel_basis_f64(SAMPLE_RATE, N_FFT, int(n_mels), 0.0, 8000.0))


def expected_keys(c: WhisperConfig) -> Dict[str, tuple]:
    """`transformers` key -> shape, as vx_wsp_create lays them out (without `mel_filters`)."""
    d, P, Tt, V = int(c.d_model), int(c.max_source_positions), int(c.max_target_positions), int(c.vocab_size)
    keys: Dict[str, tuple] = {}

    def lin(name, n, k, bias=True):
        keys[name + ".weight"] = (n, k)
        if bias:
            keys[name + ".bias"] = (n,)

    def norm(name):
        keys[name + ".weight"], keys[name + ".bias"] = (d,), (d,)

    def attn(name):
        lin(name + ".q_proj", d, d)
        lin(name + ".k_proj", d, d, bias=False)
        lin(name + ".v_proj", d, d)
        lin(name + ".out_proj", d, d)

    keys["model.encoder.conv1.weight"], keys["model.encoder.conv1.bias"] = (d, int(c.num_mel_bins), 3), (d,)
    keys["model.encoder.conv2.weight"], keys["model.encoder.conv2.bias"] = (d, d, 3), (d,)
    keys["model.encoder.embed_positions.weight"] = (P, d)
    for l in range(int(c.encoder_layers)):
        pre = f"model.encoder.layers.{l}."
        attn(pre + "self_attn")
        norm(pre + "self_attn_layer_norm")
        lin(pre + "fc1", int(c.encoder_ffn_dim), d)
        lin(pre + "fc2", d, int(c.encoder_ffn_dim))
        norm(pre + "final_layer_norm")
    norm("model.encoder.layer_norm")
    keys["model.decoder.embed_tokens.weight"] = (V, d)
    keys["model.decoder.embed_positions.weight"] = (Tt, d)
    for l in range(int(c.decoder_layers)):
        pre = f"model.decoder.layers.{l}."
        attn(pre + "self_attn")
        norm(pre + "self_attn_layer_norm")
        attn(pre + "encoder_attn")
        norm(pre + "encoder_attn_layer_norm")
        lin(pre + "fc1", int(c.decoder_ffn_dim), d)
        lin(pre + "fc2", d, int(c.decoder_ffn_dim))
        norm(pre + "final_layer_norm")
    norm("model.decoder.layer_norm")
    if not c.tie_word_embeddings:
        keys["proj_out.weight"] = (V, d)
    return keys


def synthetic_state_dict(config, seed: int = 0, head_scale: float = 3.0, pos_scale: float = 1.5, eos_boost: float = 1.6) -> Dict[str, torch.Tensor]:
    """Seeded weights in the `transformers` layout for the tests and the benchmark.  The scales keep every stage alive and make every
    part of the definition matter (norm gains and biases away from 1 and 0, positional tables of the activations' size);
    `head_scale` spreads the logits so that nearly every step is decided by far more than fp32 rounding, `pos_scale` keeps a tied
    embedding from repeating its own input for ever, and `eos_boost` lengthens the end-of-text row so that greedy runs end at
    different steps."""
    c = WhisperConfig.from_any(config)
    g = torch.Generator().manual_seed(int(seed))
    sd: Dict[str, torch.Tensor] = {}

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    for k, shape in expected_keys(c).items():
        if k.endswith("layer_norm.weight"):
            sd[k] = 1.0 + rnd(*shape, scale=0.2)
        elif k.endswith("layer_norm.bias"):
            sd[k] = rnd(*shape, scale=0.3)
        elif k.endswith(".bias"):
            sd[k] = rnd(*shape, scale=0.1)
        elif k.endswith("embed_positions.weight"):
            sd[k] = rnd(*shape, scale=pos_scale)
        elif k.endswith("embed_tokens.weight") or k == "proj_out.weight":
            sd[k] = rnd(*shape, scale=head_scale / math.sqrt(shape[1]))
        else:  # Linear and convolution weights: unit gain over the fan-in
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            sd[k] = rnd(*shape, scale=1.5 / math.sqrt(fan_in))
    for k in ("model.decoder.embed_tokens.weight", "proj_out.weight"):
        if k in sd:
            sd[k][int(c.eos_token_id)] *= eos_boost
    if c.tie_word_embeddings:
        sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"]
    return sd


# ---- ids to text ------------------------------------------------------------------------------------------
def bytes_to_unicode() -> Dict[int, str]:
    """GPT-2's table: every byte as a printable character (the printable Latin-1 bytes are themselves, the others are 256 + n in
    the order they are met)."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("\xa1"), ord("\xac") + 1)) + list(range(ord("\xae"), ord("\xff") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


_UNICODE_TO_BYTE = {c: b for b, c in bytes_to_unicode().items()}


def decode_tokens(ids: Sequence[int], id_to_token: Dict[int, str], first_special: int) -> str:
    """The byte-level rule: ids at or above `first_special` are dropped, the token strings are concatenated, GPT-2's table is
    inverted and the bytes are decoded as UTF-8 with errors="replace"."""
    s = "".join(id_to_token.get(int(i), "") for i in ids if int(i) < first_special)
    return bytes(_UNICODE_TO_BYTE[ch] for ch in s if ch in _UNICODE_TO_BYTE).decode("utf-8", errors="replace")


@dataclasses.dataclass
class WhisperTranscript:
    text: str                    # "" without a vocab
    tokens: List[int]            # the generated ids, the stopping one (eos) included
    token_logprobs: List[float]  # per token, over the processed row (suppressed tokens at -inf)
    logprob: float               # their sum
    stop_reason: str             # "eos", "max_new_tokens" or "max_target_positions"


class TokenScores(NamedTuple):
    nll: List[float]                   # per utterance -sum of the log-probabilities of the given tokens
    mean: float                        # sum of nll / number of tokens
    token_logprobs: List[List[float]]


class WhisperRecognizer(SpeechHandle):
    """`WhisperRecognizer(config, vocab=None, generation_config=None, max_batch=8, state_dict=None, keep_taps=False,
    precision="fp32")`: `config` and
    `generation_config` are dicts, paths of the checkpoint's `config.json` / `generation_config.json`, or objects with those
    attributes; `vocab` is the checkpoint's `vocab.json` mapping token -> id (without it `.text` is "").  A call serves up to
    `max_batch` (<= 64) utterances of up to one chunk (320 x max_source_positions samples at 16 kHz) each.  A head dimension other
    than 64 and an activation other than GELU raise NotImplementedError naming the field.  `precision="bf16"` runs the encoder layers
    on the bf16 matrix cores (include/vallex.h: the bf16 encoder mode); the front end, the cross-attention projections and the token
    loop stay fp32.  Any other precision raises ValueError."""
    _PREFIX, _NAME = "vx_wsp", "WhisperRecognizer"

    def __init__(self, config, vocab: Optional[Dict[str, int]] = None, generation_config=None, max_batch: int = 8,
                 state_dict: Optional[dict] = None, keep_taps: bool = False, mel_basis: Optional[torch.Tensor] = None,
                 precision: str = "fp32"):
        if precision not in _e.ENC_PRECISIONS:
            raise ValueError(f"precision = {precision!r}: one of {_e.ENC_PRECISIONS}")
        self.precision = precision
        c = self.config = WhisperConfig.from_any(config)
        gen = self.generation = WhisperGeneration.from_any(generation_config)
        if c.activation_function != "gelu":
            raise NotImplementedError(f"activation_function = {c.activation_function!r}: gelu is served")
        for side, heads in (("encoder", c.encoder_attention_heads), ("decoder", c.decoder_attention_heads)):
            if int(c.d_model) % int(heads) or int(c.d_model) // int(heads) != 64:
                raise NotImplementedError(f"{side} head_dim = d_model / {side}_attention_heads = {c.d_model} / {heads}: 64 is served")
        self.eos_token_id = int(gen.eos_token_id if gen.eos_token_id is not None else c.eos_token_id)
        self.decoder_start_token_id = int(gen.decoder_start_token_id if gen.decoder_start_token_id is not None else c.decoder_start_token_id)
        self.vocab = None if vocab is None else {str(k): int(v) for k, v in vocab.items()}
        self.id_to_token = {} if self.vocab is None else {v: k for k, v in self.vocab.items()}
        # every id from the end-of-text token on is special in the released vocabularies
        self.first_special = min(self.eos_token_id, self.decoder_start_token_id)
        self.max_batch, self.keep_taps = int(max_batch), bool(keep_taps)
        mel = mel_filters(int(c.num_mel_bins)) if mel_basis is None else torch.as_tensor(mel_basis)
        if tuple(mel.shape) != (int(c.num_mel_bins), BINS):
            raise ValueError(f"mel_basis is {tuple(mel.shape)}, expected ({c.num_mel_bins}, {BINS})")
        self.mel_basis = mel.to(torch.float32).contiguous()
        self._init_handle()
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # ---- handle -------------------------------------------------------------------------------------
    def _config_struct(self) -> "_e.VxWspConfig":
        s, c = _e.VxWspConfig(), self.config
        s.struct_size = C.sizeof(_e.VxWspConfig)
        s.n_mels, s.d_model = int(c.num_mel_bins), int(c.d_model)
        s.enc_layers, s.enc_heads, s.enc_ffn = int(c.encoder_layers), int(c.encoder_attention_heads), int(c.encoder_ffn_dim)
        s.dec_layers, s.dec_heads, s.dec_ffn = int(c.decoder_layers), int(c.decoder_attention_heads), int(c.decoder_ffn_dim)
        s.max_source_positions, s.max_target_positions = int(c.max_source_positions), int(c.max_target_positions)
        s.vocab = int(c.vocab_size)
        s.activation = 0 if c.activation_function == "gelu" else 1
        s.tie_proj = int(bool(c.tie_word_embeddings))
        s.eos_token_id = self.eos_token_id
        s.max_batch = self.max_batch
        s.flags = (_e.VX_WSP_KEEP_TAPS if self.keep_taps else 0) | (_e.VX_WSP_ENC_BF16 if self.precision == "bf16" else 0)
        return s

    def _configure(self, lib):
        sup = [int(t) for t in (self.generation.suppress_tokens or ())]
        beg = [int(t) for t in (self.generation.begin_suppress_tokens or ())]
        _e._check(lib.vx_wsp_set_suppress(self._h, (C.c_int32 * max(len(sup), 1))(*sup), len(sup), (C.c_int32 * max(len(beg), 1))(*beg), len(beg)))

    def _tensors(self):
        return list(self._weights.items()) + [("mel_filters", self.mel_basis)]

    def timings(self) -> Dict[str, float]:
        """Of the last call: host ms, workspace and weight bytes, decode steps enqueued, device ms of log-mel / encoder / token loop."""
        out = (C.c_double * 7)()
        _e._check(_e.load_library().vx_wsp_get_timings(self._handle(), out, 7))
        return dict(zip(("host_ms", "workspace_bytes", "weight_bytes", "steps", "logmel_ms", "encoder_ms", "loop_ms"), out))

    def load_state_dict(self, sd: dict):
        """Takes the `transformers` key layout (`model.encoder...`, `model.decoder...`, `proj_out.weight`; a tied checkpoint may
        carry `proj_out.weight` or not); missing and unexpected keys and wrong shapes raise by name.  Returns self."""
        want = expected_keys(self.config)
        w = dict(sd)
        if self.config.tie_word_embeddings:
            w.pop("proj_out.weight", None)
        return self._check_state_dict(want, w)

    # ---- recognition --------------------------------------------------------------------------------
    def prompt_prefix(self, language: Optional[str] = "en", task: Optional[str] = "transcribe") -> List[int]:
        """`[decoder_start, lang_to_id[...], task_to_id[...], no_timestamps]` from the generation config; an English-only checkpoint
        has no language and task ids and gets `[decoder_start, no_timestamps]`."""
        g = self.generation
        ids = [self.decoder_start_token_id]
        if g.lang_to_id and g.task_to_id:
            key = language if language in g.lang_to_id else f"<|{language}|>"
            if key not in g.lang_to_id:
                raise ValueError(f"language = {language!r} is not in the generation config's lang_to_id")
            if task not in g.task_to_id:
                raise ValueError(f"task = {task!r} is not in the generation config's task_to_id")
            ids += [int(g.lang_to_id[key]), int(g.task_to_id[task])]
        if g.no_timestamps_token_id is not None:
            ids.append(int(g.no_timestamps_token_id))
        return ids

    def _recognize_raw(self, wav_ptrs, lengths, prompts: Sequence[Sequence[int]], max_new: Sequence[int], forced, out_stride: int, tokens_ptr,
                       logprobs_ptr, counts_ptr, stops_ptr):
        """vx_wsp_recognize on raw pointers (the argument checks run before any device work)."""
        n = len(wav_ptrs)
        ps = max(max((len(p) for p in prompts), default=1), 1)
        flat = [0] * (n * ps)
        for i, p in enumerate(prompts):
            flat[i * ps:i * ps + len(p)] = [int(t) for t in p]
        fo = None
        if forced is not None:
            ff = [0] * (n * out_stride)
            for i, y in enumerate(forced):
                ff[i * out_stride:i * out_stride + len(y)] = [int(t) for t in y]
            fo = (C.c_int32 * len(ff))(*ff)
        self._call("recognize", wav_ptrs, lengths, (C.c_int32 * len(flat))(*flat), (C.c_int32 * n)(*[len(p) for p in prompts]), ps,
                   (C.c_int32 * n)(*[int(m) for m in max_new]), fo, int(out_stride), tokens_ptr, logprobs_ptr, counts_ptr, stops_ptr)

    def _prompts(self, n, language, task, prompt_ids):
        if prompt_ids is None:
            return [self.prompt_prefix(language, task)] * n
        if len(prompt_ids) == 0:
            raise ValueError("prompt_ids is empty: the decoder input starts with at least decoder_start_token_id")
        if isinstance(prompt_ids[0], int):
            return [list(prompt_ids)] * n
        assert len(prompt_ids) == n, "one prompt per waveform"
        return [list(p) for p in prompt_ids]

    @torch.no_grad()
    def _run(self, ws: List[torch.Tensor], prompts, max_new: List[int], forced):
        Tt = int(self.config.max_target_positions)
        for i, p in enumerate(prompts):
            if len(p) == 0:
                raise ValueError(f"prompt_ids of utterance {i} is empty: the decoder input starts with at least decoder_start_token_id")
            if len(p) >= Tt:
                raise ValueError(f"prompt_ids of utterance {i} has {len(p)} tokens: no room under max_target_positions = {Tt}")
        results = []
        for i in range(0, len(ws), self.max_batch):
            chunk, pr, mn = ws[i:i + self.max_batch], prompts[i:i + self.max_batch], max_new[i:i + self.max_batch]
            fc = None if forced is None else forced[i:i + self.max_batch]
            n, stride = len(chunk), max(min(max(mn), Tt), 1)
            tok = torch.full((n, stride), -1, dtype=torch.int32, device=self.device)
            lp = torch.zeros((n, stride), dtype=torch.float32, device=self.device)
            cnt = torch.zeros(n, dtype=torch.int32, device=self.device)
            stop = torch.zeros(n, dtype=torch.int32, device=self.device)
            with torch.cuda.device(self.device):
                self._recognize_raw([w.data_ptr() for w in chunk], [w.numel() for w in chunk], pr, [min(m, stride) for m in mn], fc, stride,
                                    tok.data_ptr(), lp.data_ptr(), cnt.data_ptr(), stop.data_ptr())
            tok, lp, cnt, stop = tok.cpu(), lp.cpu().double(), cnt.cpu().tolist(), stop.cpu().tolist()
            for u in range(n):
                ids, lps = tok[u, :cnt[u]].tolist(), lp[u, :cnt[u]].tolist()
                text = decode_tokens(ids, self.id_to_token, self.first_special) if self.vocab is not None else ""
                results.append(WhisperTranscript(text, ids, lps, float(sum(lps)), STOP_REASONS[stop[u]]))
        return results

    def recognize(self, wavs: Union[torch.Tensor, Sequence[torch.Tensor]], sr: int = 24000, language: Optional[str] = "en",
                  task: Optional[str] = "transcribe", prompt_ids=None, max_new_tokens: Optional[int] = None,
                  normalize: bool = False) -> List[WhisperTranscript]:
        """One waveform or a list of ragged ones, float32 (L,), (1, L) or (1, 1, L) at `sr` -> one `WhisperTranscript` per utterance by
        greedy decoding.  Audio at another rate than 16 kHz goes through the GPU `Resampler` first; audio longer than a chunk is
        refused (long-form transcription is not built).  `prompt_ids` (one list, or one per utterance) replaces the prefix
        `prompt_prefix(language, task)`.  Without `max_new_tokens` an utterance runs until eos or `max_target_positions`.  More
        than `max_batch` utterances are served in several calls; every utterance is bitwise what it is alone.  `normalize` exists
        for `recognition_error`'s call and must stay False: Whisper's front end has no such option."""
        if normalize:
            raise ValueError("normalize: Whisper's log-mel front end has no input normalisation")
        ws = self._prepare(wavs, sr)
        prompts = self._prompts(len(ws), language, task, prompt_ids)
        Tt = int(self.config.max_target_positions)
        if max_new_tokens is not None and int(max_new_tokens) < 1:
            raise ValueError(f"max_new_tokens = {max_new_tokens}")
        mn = [Tt if max_new_tokens is None else int(max_new_tokens) for p in prompts]
        return self._run(ws, prompts, mn, None)

    def score_tokens(self, wavs, token_ids: Sequence[Sequence[int]], sr: int = 24000, language: Optional[str] = "en",
                     task: Optional[str] = "transcribe", prompt_ids=None) -> TokenScores:
        """Teacher forcing: per utterance the negative log-likelihood of the given tokens after the prompt (each token's
        log-probability is taken over the same processed row greedy decoding reads), the mean per token and the per-token values."""
        ws = self._prepare(wavs, sr)
        if len(token_ids) and isinstance(token_ids[0], int):
            token_ids = [token_ids]
        assert len(token_ids) == len(ws), "one token list per waveform"
        toks = [[int(t) for t in y] for y in token_ids]
        for i, y in enumerate(toks):
            if len(y) == 0:
                raise ValueError(f"token_ids of utterance {i} is empty")
        prompts = self._prompts(len(ws), language, task, prompt_ids)
        res = self._run(ws, prompts, [len(y) for y in toks], toks)
        nll = [-r.logprob for r in res]
        return TokenScores(nll, sum(nll) / sum(len(y) for y in toks), [r.token_logprobs for r in res])


# ---- the token loop's kernels on caller data (tests) -------------------------------------------------------------------------------
def _f32(t, *shape):
    assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and (not shape or tuple(t.shape) == shape), (t.dtype, tuple(t.shape), shape)
    return t.data_ptr()


def _i32(t, *shape):
    assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and (not shape or tuple(t.shape) == shape), (t.dtype, tuple(t.shape), shape)
    return t.data_ptr()


def op_wsp_gemm(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], res: Optional[torch.Tensor], out: torch.Tensor, act: int = 0):
    """wsp_skinny_gemm through the recogniser's launcher (vx_op_wsp_gemm): out (M, N) = act(x (M, K) W (N, K)^T + bias) + res, fp32 on
    the device; `res` may be `out`; act 1 is the exact GELU."""
    (M, K), N = x.shape, W.shape[0]
    _e._check(_e.load_library().vx_op_wsp_gemm(_f32(x), _f32(W, N, K), None if bias is None else _f32(bias, N),
                                               None if res is None else _f32(res, M, N), _f32(out, M, N), M, N, K, int(act),
                                               _e.current_stream_ptr(x.device)))
    return out


def op_wsp_decode_attn(q: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, out: torch.Tensor, ld: int, heads: int, rows_per_utt: int,
                       max_keys: int, knew: Optional[torch.Tensor] = None, vnew: Optional[torch.Tensor] = None,
                       pos: Optional[torch.Tensor] = None, keys: int = 0):
    """wsp_decode_attn through the recogniser's launcher (vx_op_wsp_decode_attn): q (n, ldq) and out (n, 64 heads) fp32 on the device;
    `kcache` and `vcache` are the tensors (views into one buffer are fine) whose data pointers are the key and value bases, row stride
    `ld`.  With knew / vnew (n, ldq) and pos (n) int32 it is the self-attention step, which also appends; without, `keys` cross keys."""
    n, ldq = q.shape
    for t in (kcache, vcache):
        assert t.dtype == torch.float32 and t.is_cuda
    _e._check(_e.load_library().vx_op_wsp_decode_attn(_f32(q), None if knew is None else _f32(knew, n, ldq), None if vnew is None else _f32(vnew, n, ldq),
                                                      kcache.data_ptr(), vcache.data_ptr(), _f32(out, n, 64 * heads), int(ld), ldq, 64 * heads,
                                                      int(heads), n, None if pos is None else _i32(pos, n), int(keys), int(rows_per_utt),
                                                      int(max_keys), _e.current_stream_ptr(q.device)))
    return out


def op_wsp_head(logits: torch.Tensor, suppress: torch.Tensor, prompt: torch.Tensor, n_prompt: torch.Tensor, max_new: torch.Tensor,
                forced: Optional[torch.Tensor], state: Sequence[torch.Tensor], outputs: Sequence[torch.Tensor], eos: int, max_target: int):
    """One wsp_head_reduce step (vx_op_wsp_head) on logits (n, V): `suppress` (V) uint8 (1 suppress_tokens, 2 begin_suppress_tokens),
    `prompt` (n, stride), `state` = (cur, pos, count, finished) and `outputs` = (tokens (n, out_stride) int32, logprobs (n, out_stride)
    float32, counts (n), stops (n)), all int32 on the device and changed in place."""
    n, V = logits.shape
    assert suppress.dtype == torch.uint8 and suppress.is_cuda and suppress.is_contiguous() and suppress.numel() == V
    cur, pos, count, finished = state
    tok, lp, cnt, stop = outputs
    stride = tok.shape[1]
    _e._check(_e.load_library().vx_op_wsp_head(_f32(logits), n, V, suppress.data_ptr(), _i32(prompt), prompt.shape[1], _i32(n_prompt, n),
                                               _i32(max_new, n), None if forced is None else _i32(forced, n, stride), _i32(cur, n), _i32(pos, n),
                                               _i32(count, n), _i32(finished, n), _i32(tok, n, stride), _f32(lp, n, stride), _i32(cnt, n),
                                               _i32(stop, n), stride, int(eos), int(max_target), _e.current_stream_ptr(logits.device)))


def op_wsp_embed(tok_emb: torch.Tensor, pos_emb: torch.Tensor, cur: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """wsp_embed (vx_op_wsp_embed): (n, d) = tok_emb[cur] + pos_emb[pos], fp32 tables and int32 indices on the device."""
    n, d = cur.numel(), tok_emb.shape[1]
    x = torch.empty((n, d), dtype=torch.float32, device=tok_emb.device)
    _e._check(_e.load_library().vx_op_wsp_embed(_f32(tok_emb), _f32(pos_emb, pos_emb.shape[0], d), _i32(cur, n), _i32(pos, n), _f32(x), n, d,
                                                tok_emb.shape[0], pos_emb.shape[0], _e.current_stream_ptr(tok_emb.device)))
    return x


# ---- the bf16 encoder mode's kernels on caller data (tests) ------------------------------------------------------------------------
def _bf16(t, *shape):
    assert t.dtype == torch.bfloat16 and t.is_cuda and t.is_contiguous() and (not shape or tuple(t.shape) == shape), (t.dtype, tuple(t.shape), shape)
    return t.data_ptr()


def op_enc16_gemm(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, epi: int, res: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ebf_gemm through the recognisers' launcher (vx_op_enc16_gemm): A (M, K) and W (N, K) bf16 and bias (N) fp32 on the device.
    epi 0: bf16 (M, N) = A W^T + bias; 1: bf16 = gelu(A W^T + bias); 2: fp32 = (A W^T + bias) + res, res (M, N) fp32 (it may be `out`)."""
    (M, K), N = A.shape, W.shape[0]
    dt = torch.float32 if epi == _e.EBF_EPI_RESID_F32 else torch.bfloat16
    if out is None:
        out = torch.empty((M, N), dtype=dt, device=A.device)
    assert out.dtype == dt and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (M, N)
    _e._check(_e.load_library().vx_op_enc16_gemm(int(epi), _bf16(A), _bf16(W, N, K), _f32(bias, N), None if res is None else _f32(res, M, N),
                                                 out.data_ptr(), M, N, K, _e.current_stream_ptr(A.device)))
    return out


def op_enc16_add_ln(a: torch.Tensor, b: Optional[torch.Tensor], w: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5, bmod: int = 0,
                    want_sum: bool = True):
    """ebf_add_layernorm (vx_op_enc16_add_ln): a (M, d) fp32, b (M, d) or (bmod, d) fp32 or None -> (sum (M, d) fp32 or None, rows (M, d)
    bf16)."""
    M, d = a.shape
    y = torch.empty((M, d), dtype=torch.bfloat16, device=a.device)
    s = torch.empty((M, d), dtype=torch.float32, device=a.device) if want_sum else None
    _e._check(_e.load_library().vx_op_enc16_add_ln(_f32(a), None if b is None else _f32(b, bmod if bmod else M, d), int(bmod), _f32(w, d), _f32(beta, d),
                                                   None if s is None else s.data_ptr(), y.data_ptr(), M, d, float(eps),
                                                   _e.current_stream_ptr(a.device)))
    return s, y


def op_enc16_attn(qkv: torch.Tensor, seg_len: Sequence[int], heads: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ebf_attention (vx_op_enc16_attn): qkv (rows, 3 x 64 heads) bf16 on the device, the segments of `seg_len` rows packed tightly ->
    (rows, 64 heads) bf16."""
    rows, d = qkv.shape[0], 64 * int(heads)
    assert sum(seg_len) == rows
    if out is None:
        out = torch.empty((rows, d), dtype=torch.bfloat16, device=qkv.device)
    _e._check(_e.load_library().vx_op_enc16_attn(_bf16(qkv, rows, 3 * d), _bf16(out, rows, d), len(seg_len), (C.c_int32 * len(seg_len))(*[int(t) for t in seg_len]),
                                                 int(heads), _e.current_stream_ptr(qkv.device)))
    return out
