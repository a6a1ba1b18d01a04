"""Host-side mirror of the reference's model interface for the inference hot path.

``VALLE`` keeps the constructor and the ``inference`` signature of
``valle.models.VALLE`` (/root/reference/valle/models/valle.py:727-760, 961-985) and
``get_model`` / ``add_model_arguments`` those of /root/reference/valle/models/__init__.py, so
that ``valle/bin/infer.py`` only needs its import line changed.  All arithmetic
runs in libvallex.so through the C ABI (engine.py); this file holds only what the reference
does on the host: argument checks, the prefix-mode text trim, RNG bookkeeping, exceptions.
"""
from __future__ import annotations

from collections import OrderedDict, namedtuple
from dataclasses import dataclass
from typing import List, Optional

import torch

from .config import NUM_AUDIO_TOKENS, NUM_TEXT_TOKENS, ModelConfig, add_model_arguments  # noqa: F401
from .meltf import Transformer  # noqa: F401  (the reference's third model, valle/models/transformer.py)
from .weights import expected_keys, synthetic_state_dict, tied_keys

_IncompatibleKeys = namedtuple("IncompatibleKeys", ["missing_keys", "unexpected_keys"])


def _ids_out_of_range(x: torch.Tensor, y: torch.Tensor) -> bool:
    """Text ids outside [0, NUM_TEXT_TOKENS) or codec ids outside [0, NUM_AUDIO_TOKENS): both tests on the device, ONE
    device-to-host read (four `int(t.min())`-style syncs before).  An empty prompt is legal with prepend_bos."""
    tx, ty = x.reshape(-1), y.reshape(-1)
    flags = [((tx < 0) | (tx >= NUM_TEXT_TOKENS)).any()]
    if ty.numel():
        flags.append(((ty < 0) | (ty >= NUM_AUDIO_TOKENS)).any())
    return bool(torch.stack(flags).any())


# d_model of batched decode (max_batch >= 2): the step's GEMM kernel runs K = ns x kgroups x 128 with ns in {1, 2, 4, 8} and
# kgroups in {1, 4}, which K = d and K = 4 d fit at these widths only (vx_create refuses the others)
BATCH_WIDTHS = (128, 256, 512, 1024)


def _check_top_p(top_p) -> float:
    """The nucleus filter's ``top_p`` (top_k_top_p_filtering, valle.py:1262-1282): a number in (0, 1]; 1.0 is off."""
    try:
        v = float(top_p)
    except (TypeError, ValueError):
        raise ValueError(f"top_p must be a number in (0, 1], got {top_p!r}") from None
    if not 0.0 < v <= 1.0:  # NaN fails too
        raise ValueError(f"top_p must be in (0, 1], got {top_p!r}")
    return v


@dataclass
class ScoreResult:
    """What ``VALLE.score`` returns: the per-row terms of the reference's validation numbers (VALLE.forward, valle.py:827-881 for
    the AR decoder, 886-950 for a NAR stage) and their aggregates.  T scored frames, Q codebooks.
      ar_nll (T+1,) fp32 / ar_rank (T+1,) int32   rows predicting codes[P:, 0] and the closing EOS
      nar_nll (Q-1, T) / nar_rank (Q-1, T)        stage i's rows against codes[P:, i+1]; None for Q = 1
      ar_loss, nar_loss[i]                        sums of the nll (F.cross_entropy(reduction="sum"))
      ar_topk_acc, nar_topk_acc[i]                mean(rank < top_k) over the rows whose target is not EOS (1024), the
                                                  reference's MulticlassAccuracy(top_k, ignore_index=1024)"""
    ar_nll: Optional[torch.Tensor]
    ar_rank: Optional[torch.Tensor]
    nar_nll: Optional[torch.Tensor]
    nar_rank: Optional[torch.Tensor]
    ar_loss: Optional[float]
    nar_loss: Optional[List[float]]
    ar_topk_acc: Optional[float]
    nar_topk_acc: Optional[List[float]]
    top_k: int = 10


def aggregate_score(ar_nll, ar_rank, ar_targets, nar_nll, nar_rank, nar_targets, top_k: int = 10) -> ScoreResult:
    """Per-row scores -> ScoreResult.  ``ar_targets`` (T+1,) / ``nar_targets`` (Q-1, T): the ids the rows were scored against;
    rows whose target is NUM_AUDIO_TOKENS (EOS) count in the losses and not in the accuracies, as in the reference, where the
    loss has no ignore_index and the metric has ignore_index=1024 (valle.py:873-881)."""
    def acc(rank, tgt):
        keep = tgt.to(rank.device) != NUM_AUDIO_TOKENS
        return float((rank[keep] < top_k).float().mean()) if bool(keep.any()) else float("nan")

    ar_loss = ar_acc = nar_loss = nar_acc = None
    if ar_nll is not None:
        ar_loss, ar_acc = float(ar_nll.double().sum()), acc(ar_rank, ar_targets)
    if nar_nll is not None:
        nar_loss = [float(r.double().sum()) for r in nar_nll]
        nar_acc = [acc(r, t) for r, t in zip(nar_rank, nar_targets)]
    return ScoreResult(ar_nll, ar_rank, nar_nll, nar_rank, ar_loss, nar_loss, ar_acc, nar_acc, int(top_k))


EOS_STOPS = (1, 2)  # VX_STOP_EOS_ARGMAX, VX_STOP_EOS_SAMPLE: the pass that stopped the decode is scored at EOS


@dataclass
class GenLogProbs:
    """What generation reports next to the codes on a model built with ``logprobs=True`` (VX_FLAG_LOGPROBS): the model's
    log-probability of every token it emitted, on the raw logits (before temperature, top-k and top-p).
      ar (n_pass,) fp32     pass i: log p(t_i), t_i the appended token (the forced one under teacher forcing), EOS for the pass
                            that ended the decode on EOS, else the sampled token.  ar[:n_tokens] lines up with codebook 0 of the
                            codes; after an EOS stop ar[n_tokens] is the EOS term and the sum is -ScoreResult.ar_loss of the codes
      nar (Q-1, T) fp32     stage i, frame t: log p of the code the stage picked (its argmax); None when Q == 1 or T == 0
      n_tokens, stop_reason of the AR decode (engine.STOP_REASONS)"""
    ar: torch.Tensor
    nar: Optional[torch.Tensor]
    n_tokens: int
    stop_reason: int

    @property
    def ar_mean(self) -> float:
        """Mean log-probability per emitted AR token, the closing EOS included when the decode stopped on it (NaN when nothing
        was emitted): the length-normalised score best-of-N ranks by."""
        n = self.n_tokens + (1 if self.stop_reason in EOS_STOPS else 0)
        return float(self.ar[:n].double().mean()) if n > 0 else float("nan")


@dataclass
class BestOf:
    """What ``inference_best_of`` reports next to the winner's codes: the winner's ``index`` among the n candidates, their
    ``seeds``, ``ar_mean`` (n floats, GenLogProbs.ar_mean) and ``tokens`` (the n codebook-0 sequences), and the winner's
    ``logprobs``.  ``rank_key``: the n values the candidates were ranked by (``ar_mean`` itself under ``rank_by="logprob"``);
    ``alignments``: the n candidates' ``Alignment`` (None for a candidate that emitted nothing) when the ranking asked for them,
    else None."""
    index: int
    seeds: List[int]
    ar_mean: List[float]
    tokens: List[torch.Tensor]
    logprobs: Optional[GenLogProbs] = None
    alignments: Optional[list] = None
    rank_key: Optional[List[float]] = None


def best_of_index(ar_mean) -> int:
    """Best-of-N's choice: the highest mean log-probability, ties to the lower index; a candidate that emitted nothing (NaN)
    ranks last."""
    vals = [float("-inf") if v != v else float(v) for v in ar_mean]
    if not vals:
        raise ValueError("no candidates")
    return max(range(len(vals)), key=lambda i: (vals[i], -i))


def alignment_rank_key(alignment, genlogprobs=None) -> float:
    """Best-of-N's key under ``rank_by="alignment"``: the score of the best monotonic path per scored frame, path_score / T; -inf
    for a candidate without a path (T < Sw) or without output (``alignment`` None)."""
    if alignment is None or alignment.path is None:
        return float("-inf")
    T = int(alignment.attn.shape[0])
    return float(alignment.path_score) / T if T > 0 else float("-inf")


def best_of_rank(keys, ar_mean) -> int:
    """Best-of-N's choice by a key other than the log-probability: the highest key; a key of -inf or NaN ranks last; ties go to
    the higher ``ar_mean``, then to the lower index.  When no candidate has a finite-or-+inf key the order is ``best_of_index``'s."""
    ks = [float("-inf") if k != k else float(k) for k in keys]
    if len(ks) != len(ar_mean):
        raise ValueError(f"{len(ks)} keys for {len(ar_mean)} candidates")
    if all(k == float("-inf") for k in ks):
        return best_of_index(ar_mean)
    ms = [float("-inf") if v != v else float(v) for v in ar_mean]
    return max(range(len(ks)), key=lambda i: (ks[i], ms[i], -i))


FRAME_RATE = 75.0  # codec frames per second (EnCodec at 24 kHz, hop 320)


@dataclass
class Alignment:
    """What ``VALLE.align`` returns: the attention the AR decoder pays to the text while it predicts each of the T scored frames,
    over the Sw text tokens of the window, and the timestamps that follow from it.
      attn (T, Sw) fp32        head-weighted softmax probability of frame t on text token j (VALL-E: the text columns of the
                               self-attention; VALL-F: the cross-attention over the text memory)
      text_mass (T,) fp32      weighted share of frame t's attention that goes to the text at all (1 for VALL-F)
      path (T,) int32 / None   the best monotonic path (token 0 at frame 0, token Sw-1 at frame T-1, steps of 0 or 1); None when
                               T < Sw, i.e. the audio is too short to speak every token
      path_score float         sum_t log attn[t, path[t]] (-inf without a path)
      spans (Sw, 2) int32      [start, end) frame of each text token on the path; None without a path
      seconds (Sw, 2) fp32     spans / 75.0
      token_mass (Sw,) fp32    attn.sum(0): how much attention each token received in all (near 0: a skipped token)
      per_head (L, H, T, Sw)   every head's own map, when asked for"""
    attn: torch.Tensor
    text_mass: torch.Tensor
    path: Optional[torch.Tensor]
    path_score: float
    spans: Optional[torch.Tensor]
    seconds: Optional[torch.Tensor]
    token_mass: torch.Tensor
    per_head: Optional[torch.Tensor] = None


def path_spans(path: torch.Tensor, Sw: int) -> torch.Tensor:
    """(Sw, 2) int32 [start, end) frame of each token of a monotonic path (T,) that visits every column 0 .. Sw-1 in order."""
    p = path.to(torch.int64)
    counts = torch.bincount(p, minlength=Sw)
    end = torch.cumsum(counts, 0)
    return torch.stack([end - counts, end], 1).to(torch.int32)


def make_alignment(attn, text_mass, path, path_score, per_head=None) -> Alignment:
    """Engine outputs -> Alignment (spans, seconds and token_mass computed here with torch)."""
    score = float(path_score) if path_score is not None else float("-inf")
    if path is None or (path.numel() and int(path[0]) < 0):
        path = spans = seconds = None
    else:
        spans = path_spans(path, attn.shape[1])
        seconds = spans.to(torch.float32) / FRAME_RATE
    return Alignment(attn, text_mass, path, score, spans, seconds, attn.sum(0), per_head)


def head_weights(heads, L: int, H: int) -> Optional[torch.Tensor]:
    """``align``'s ``heads`` -> None (all heads, uniform) or an (L, H) fp32 tensor that sums to 1: a list of (layer, head) pairs
    (uniform over them) or an (L, H) tensor of non-negative weights (normalised)."""
    if heads is None:
        return None
    if isinstance(heads, torch.Tensor):
        w = heads.detach().to("cpu", torch.float64)
        if tuple(w.shape) != (L, H):
            raise ValueError(f"heads tensor must be ({L}, {H}), got {tuple(w.shape)}")
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()) or float(w.sum()) <= 0:
            raise ValueError("heads weights must be finite, >= 0 and not all zero")
        return (w / w.sum()).to(torch.float32)
    pairs = list(heads)
    if not pairs:
        raise ValueError("heads is empty: no head to align by")
    w = torch.zeros((L, H), dtype=torch.float64)
    for pr in pairs:
        try:
            l, h = (int(v) for v in pr)
        except (TypeError, ValueError):
            raise ValueError(f"heads must be (layer, head) pairs, got {pr!r}") from None
        if not (0 <= l < L and 0 <= h < H):
            raise ValueError(f"head {(l, h)} outside ({L}, {H})")
        if w[l, h] != 0:
            raise ValueError(f"head {(l, h)} listed twice")
        w[l, h] = 1.0
    return (w / w.sum()).to(torch.float32)


class VALLE:
    """Decoder-only VALL-E (inference only).  Engine-specific keyword arguments (not in the
    reference): ``precision`` ("bf16" | "fp32" | "fp8nar"), ``max_text``, ``max_audio`` (capacities), ``max_batch`` (slots of
    ``inference_batch`` / ``inference_stream``; >= 2 needs head_dim 64 and d_model in BATCH_WIDTHS), ``kv_cache`` ("bf16" |
    "fp8": storage of those slots' KV caches; "fp8" needs max_batch >= 2, a bf16 / fp8nar precision, head_dim 64 and a pre-norm
    VALL-E without prenets),
    ``sampling`` ("device": on-GPU counter RNG seeded from torch's global generator;
    "torch_cpu": reproduce the exact Exp(1) stream torch.multinomial would consume on CPU).  ``inference``,
    ``inference_batch`` and ``inference_stream`` take a ``top_p`` keyword (default 1.0, off): the reference's nucleus filter
    (top_k_top_p_filtering, valle.py:1262-1282) after temperature and top-k, which its VALLE.inference does not expose.
    ``logprobs=True`` (VX_FLAG_LOGPROBS, any configuration): generation also records the model's log-probability of every token it
    emits; ``inference`` / ``inference_batch`` / ``inference_stream`` then accept ``return_logprobs=True`` and return
    ``(codes, GenLogProbs)`` per utterance, and ``inference_best_of`` (max_batch >= 2) samples n candidates of one utterance and
    keeps the most likely.  Without it nothing changes.
    ``align`` (vx_align, any configuration) returns the attention of the AR decoder over the text for given codes and the
    per-token timestamps that follow from it (``Alignment``); ``inference(..., return_alignment=True)`` runs it on what it
    generated."""

    MODEL_NAME = "VALL-E"  # what the EOS line prints and get_model dispatches on (models/__init__.py:98-124)

    def __init__(self, d_model: int, nhead: int, num_layers: int, norm_first: bool = True, add_prenet: bool = False,
                 prefix_mode: int = 0, share_embedding: bool = True, nar_scale_factor: float = 1.0, **kwargs):
        self.engine_opts = dict(
            precision=kwargs.pop("precision", "bf16"), max_text=kwargs.pop("max_text", 512),
            max_audio=kwargs.pop("max_audio", 4096), trace_logits=kwargs.pop("trace_logits", False),
            no_graph=kwargs.pop("no_graph", False), simple_rows=kwargs.pop("simple_rows", False),
            max_batch=kwargs.pop("max_batch", 0), kv_cache=kwargs.pop("kv_cache", "bf16"),
            batched_rows=bool(kwargs.pop("batched_rows", False)), logprobs=bool(kwargs.pop("logprobs", False)))
        self.sampling = kwargs.pop("sampling", "device")
        self.print_eos = kwargs.pop("print_eos", True)
        self.cfg = ModelConfig(model_name=self.MODEL_NAME, decoder_dim=d_model, nhead=nhead, num_decoder_layers=num_layers, norm_first=norm_first,
                               add_prenet=add_prenet, prefix_mode=prefix_mode, share_embedding=share_embedding,
                               scale_factor=nar_scale_factor, prepend_bos=kwargs.pop("prepend_bos", False),
                               num_quantizers=kwargs.pop("num_quantizers", 8))
        if kwargs:
            raise TypeError(f"unexpected arguments {sorted(kwargs)}")
        kv = self.engine_opts["kv_cache"]
        if kv not in ("bf16", "fp8"):
            raise ValueError(f"kv_cache must be 'bf16' or 'fp8', got {kv!r}")
        if kv == "fp8":  # the engine refuses these too (VX_FLAG_KV_FP8); here they fail before an engine exists
            if self.engine_opts["max_batch"] < 2:
                raise NotImplementedError("kv_cache='fp8' is the batched decode's slot cache: it needs max_batch >= 2")
            if self.engine_opts["precision"] not in ("bf16", "fp8nar"):
                raise NotImplementedError("kv_cache='fp8' needs precision 'bf16' or 'fp8nar'")
            if not norm_first or add_prenet or self.cfg.is_vallf:
                raise NotImplementedError("kv_cache='fp8' needs a pre-norm VALL-E without prenets")
            if d_model % nhead or d_model // nhead != 64:
                raise NotImplementedError("kv_cache='fp8' needs head_dim 64")
        if self.engine_opts["batched_rows"]:  # the engine refuses these too (VX_FLAG_VALLF_ROWS); here they fail before one exists
            if not self.cfg.is_vallf:
                raise ValueError("batched_rows=True is the VALL-F option: a VALL-E model batches its prefill, admission and NAR as it is")
            if self.engine_opts["max_batch"] < 2:
                raise NotImplementedError("batched_rows=True needs max_batch >= 2")
            if not norm_first or add_prenet or self.engine_opts["simple_rows"]:
                raise NotImplementedError("batched_rows=True needs a pre-norm VALL-F without prenets on the MFMA row kernels")
        if (not norm_first or add_prenet) and self.engine_opts.get("max_batch", 0) > 1:
            raise NotImplementedError("norm_first=False / add_prenet=True run on the batch-1 path only (inference_batch needs the defaults)")
        if self.cfg.is_vallf and self.engine_opts["max_batch"] > 1:  # the engine refuses these too (vx_create)
            if self.engine_opts["precision"] != "bf16":
                raise NotImplementedError("VALL-F with max_batch >= 2 needs precision 'bf16'")
            if d_model % nhead or d_model // nhead != 64:
                raise NotImplementedError("VALL-F with max_batch >= 2 needs head_dim 64")
        if self.cfg.is_vallf and self.engine_opts["precision"] == "fp8nar":
            raise NotImplementedError("precision 'fp8nar' is built for VALL-E only")
        # head_dim 64 is the tuned geometry; 4/8/16/32 (the reference's own test: decoder_dim 64, nhead 16, valle_test.py:93-95)
        # run on the plain kernels, batch-1 only
        hds = [d_model // nhead if nhead > 0 and d_model % nhead == 0 else 0]
        if self.cfg.num_quantizers > 1:
            hds.append(self.cfg.nar_dim // self.cfg.nar_nhead if self.cfg.nar_nhead > 0 and self.cfg.nar_dim % self.cfg.nar_nhead == 0 else 0)
        if any(h not in (4, 8, 16, 32, 64) for h in hds):
            raise NotImplementedError(f"head_dim must be 4, 8, 16, 32 or 64 (got {hds}; DESIGN.md)")
        if any(h != 64 for h in hds) and self.engine_opts.get("max_batch", 0) > 1:
            raise NotImplementedError("inference_batch needs head_dim 64")
        if self.engine_opts.get("max_batch", 0) > 1 and d_model not in BATCH_WIDTHS:  # the engine refuses these too (vx_create)
            raise NotImplementedError(f"batched decode (max_batch >= 2) needs d_model in {BATCH_WIDTHS} (got {d_model}; DESIGN.md 4.3)")
        self.ar_audio_prepend_bos = self.cfg.prepend_bos
        self.num_quantizers = self.cfg.num_quantizers
        self.prefix_mode = prefix_mode
        self.num_heads = nhead
        self.device = torch.device("cpu")
        self.training = True
        self._engine = None
        # nn.Module would random-init here; same distributions, fresh seed from the global RNG
        self._sd = synthetic_state_dict(self.cfg, seed=int(torch.randint(0, 2**31 - 1, (1,))), zero_eos=False)

    # ---- nn.Module-like surface used by bin/infer.py:137-148 ---------------------------------------
    def state_dict(self):
        return OrderedDict(self._sd)

    def load_state_dict(self, state_dict, strict: bool = True):
        want = expected_keys(self.cfg)
        missing = [k for k in want if k not in state_dict]
        unexpected = [k for k in state_dict if k not in want]
        bad = [k for k in want if k in state_dict and tuple(state_dict[k].shape) != tuple(want[k])]
        if bad or (strict and (missing or unexpected)):
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}: missing {missing}, unexpected {unexpected}, "
                               f"size mismatch {bad}")
        for k in want:
            if k in state_dict:
                keep = k.endswith("num_batches_tracked")  # int64 scalar of BatchNorm1d
                self._sd[k] = state_dict[k].detach().to("cpu", state_dict[k].dtype if keep else torch.float32).contiguous()
        if self.cfg.share_embedding:  # valle.py:261-271: tied tensors are one storage
            for pk, ek in tied_keys(self.cfg).items():
                if pk in state_dict and ek in state_dict and not torch.equal(self._sd[pk], self._sd[ek]):
                    raise RuntimeError(f"tied weights differ: {pk} vs {ek}")
        self._drop_engine()
        return _IncompatibleKeys(missing, unexpected)

    def _drop_engine(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    def to(self, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._drop_engine()
        return self

    def cuda(self, index: int = 0):
        return self.to(torch.device("cuda", index))

    def eval(self):
        self.training = False
        return self

    def engine(self):
        """Creates the HIP engine on first use; there is no CPU path."""
        if self._engine is None:
            if self.device.type != "cuda":
                raise RuntimeError("valle_amd.VALLE runs only on an MI355X: call .to('cuda') first (no CPU fallback)")
            from .engine import Engine

            self._engine = Engine(self.cfg, device=self.device.index or 0, **self.engine_opts)
            self._engine.load_state_dict(self._sd)
        return self._engine

    # ---- the hot path -------------------------------------------------------------------------------
    @torch.no_grad()
    def inference(self, x: torch.Tensor, x_lens: torch.Tensor, y: torch.Tensor, enroll_x_lens: Optional[torch.Tensor],
                  top_k: int = -100, temperature: float = 1.0, exp_noise: Optional[torch.Tensor] = None,
                  max_new_tokens: int = -1, top_p: float = 1.0, return_logprobs: bool = False,
                  return_alignment: bool = False) -> torch.Tensor:
        """Same contract as the reference (valle.py:961-985): x (1,S) int64, x_lens (1,), y (1,P,8) int64 →
        (1,T,num_quantizers) int64 on the model's device.  ``exp_noise`` / ``max_new_tokens`` / ``top_p`` are extras.
        This batch-1 path keeps its own bf16 KV cache on every model, ``kv_cache="fp8"`` included (that option only
        changes the slot caches of ``inference_batch`` / ``inference_stream``).  ``return_logprobs=True`` (models built with
        ``logprobs=True``): returns ``(codes, GenLogProbs)``.  ``return_alignment=True``: ``align`` of the prompt plus the
        generated codes follows the synthesis and the call returns ``(codes, Alignment)`` (with both flags ``(codes, GenLogProbs,
        Alignment)``); the codes are those of the same call without the flag."""
        top_p = _check_top_p(top_p)
        self._check_logprobs(return_logprobs)
        if return_alignment:
            res = self.inference(x, x_lens, y, enroll_x_lens, top_k=top_k, temperature=temperature, exp_noise=exp_noise,
                                 max_new_tokens=max_new_tokens, top_p=top_p, return_logprobs=return_logprobs)
            codes = res[0] if return_logprobs else res
            Q = self.num_quantizers
            full = torch.cat([y[:, :, :Q].to(codes.device), codes], 1)
            al = self.align(x, x_lens, full, y.shape[1], enroll_x_lens=enroll_x_lens)
            return (codes, res[1], al) if return_logprobs else (codes, al)
        u = (x, x_lens, y, enroll_x_lens)
        self._check_utterance(u)
        eng = self.engine()
        S, P, bos = x.shape[1], y.shape[1], int(self.ar_audio_prepend_bos)
        eng.ar_prefill(x[0], y[0, :, 0].contiguous())
        n_max = max(1, 16 * S + 2 - bos)
        rng_state = None
        seed = 0
        if exp_noise is None and self.sampling == "torch_cpu":
            rng_state = torch.get_rng_state()
            exp_noise = torch.stack([torch.empty(1, NUM_AUDIO_TOKENS + 1).exponential_(1)[0] for _ in range(n_max)])
        elif exp_noise is None:
            seed = int(torch.randint(0, 2**62, (1,)))
        eng.ar_decode(top_k=top_k, temperature=temperature, exp_noise=exp_noise, seed=seed, max_new_tokens=max_new_tokens,
                      top_p=top_p)
        tokens, reason, n_pass = eng.ar_result()
        lp_ar = eng.ar_logprobs() if return_logprobs else None
        if rng_state is not None:
            # leave the global generator where the reference would: one draw per executed pass, including
            # the pass that trips the stop rule (valle.py:1040-1055)
            torch.set_rng_state(rng_state)
            for _ in range(tokens.numel() + 1):
                torch.empty(1, NUM_AUDIO_TOKENS + 1).exponential_(1)
        r = self._ar_finished(u, tokens, max_new_tokens)
        if self.print_eos:
            print(f"{self.MODEL_NAME} EOS [{P} -> {P + bos + tokens.numel()}]")  # valle.py:1054 / 646
        if isinstance(r, torch.Tensor):
            return (r, GenLogProbs(lp_ar, None, tokens.numel(), reason)) if return_logprobs else r
        codes = eng.nar(*r, out_device=self.device).unsqueeze(0)
        if return_logprobs:
            return codes, GenLogProbs(lp_ar, eng.nar_logprobs(0, tokens.numel()), tokens.numel(), reason)
        return codes


    @torch.no_grad()
    def inference_batch(self, utterances, top_k: int = -100, temperature: float = 1.0, seeds=None, batched_nar: bool = True,
                        batched_prefill: bool = True, top_p: float = 1.0, return_logprobs: bool = False,
                        return_alignment: bool = False):
        """Engine extension (BASELINE configs[2]): ``utterances`` = list of (x, x_lens, y[, enroll_x_lens]) as for
        ``inference``; up to ``max_batch`` of them advance together, one shared weight stream per AR step, each with
        its own KV cache / sampler / stop rule; the NAR stages then run per utterance.  Returns a list of (1,T_i,Q), with
        ``return_logprobs=True`` (models built with ``logprobs=True``) a list of ((1,T_i,Q), GenLogProbs).
        ``return_alignment=True``: after a group's NAR stages one ``align_batch`` runs over the prompt plus the generated codes of
        the group, and every entry gains its ``Alignment`` (None for an empty output), placed as ``inference`` places it; the
        codes are those of the same call without the flag."""
        top_p = _check_top_p(top_p)
        self._check_logprobs(return_logprobs)
        eng = self._batch_engine("inference_batch")
        Q = self.num_quantizers
        out = [None] * len(utterances)
        for g0 in range(0, len(utterances), eng.max_batch):
            group = utterances[g0 : g0 + eng.max_batch]
            sd = self._ar_group(eng, group, None if seeds is None else list(seeds[g0 : g0 + len(group)]), top_k, temperature, top_p,
                                batched_prefill)
            todo = []  # (index, text_nar, prompts, tokens) of the utterances that go through the NAR stages
            glp = {}   # index -> GenLogProbs (return_logprobs)
            for b, u in enumerate(group):
                lp_ar = eng.batch_logprobs(b) if return_logprobs else None
                tokens, reason = eng.batch_result(b)
                if return_logprobs:
                    glp[g0 + b] = GenLogProbs(lp_ar, None, tokens.numel(), reason)
                r = self._ar_finished(u, tokens)
                if isinstance(r, torch.Tensor):
                    out[g0 + b] = r
                else:
                    todo.append((g0 + b,) + r)
            for i, r in self._run_nar(eng, todo, batched_nar, glp if return_logprobs else None):
                out[i] = r
            als = self._align_generated(group, out[g0 : g0 + len(group)]) if return_alignment else None
            for b in range(len(group)):
                i = g0 + b
                if return_logprobs or return_alignment:
                    out[i] = (out[i],) + ((glp[i],) if return_logprobs else ()) + ((als[b],) if return_alignment else ())
        return out

    def _align_generated(self, group, codes):
        """One ``align_batch`` over prompt + generated codes of a group: ``codes[b]`` (1, T_b, Q) belongs to ``group[b]``; an
        utterance with an empty output gets None."""
        Q = self.num_quantizers
        idx = [b for b, c in enumerate(codes) if c.shape[1] > 0]
        full = [(group[b][0], group[b][1], torch.cat([group[b][2][:, :, :Q].to(codes[b].device), codes[b]], 1),
                 group[b][3] if len(group[b]) > 3 else None) for b in idx]
        out = [None] * len(codes)
        for b, al in zip(idx, self.align_batch(full, [int(group[b][2].shape[1]) for b in idx])):
            out[b] = al
        return out

    def _ar_group(self, eng, group, seeds, top_k, temperature, top_p, batched_prefill):
        """Prefills ``group`` (at most max_batch utterances) into slots 0.. and decodes them together; returns the seeds used
        (drawn from torch's global generator when none are given)."""
        for b, u in enumerate(group):
            x, y = u[0], u[2]
            self._check_utterance(u)
            if not (batched_prefill and eng.mfma_rows):
                eng.batch_prefill(b, x[0], y[0, :, 0].contiguous())
        if batched_prefill and eng.mfma_rows:  # one pass over the concatenated rows of the whole group
            eng.batch_prefill_all([u[0][0] for u in group], [u[2][0, :, 0].contiguous() for u in group])
        sd = [int(torch.randint(0, 2**62, (1,))) for _ in group] if seeds is None else seeds
        eng.batch_decode(len(group), top_k=top_k, temperature=temperature, seeds=sd, top_p=top_p)
        return sd

    @torch.no_grad()
    def inference_best_of(self, x: torch.Tensor, x_lens: torch.Tensor, y: torch.Tensor, enroll_x_lens: Optional[torch.Tensor],
                          n: int, top_k: int = -100, temperature: float = 1.0, top_p: float = 1.0, seeds=None, rank_by="logprob"):
        """Engine extension: best-of-N synthesis.  The utterance (arguments as for ``inference``) is sampled ``n`` times with
        ``n`` different seeds (``seeds``, or drawn as ``inference_batch`` draws them) in the slots of the batched decode, in
        groups of max_batch; the candidates are ranked by their mean AR log-probability (GenLogProbs.ar_mean, which the decode
        itself recorded: no scoring pass), highest first, ties to the lower index, and the NAR stages run for the winner only.
        Returns ``(codes (1,T,Q), BestOf)``; the codes are what ``inference_batch`` returns for the utterance with the winner's
        seed.  Needs a model built with ``logprobs=True`` (ValueError) and ``max_batch >= 2`` (NotImplementedError).
        ``rank_by="alignment"``: the candidates' prompt + AR tokens are aligned in one ``align_batch`` before any NAR stage (the
        AR pass reads codebook 0 only; the other codebooks of the generated frames are zeros) and ranked by ``alignment_rank_key``,
        the best path's score per frame: a candidate without a path or without output ranks last, ties go to the higher
        ``ar_mean``, then the lower index, and when no candidate has a path the order is the log-probability's.  A callable
        ``rank_by(alignment, genlogprobs) -> float`` (higher is better; ``alignment`` is None for an empty output) takes the place
        of that key under the same rules.  ``BestOf.alignments`` and ``BestOf.rank_key`` report both.  Which key picks the better
        audio on a trained checkpoint is NOT validated here: the weights this project tests with are synthetic, so the mechanics
        are tested, not the quality."""
        if not (rank_by in ("logprob", "alignment") or callable(rank_by)):
            raise ValueError(f"rank_by must be 'logprob', 'alignment' or a callable (got {rank_by!r})")
        top_p = _check_top_p(top_p)
        self._check_logprobs(True, "inference_best_of")
        if self.engine_opts["max_batch"] < 2:
            raise NotImplementedError("inference_best_of decodes its candidates in the slots of the batched decode: it needs max_batch >= 2")
        n = int(n)
        if n < 1:
            raise ValueError(f"n must be >= 1 (got {n})")
        if seeds is not None and len(seeds) != n:
            raise ValueError(f"{len(seeds)} seeds for n = {n} candidates")
        u = (x, x_lens, y, enroll_x_lens)
        self._check_utterance(u)
        eng = self._batch_engine("inference_best_of")
        rows = self.engine_opts["batched_rows"] if self.cfg.is_vallf else True  # as inference_batch's defaults on this model
        used, cands = [], []
        for g0 in range(0, n, eng.max_batch):
            k = min(eng.max_batch, n - g0)
            used += self._ar_group(eng, [u] * k, None if seeds is None else [int(s) for s in seeds[g0 : g0 + k]], top_k, temperature,
                                   top_p, rows)
            for b in range(k):
                lp_ar = eng.batch_logprobs(b)
                tokens, reason = eng.batch_result(b)
                cands.append((tokens, GenLogProbs(lp_ar, None, tokens.numel(), reason)))
        means = [c[1].ar_mean for c in cands]
        als, keys = None, means
        if rank_by == "logprob":
            w = best_of_index(means)
        else:
            Q = self.num_quantizers
            gen = []  # prompt + AR tokens of every candidate that emitted something
            for tk, _ in cands:
                if tk.numel():
                    rows_ = torch.zeros((1, tk.numel(), Q), dtype=torch.int64, device=y.device)
                    rows_[0, :, 0] = tk.to(y.device)
                    gen.append((x, x_lens, torch.cat([y[:, :, :Q], rows_], 1), enroll_x_lens))
            done = iter(self.align_batch(gen, int(y.shape[1])))
            als = [next(done) if c[0].numel() else None for c in cands]
            key = alignment_rank_key if rank_by == "alignment" else rank_by
            keys = [float(key(a, c[1])) for a, c in zip(als, cands)]
            w = best_of_rank(keys, means)
        tokens, lp = cands[w]
        glp = {0: lp}
        r = self._ar_finished(u, tokens)
        codes = r if isinstance(r, torch.Tensor) else self._run_nar(eng, [(0,) + r], rows, glp)[0][1]
        return codes, BestOf(w, used, means, [c[0] for c in cands], lp, als, list(keys))

    # ---- shared by inference, inference_batch and inference_stream ------------------------------------
    def _check_logprobs(self, wanted: bool, what: str = "return_logprobs=True"):
        if wanted and not self.engine_opts["logprobs"]:
            raise ValueError(f"{what} needs a model built with logprobs=True (VX_FLAG_LOGPROBS)")

    def _batch_engine(self, what: str):
        eng = self.engine()
        if eng.max_batch < 2:
            raise RuntimeError(f"construct the model with max_batch >= 2 for {what}")
        return eng

    def _check_utterance(self, u):
        """The reference's checks of one (x, x_lens, y[, enroll_x_lens]) (valle.py:986-991)."""
        x, x_lens, y = u[0], u[1], u[2]
        assert x.ndim == 2 and x_lens.ndim == 1 and y.ndim == 3 and y.shape[0] == 1 and torch.all(x_lens > 0)
        S = int(x_lens.max())
        if x.shape[1] != S or x.shape[0] != 1:
            # the reference builds its mask from x_lens.max() but concatenates all of x: any padding makes
            # its attention shapes disagree (valle.py:1009-1038)
            raise RuntimeError(f"x must be one unpadded sequence: x {tuple(x.shape)} vs x_lens.max() {S}")
        if _ids_out_of_range(x, y[..., :self.num_quantizers]):
            raise IndexError("index out of range in self")  # what nn.Embedding raises in the reference

    def _ar_finished(self, u, tokens, max_new_tokens: int = -1):
        """An utterance's AR tokens -> its final (1, T, Q) codes when no NAR stage runs (Q == 1, empty output), else the
        (text_nar, prompts, tokens) of its NAR stages (prefix-mode 2/4 trim, valle.py:1068-1079).  An empty output without
        a BOS row is the reference's SyntaxError (valle.py:1049-1052), unless max_new_tokens == 0 asked for it."""
        Q, bos = self.num_quantizers, int(self.ar_audio_prepend_bos)
        x, y = u[0], u[2]
        enroll = u[3] if len(u) > 3 else None
        if tokens.numel() == 0 and not bos and max_new_tokens != 0:
            raise SyntaxError("well trained model shouldn't reach here.")
        if Q == 1 or tokens.numel() == 0:
            codes = torch.zeros((tokens.numel(), Q), dtype=torch.int64)
            codes[:, 0] = tokens
            return codes.unsqueeze(0).to(self.device)
        text_nar = x[0]
        if self.prefix_mode in [2, 4]:
            enrolled_len = int(enroll.max().item())
            text_nar = torch.concat([x[0][:1], x[0][enrolled_len - 1:]])
        return (text_nar, y[0, :, :Q].contiguous(), tokens)

    def _run_nar(self, eng, todo, batched_nar: bool, glp=None):
        """[(index, text_nar, prompts, tokens)] -> [(index, (1, T, Q) codes)]: one vx_nar_batch over all, or vx_nar each.
        ``glp`` (index -> GenLogProbs): each utterance's ``nar`` is filled in from the call that ran its stages."""
        if todo and batched_nar:
            res = eng.nar_batch([t[1] for t in todo], [t[2] for t in todo], [t[3] for t in todo], out_device=self.device)
            if glp is not None:
                for z, t in enumerate(todo):
                    glp[t[0]].nar = eng.nar_logprobs(z, t[3].numel())
            return [(t[0], r.unsqueeze(0)) for t, r in zip(todo, res)]
        out = []
        for i, tn, pr, tk in todo:
            out.append((i, eng.nar(tn, pr, tk, out_device=self.device).unsqueeze(0)))
            if glp is not None:
                glp[i].nar = eng.nar_logprobs(0, tk.numel())
        return out

    @torch.no_grad()
    def inference_stream(self, utterances, top_k: int = -100, temperature: float = 1.0, seeds=None, nar_group=None,
                         poll_steps: int = 0, batched_admit: bool = True, batched_nar: bool = True, refill_at=None,
                         top_p: float = 1.0, return_logprobs: bool = False, return_alignment: bool = False):
        """Engine extension: continuous batching.  A generator over ``utterances`` (as for ``inference_batch``) that yields
        ``(index, codes)``, codes (1, T_i, Q) as ``inference_batch`` returns them, as utterances finish.  A slot whose utterance
        stopped is refilled from the queue while the others keep decoding: new utterances are admitted once ``refill_at``
        slots are free (default max_batch // 16, at least 1) and whenever the rest of the queue fits.  Finished utterances
        wait for their NAR stages until ``nar_group`` (default max_batch) are pending or the queue is empty.  ``seeds[i]``
        belongs to utterance i, so the codes do not depend on the schedule.  ``batched_admit=False`` prefills slot by slot
        (bitwise the static path); ``poll_steps``: steps between stop polls (0: the engine default).  ``return_logprobs=True``
        (models built with ``logprobs=True``): yields ``(index, (codes, GenLogProbs))``.  ``return_alignment=True``: one
        ``align_batch`` follows the NAR stages of every NAR group, over the prompt plus the generated codes of that group, and the
        yield gains the ``Alignment`` (None for an empty output) as in ``inference_batch``."""
        top_p = _check_top_p(top_p)
        self._check_logprobs(return_logprobs)
        eng = self._batch_engine("inference_stream")
        utterances = list(utterances)
        for u in utterances:
            self._check_utterance(u)
        N, B = len(utterances), eng.max_batch
        if seeds is None:
            seeds = [int(torch.randint(0, 2**62, (1,))) for _ in utterances]
        elif len(seeds) < N:
            raise ValueError(f"{len(seeds)} seeds for {N} utterances")
        refill_at = max(1, B // 16) if refill_at is None else max(1, int(refill_at))
        nar_group = B if nar_group is None else max(1, int(nar_group))
        batched_admit = batched_admit and eng.mfma_rows
        return self._stream(eng, utterances, seeds, top_k, temperature, nar_group, poll_steps, batched_admit, batched_nar, refill_at,
                            top_p, return_logprobs, return_alignment)

    def _stream(self, eng, utterances, seeds, top_k, temperature, nar_group, poll_steps, batched_admit, batched_nar, refill_at,
                top_p=1.0, return_logprobs=False, return_alignment=False):
        N, B = len(utterances), eng.max_batch
        glp = {} if return_logprobs else None  # index -> GenLogProbs of the utterances not yet yielded

        def give(i, c, al=None):
            if not (return_logprobs or return_alignment):
                return i, c
            return i, (c,) + ((glp.pop(i),) if return_logprobs else ()) + ((al,) if return_alignment else ())

        eng.batch_open()
        free = list(range(B))
        live = {}      # slot -> utterance index
        pending = []   # (index, text_nar, prompts, tokens) waiting for the NAR stages
        nxt = 0        # next utterance of the queue
        while nxt < N or live or pending:
            k = min(len(free), N - nxt)
            if k and (k >= refill_at or k == N - nxt or not live):
                slots, free = free[:k], free[k:]
                us = utterances[nxt : nxt + k]
                eng.batch_admit(slots, [u[0][0] for u in us], [u[2][0, :, 0].contiguous() for u in us], top_k=top_k,
                                temperature=temperature, seeds=seeds[nxt : nxt + k], batched=batched_admit, top_p=top_p)
                live.update((s, nxt + z) for z, s in enumerate(slots))
                nxt += k
            if live:
                need = 1 if nxt >= N else max(1, refill_at - len(free))
                for s in eng.batch_run(need, poll_steps):
                    i = live.pop(s)
                    lp_ar = eng.batch_logprobs(s) if return_logprobs else None  # while the slot is STOPPED: the result vacates it
                    tokens, reason = eng.batch_result(s)
                    if return_logprobs:
                        glp[i] = GenLogProbs(lp_ar, None, tokens.numel(), reason)
                    free.append(s)
                    r = self._ar_finished(utterances[i], tokens)
                    if isinstance(r, torch.Tensor):
                        yield give(i, r)
                    else:
                        pending.append((i,) + r)
            if pending and (len(pending) >= nar_group or nxt >= N):
                done, pending = pending, []
                res = self._run_nar(eng, done, batched_nar, glp)
                als = self._align_generated([utterances[i] for i, _ in res], [c for _, c in res]) if return_alignment else [None] * len(res)
                for (i, c), al in zip(res, als):
                    yield give(i, c, al)

    # ---- scoring ---------------------------------------------------------------------------------------
    def _score_args(self, x, x_lens, y, prompt_frames, enroll_x_lens, top_k):
        """Checks of one utterance to score, as ``inference``'s, -> (text, text_nar, codes (A, Q), P)."""
        self._check_utterance((x, x_lens, y, enroll_x_lens))
        Q, bos = self.num_quantizers, int(self.ar_audio_prepend_bos)
        A, P = int(y.shape[1]), int(prompt_frames)
        if y.shape[2] < Q:
            raise ValueError(f"y has {y.shape[2]} codebooks, the model {Q}")
        if not 0 <= P < A:
            raise ValueError(f"prompt_frames must be in [0, {A}) (got {P})")
        if P == 0 and not bos:
            raise ValueError("prompt_frames=0 needs prepend_bos: without a BOS row nothing predicts the first frame")
        if int(top_k) < 1:
            raise ValueError(f"top_k must be >= 1 (got {top_k})")
        text_nar = x[0]
        if self.prefix_mode in [2, 4] and enroll_x_lens is not None:  # the NAR text trim of inference (valle.py:1068-1079)
            enrolled_len = int(enroll_x_lens.max().item())
            text_nar = torch.concat([x[0][:1], x[0][enrolled_len - 1:]])
        return x[0], text_nar, y[0, :, :Q].contiguous(), P

    @staticmethod
    def _score_result(codes, P, parts, top_k) -> ScoreResult:
        an, ak, nn_, nk = parts
        eos = torch.full((1,), NUM_AUDIO_TOKENS, dtype=torch.int64, device=codes.device)
        return aggregate_score(an, ak, torch.cat([codes[P:, 0], eos]), nn_, nk, codes[P:, 1:].t(), top_k)

    @torch.no_grad()
    def score(self, x: torch.Tensor, x_lens: torch.Tensor, y: torch.Tensor, prompt_frames: int = 0, top_k: int = 10,
              enroll_x_lens: Optional[torch.Tensor] = None) -> ScoreResult:
        """Engine extension: how well the model predicts the given codes, teacher-forced (vx_score).  x (1,S), x_lens (1,), y
        (1,A,Q) as for ``inference``; the first ``prompt_frames`` frames of y are the prompt, the others are scored.  With
        ``prompt_frames=0`` on a prepend_bos model (or 1 without BOS) ``ar_loss`` / ``ar_topk_acc`` are the reference's summed
        AR loss and ArTop10Accuracy of VALLE.forward at batch size 1 (valle.py:863-881).  ``enroll_x_lens``: the text trim of
        prefix modes 2 / 4, as in ``inference``."""
        text, text_nar, codes, P = self._score_args(x, x_lens, y, prompt_frames, enroll_x_lens, top_k)
        return self._score_result(codes, P, self.engine().score(text, text_nar, codes, P), top_k)

    @torch.no_grad()
    def score_batch(self, utterances, prompt_frames=0, top_k: int = 10) -> List[ScoreResult]:
        """``score`` of several utterances, (x, x_lens, y[, enroll_x_lens]) each; ``prompt_frames``: one value or one per
        utterance.  Groups of at most max_batch (64 on a batch-1 engine) go through one pass over the concatenated rows
        (vx_score_batch); where the engine has no such pass (fp32, VALL-F, prenets, other head sizes) every utterance is
        scored by itself."""
        from .engine import BMAX, VxError

        eng = self.engine()
        Ps = list(prompt_frames) if isinstance(prompt_frames, (list, tuple)) else [prompt_frames] * len(utterances)
        if len(Ps) != len(utterances):
            raise ValueError(f"{len(Ps)} prompt_frames for {len(utterances)} utterances")
        args = [self._score_args(u[0], u[1], u[2], p, u[3] if len(u) > 3 else None, top_k) for u, p in zip(utterances, Ps)]
        group = eng.max_batch if eng.max_batch >= 2 else BMAX
        out = []
        for g0 in range(0, len(args), group):
            g = args[g0 : g0 + group]
            try:
                parts = eng.score_batch([a[0] for a in g], [a[1] for a in g], [a[2] for a in g], [a[3] for a in g])
            except VxError as err:
                if err.code != 5:  # VX_ERR_UNSUPPORTED: exactly where vx_score_batch refuses
                    raise
                parts = [eng.score(*a) for a in g]
            out += [self._score_result(a[2], a[3], p, top_k) for a, p in zip(g, parts)]
        return out

    # ---- alignment -------------------------------------------------------------------------------------
    def _align_args(self, x, x_lens, y, prompt_frames, enroll_x_lens, heads):
        """Checks of one utterance to align, before any engine exists -> (text, codes (A, Q), P, c0, head weights or None)."""
        text, _, codes, P = self._score_args(x, x_lens, y, prompt_frames, enroll_x_lens, 10)
        S = int(text.numel())
        c0 = 0 if enroll_x_lens is None else int(torch.as_tensor(enroll_x_lens).max().item())
        if not 0 <= c0 < S:
            raise ValueError(f"enroll_x_lens={c0}: the text window [{c0}, {S}) is empty or outside the text")
        return text, codes, P, c0, head_weights(heads, self.cfg.num_decoder_layers, self.cfg.nhead)

    @torch.no_grad()
    def align(self, x: torch.Tensor, x_lens: torch.Tensor, y: torch.Tensor, prompt_frames: int,
              enroll_x_lens: Optional[torch.Tensor] = None, heads=None, per_head: bool = False) -> Alignment:
        """Engine extension: when is each text token spoken (vx_align).  x (1,S), x_lens (1,), y (1,A,Q) as for ``score``: the
        first ``prompt_frames`` frames of y are the prompt, and the attention of the AR decoder over the text is taken, teacher-
        forced, on the rows that predict the other T = A - prompt_frames frames.  The text window is [enroll_x_lens or 0, S): with
        a transcribed prompt the generated frames speak only the text after it.  ``heads``: None (every head of every layer,
        uniform), a list of (layer, head) pairs (uniform over them) or an (L, H) tensor of weights (normalised to sum 1).
        ``per_head=True`` also returns every head's own map, to pick alignment heads on a trained checkpoint."""
        text, codes, P, c0, hw = self._align_args(x, x_lens, y, prompt_frames, enroll_x_lens, heads)
        attn, mass, path, score, ph = self.engine().align(text, codes, P, c0=c0, head_w=hw, per_head=per_head)
        return make_alignment(attn, mass, path, score, ph)

    def _align_batch_args(self, utterances, prompt_frames, heads):
        """Checks of ``align_batch``'s arguments, before any engine exists -> [(text, codes, P, c0)], head weights or None."""
        utterances = list(utterances)
        Ps = list(prompt_frames) if isinstance(prompt_frames, (list, tuple)) else [prompt_frames] * len(utterances)
        if len(Ps) != len(utterances):
            raise ValueError(f"{len(Ps)} prompt_frames for {len(utterances)} utterances")
        hw = head_weights(heads, self.cfg.num_decoder_layers, self.cfg.nhead)
        args = []
        for u, p in zip(utterances, Ps):
            if not isinstance(u, (list, tuple)) or not 3 <= len(u) <= 4:
                raise ValueError("an utterance is (x, x_lens, y[, enroll_x_lens])")
            args.append(self._align_args(u[0], u[1], u[2], p, u[3] if len(u) > 3 else None, None)[:4])
        return args, hw

    @torch.no_grad()
    def align_batch(self, utterances, prompt_frames, heads=None) -> List[Alignment]:
        """``align`` of several utterances, (x, x_lens, y[, enroll_x_lens]) each; ``prompt_frames``: one value or one per
        utterance; ``heads`` as for ``align``, shared by all.  The window of each is [enroll_x_lens or 0, S), as in ``align``.
        Groups of at most 64 go through one pass over the concatenated rows with the attention tap on the matrix pipe
        (vx_align_batch): the maps agree with ``align``'s within the bf16 bound, not bit for bit.  Where the engine has no such
        pass (fp32, VALL-F, prenets, post-norm, other head sizes) every utterance is aligned by ``align``'s own call, so this
        works wherever ``align`` does."""
        from .engine import BMAX, VxError

        args, hw = self._align_batch_args(utterances, prompt_frames, heads)
        if not args:
            return []
        eng = self.engine()
        out = []
        for g0 in range(0, len(args), BMAX):
            g = args[g0 : g0 + BMAX]
            try:
                parts = eng.align_batch([a[0] for a in g], [a[1] for a in g], [a[2] for a in g], [a[3] for a in g], head_w=hw)
            except VxError as err:
                if err.code != 5:  # VX_ERR_UNSUPPORTED: exactly where vx_align_batch refuses
                    raise
                parts = [eng.align(a[0], a[1], a[2], c0=a[3], head_w=hw)[:4] for a in g]
            out += [make_alignment(*p) for p in parts]
        return out

    @torch.no_grad()
    def continual(self, x: torch.Tensor, x_lens: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """VALLE.continual (valle.py:1139-1238; reached by bin/infer.py:224-230 with --continual): the first half
        of y (at most 225 frames) is the prompt, codebook 0 of the rest is kept and its codebooks 1..7 are
        predicted by the NAR stages.  Returns (1, T - prefix_len, 8)."""
        assert x.ndim == 2, x.shape
        assert x_lens.ndim == 1, x_lens.shape
        assert y.ndim == 3, y.shape
        assert y.shape[0] == 1, y.shape
        assert torch.all(x_lens > 0)
        assert self.num_quantizers == 8
        if _ids_out_of_range(x, y):
            raise IndexError("index out of range in self")
        eng = self.engine()
        prefix_len = min(int(y.shape[1] * 0.5), 3 * 75)
        prompts = y[0, :prefix_len, :8].contiguous()
        rest0 = y[0, prefix_len:, 0].contiguous()
        codes = eng.nar(x[0], prompts, rest0, out_device=self.device, continual=True)
        return codes.unsqueeze(0)


class VALLF(VALLE):
    """The cross-attention variant (valle.py:49-719; ``--model-name VALL-F``): ``inference`` has VALLE.inference's signature and
    result (valle.py:566-710).  The text is embedded once as the memory of a TransformerDecoder whose target is the audio
    sequence alone; the reference masks memory positions >= x_lens (all-false for the unpadded batch-1 input it accepts).
    The reference's VALLF has no ``continual`` and no batched entry point.  This one has no ``continual`` either; built with
    ``max_batch >= 2`` (pre-norm, no prenets, head_dim 64, d_model in {128, 256, 512, 1024}, bf16) it has ``inference_batch`` and
    ``inference_stream``.  By default these prefill and admit slot by slot and run the NAR stages per utterance
    (``batched_prefill``, ``batched_admit`` and ``batched_nar`` are ignored).  Built with ``batched_rows=True`` as well
    (VX_FLAG_VALLF_ROWS) they honour the three switches as VALLE does: the prefill / admission of a group and the NAR stages of a
    group each run as one pass over the concatenated audio rows, with the cross-attention of every utterance over its own text
    memory.  The option costs a packed text-memory buffer for the batched NAR pass (2 nar_layers nar_dim bf16 per text row of a
    group) and is refused on a VALLE model."""

    MODEL_NAME = "VALL-F"

    def continual(self, *a, **k):
        raise AttributeError("'VALLF' object has no attribute 'continual'")  # valle.py:1139 defines it on VALLE only

    @torch.no_grad()
    def align_batch(self, utterances, prompt_frames, heads=None) -> List[Alignment]:
        """``align`` of every utterance in turn: the segmented row pass holds one text memory, so VALL-F has no batched tap."""
        args, hw = self._align_batch_args(utterances, prompt_frames, heads)
        eng = self.engine() if args else None
        return [make_alignment(*eng.align(a[0], a[1], a[2], c0=a[3], head_w=hw)[:4]) for a in args]

    def _vallf_batched(self, what: str):
        if self.engine_opts["max_batch"] < 2:
            raise NotImplementedError(f"VALL-F {what} needs a model built with max_batch >= 2 (otherwise batch-1 path only)")

    def inference_batch(self, utterances, top_k: int = -100, temperature: float = 1.0, seeds=None, batched_nar: bool = True,
                        batched_prefill: bool = True, top_p: float = 1.0, return_logprobs: bool = False,
                        return_alignment: bool = False):
        self._vallf_batched("inference_batch")
        rows = self.engine_opts["batched_rows"]
        return super().inference_batch(utterances, top_k=top_k, temperature=temperature, seeds=seeds, batched_nar=rows and batched_nar,
                                       batched_prefill=rows and batched_prefill, top_p=top_p, return_logprobs=return_logprobs,
                                       return_alignment=return_alignment)

    def inference_stream(self, utterances, top_k: int = -100, temperature: float = 1.0, seeds=None, nar_group=None,
                         poll_steps: int = 0, batched_admit: bool = True, batched_nar: bool = True, refill_at=None,
                         top_p: float = 1.0, return_logprobs: bool = False, return_alignment: bool = False):
        self._vallf_batched("inference_stream")
        rows = self.engine_opts["batched_rows"]
        return super().inference_stream(utterances, top_k=top_k, temperature=temperature, seeds=seeds, nar_group=nar_group,
                                        poll_steps=poll_steps, batched_admit=rows and batched_admit, batched_nar=rows and batched_nar,
                                        refill_at=refill_at, top_p=top_p, return_logprobs=return_logprobs,
                                        return_alignment=return_alignment)


def get_model(params):
    """models/__init__.py:98-136: --model-name VALL-E / VALL-F, and (anything else there) the mel-spectrogram ``Transformer``
    (models/__init__.py:125-134), which takes --scaling-xformers."""
    cfg = ModelConfig.from_params(params)
    get = params.get if isinstance(params, dict) else lambda k, d=None: getattr(params, k, d)
    if cfg.model_name == "Transformer":  # models/__init__.py:126 asserts this spelling
        # models/__init__.py:133 reads params.scaling_xformers unconditionally: the reference serves this model only from the full
        # argument set of add_model_arguments.  So does this factory - a params object without the field asks for a model variant
        # nobody named, and is refused rather than given a default (models.Transformer(...) takes the default directly).
        if get("scaling_xformers", None) is None:
            raise NotImplementedError("get_model(model_name='Transformer') needs params.scaling_xformers (add_model_arguments sets it; "
                                      "models/__init__.py:133 reads it unconditionally): the stock variant (False) is built, "
                                      "ScaledLinear / BasicNorm (True) is not - or construct valle_amd.models.Transformer directly")
        extra = {k: get(k) for k in ("precision", "max_text", "max_frames", "no_graph") if get(k, None) is not None}
        return Transformer(cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers, norm_first=cfg.norm_first, add_prenet=cfg.add_prenet,
                           scaling_xformers=bool(get("scaling_xformers", False)), **extra)
    if cfg.model_name.lower() in ("vall-f", "vallf"):
        cls = VALLF
    elif cfg.model_name.lower() in ("vall-e", "valle"):
        cls = VALLE
    else:
        raise NotImplementedError(f"model {cfg.model_name!r}: VALL-E, VALL-F and Transformer are built (DESIGN.md)")
    extra = {}
    for k in ("precision", "max_text", "max_audio", "sampling", "max_batch", "kv_cache", "batched_rows", "logprobs"):
        if get(k, None) is not None:
            extra[k] = get(k)
    return cls(cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers, norm_first=cfg.norm_first, add_prenet=cfg.add_prenet,
                 prefix_mode=cfg.prefix_mode, share_embedding=cfg.share_embedding, nar_scale_factor=cfg.scale_factor,
                 prepend_bos=cfg.prepend_bos, num_quantizers=cfg.num_quantizers, **extra)
