"""Shared inputs of the scoring tests (test_score_cpu.py, test_gpu_score.py): the models, the test utterance with its fp64
reference score (computed once per process), and the tolerances, which are those of test_gpu_engine.py.

The utterance.  Synthetic weights give AR logits of scale ~3 over 1025 entries: neighbouring values lie ~5e-3 apart, so a
uniformly random target has another entry within the fp32 margin (4e-4) in a quarter of the rows, for every seed.  A recording a
model is scored on is not a uniformly random sequence under that model, and the test utterance is not either: codebook 0 of every
scored frame is the oracle's own k-th most likely token given the frames before it, k = frame mod 10 (so every rank 0..9 occurs
and the values near the target are spaced like the top of the distribution), except every 8th frame, which keeps its random token
(ranks in the hundreds).  The choice uses the fp64 oracle only, never the engine.  Codebooks 1..Q-1 and the prompt stay random:
NAR logits have scale ~100 and decide 95 % of random rows as they are."""
import torch

import score_ref as sr

FP32_AR_TOL = 2e-4     # fp32 AR logits against the oracle (test_fp32_engine_reproduces_reference_codes)
FP32_NAR_REL = 1e-5    # fp32 NAR logits, as a fraction of the row's largest magnitude (test_nar_stages_teacher_forced_margin_rule)
BF16_REL_TOL = 0.03    # bf16 teacher-forced logits, same fraction (test_bf16_engine_teacher_forced, NAR_REL_TOL)
BF16_AGREE_MIN = 0.93  # argmax agreement floor of test_bf16_engine_teacher_forced
DECIDED_MIN = 0.9

_CACHE = {}


def config(**kw):
    from valle_amd.config import ModelConfig

    a = dict(decoder_dim=256, nhead=4, num_decoder_layers=2)
    a.update(kw)
    return ModelConfig(**a)


def utterance(cfg, S=7, A=70, P=5, seed=1, weight_seed=0, likely=True):
    """dict(cfg, sd, text (S,), codes (A, Q), P, x / x_lens / y as `inference` takes them, ref = the fp64 score).
    likely=False: every token stays random (ranks over the whole vocabulary; the margin decides fewer AR rows)."""
    key = (repr(cfg), S, A, P, seed, weight_seed, likely)
    if key in _CACHE:
        return _CACHE[key]
    from valle_amd.weights import synthetic_inputs, synthetic_state_dict

    sd = synthetic_state_dict(cfg, weight_seed)
    x, x_lens, y = synthetic_inputs(S, A, cfg.num_quantizers, seed=seed)
    text, codes = x[0], y[0].clone()
    m = sr.oracle(cfg, sd)
    for t in range(P, A):
        if t % 8 == 7 or not likely:
            continue
        row = sr.ar_score_logits(m, text, codes[:t], t)[0, :1024]  # the row that predicts frame t (an audio token, not EOS)
        codes[t, 0] = int(row.topk(10).indices[t % 10])
    u = dict(cfg=cfg, sd=sd, text=text, codes=codes, P=P, x=x, x_lens=x_lens, y=codes.unsqueeze(0), ref=sr.score(m, text, codes, P))
    _CACHE[key] = u
    return u


def absmax(logits):
    return logits.abs().amax(-1)


def decided_fp32(ref):
    """(AR rows, NAR (Q-1, T) rows) the fp32 tolerances decide."""
    d_ar = sr.decided(ref["ar_logits"], ref["ar_targets"], FP32_AR_TOL)
    if "nar_logits" not in ref:
        return d_ar, None
    d_nar = torch.stack([sr.decided(l, t, FP32_NAR_REL * absmax(l).double() + 1e-6) for l, t in zip(ref["nar_logits"], ref["nar_targets"])])
    return d_ar, d_nar


def decided_bf16(ref):
    d_ar = sr.decided(ref["ar_logits"], ref["ar_targets"], BF16_REL_TOL * absmax(ref["ar_logits"]).double())
    if "nar_logits" not in ref:
        return d_ar, None
    d_nar = torch.stack([sr.decided(l, t, BF16_REL_TOL * absmax(l).double()) for l, t in zip(ref["nar_logits"], ref["nar_targets"])])
    return d_ar, d_nar
