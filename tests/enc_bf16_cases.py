"""The cases of the recognisers' bf16 encoder mode, shared by test_enc_bf16_cpu.py, test_gpu_whisper_bf16.py and test_gpu_asr_bf16.py.
The utterances, weights and prompts are whisper_cases' and asr_cases', unchanged; this file adds the rounding restatement
(enc_bf16_ref) of each, computed once and left unchanged, and the bounds.

Bound: the project's standing rule.  Engine max-abs error against the UNROUNDED fp64 restatement (whisper_ref / asr_ref) <=
TOL_FACTOR x floor, per tap and per utterance; the floor is the rounding restatement in torch fp32 on the host against that same
fp64.  Decisions are compared teacher-forced: a step (frame) is decided when fp64's top-two margin exceeds 2 x TOL_FACTOR x the
case's bf16 logits floor.  WHISPER_DECIDED_SHARE / CTC_DECIDED_SHARE of the steps / frames must be decided, every case must have a
decided one, and at least FULLY_DECIDED_CASES Whisper cases must be decided at every step (those are compared free-running)."""
import torch

import asr_cases as AC
import enc_bf16_ref as ER
import whisper_cases as WC

TOL_FACTOR = 4.0
WHISPER_DECIDED_SHARE = 0.70
CTC_DECIDED_SHARE = 0.60
FULLY_DECIDED_CASES = 6

# ---- Whisper ------------------------------------------------------------------------------------------------------------------------
WSP_GPU_GEOMETRIES = ("A", "C", "D", "B")  # B (d = 192, ffn 384) is served: both are multiples of 64
_WENC, _WFORCED, _TF = {}, {}, {}


def wsp_encoded(cid, dtype):
    """The rounding restatement's encoder taps of a case of whisper_cases.CASES."""
    key = (cid, dtype)
    if key not in _WENC:
        name = WC.CASES[cid][0]
        _WENC[key] = ER.whisper_encode(WC.state_dict(name), WC.config(name), WC.encoded(cid, dtype), dtype)
    return _WENC[key]


def wsp_forced(cid, dtype):
    """The teacher-forced raw logits of fp64's greedy tokens on the rounding restatement's encoder output."""
    key = (cid, dtype)
    if key not in _WFORCED:
        name = WC.CASES[cid][0]
        _WFORCED[key] = WC.R.forced_logits(WC.state_dict(name), WC.config(name), wsp_encoded(cid, dtype), WC.case_prompt(cid),
                                           WC.generated(cid)["tokens"], dtype)
    return _WFORCED[key]


def wsp_taps(cid, dtype):
    name = WC.CASES[cid][0]
    e = wsp_encoded(cid, dtype)
    out = {k: e[k] for k in WC.tap_names(name) if k != "logits"}
    out["logits"] = wsp_forced(cid, dtype)
    return out


def wsp_floors(cid):
    """tap -> max-abs error of the rounding restatement in fp32 against the unrounded fp64 restatement."""
    r64, r16 = WC.named_taps(cid, torch.float64), wsp_taps(cid, torch.float32)
    return {k: float((r16[k].double() - r64[k]).abs().max()) for k in r64}


def wsp_decided(cid):
    """Per generated step of fp64's greedy run: its margin exceeds 2 x TOL_FACTOR x the case's bf16 logits floor."""
    bound = 2 * TOL_FACTOR * wsp_floors(cid)["logits"]
    return [m > bound for m in WC.generated(cid)["margins"]]


def wsp_tf_taps(dtype):
    """The rounding restatement of whisper_cases' 260-token teacher-forced run on D."""
    if dtype not in _TF:
        name = WC.TF_CASE[0]
        sd, cfg = WC.state_dict(name), WC.config(name)
        base = WC.R.encode(sd, cfg, WC.tf_wave(), WC.mel(name), dtype)
        e = ER.whisper_encode(sd, cfg, base, dtype)
        out = {k: e[k] for k in WC.tap_names(name) if k != "logits"}
        out["logits"] = WC.R.forced_logits(sd, cfg, e, WC.tf_prompt(), WC.tf_tokens(), dtype)
        _TF[dtype] = out
    return _TF[dtype]


def wsp_tf_floors():
    r64, r16 = WC.tf_taps(torch.float64), wsp_tf_taps(torch.float32)
    return {k: float((r16[k].double() - r64[k]).abs().max()) for k in r64}


# ---- CTC ----------------------------------------------------------------------------------------------------------------------------
ASR_CASES = [("hd64_layer", f) for f in AC.FRAMES] + [("large2", f) for f in AC.WIDE_FRAMES]
_AREF = {}


def asr_reference(name, frames, dtype):
    key = (name, frames, dtype)
    if key not in _AREF:
        _AREF[key] = ER.asr_forward(AC.ref_state_dict(AC.state_dict(name)), AC.config(name), AC.reference(name, frames, dtype), dtype)
    return _AREF[key]


def asr_floors(name, frames):
    r64, r16 = AC.named_taps(AC.reference(name, frames, torch.float64)), AC.named_taps(asr_reference(name, frames, torch.float32))
    return {k: float((r16[k].double() - r64[k]).abs().max()) for k in r64}


def asr_decided_frames(name, frames):
    """(fp64 argmax per frame, mask of the frames whose fp64 top-two margin exceeds 2 x TOL_FACTOR x the bf16 logits floor)."""
    lg = AC.reference(name, frames, torch.float64)["logits"]
    if lg.shape[1] < 2:
        return lg.argmax(1), torch.ones(lg.shape[0], dtype=torch.bool)
    top = lg.topk(2, dim=1).values
    return lg.argmax(1), (top[:, 0] - top[:, 1]) > 2 * TOL_FACTOR * asr_floors(name, frames)["logits"]
