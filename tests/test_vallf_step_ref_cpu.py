"""CPU: the conditions under which tests/test_gpu_vallf_step.py means something, checked on the fp64 reference alone.

  (1) StepRefF is the oracle: teacher-forced from its own fp64 cache and memory, with no bf16 rounding, it reproduces the traced AR
      logits of valle_oracle.inference_f (the no-cache restatement of VALLF.inference) to 1e-9, pre-norm, post-norm and with the
      prenets.
  (2) Every wrong answer of ar_step_ref.wrong_f is at least SEP + 1 bounds (C_LOGIT units of 2^-24 sum |w| |h| of the head) from
      the right answer at every pass of every utterance of every GPU case, with the GPU test's weights, texts, prompts and forced
      tokens.  A correct engine lies within one bound of the reference, so it keeps SEP bounds from every wrong answer.  The cache
      and the memory are the reference's own, rounded to bf16 where the engine stores bf16, and the memory keeps the rows of the
      earlier, longer texts as the engine's does.  f_bf16_d1024 runs here at d 256 with 4 heads (head_dim 64 as on the GPU) under
      the same S and M schedule: fp64 at d 1024 takes too long for a CPU test; every other case runs at its own size.
  (3) is_matrix_key / engine_state_dict / bf16_miss on the keys and rows VALL-F adds."""
import pytest
import torch

from ar_step_ref import (U32, VALLF_CASES, VALLF_L, VALLF_MAX_AUDIO, VALLF_MAX_TEXT, VALLF_SEED, VALLF_TEXT_LENS, WRONG_F, StepRefF,
                         bf16_bracket, bf16_miss, engine_state_dict, is_matrix_key, mem_rows, mem_split_ranges, vallf_inputs, wrong_f)
from oracle import valle_oracle as vo
from test_gpu_ar_step import C_LOGIT, Q_SHARPEN, SEP

L = VALLF_L


def _own_state(ref, text, yy, mem, store):
    """The reference's own prefill: the cache (L, 2, H, rows, hd) with rows 0..A-1 filled, `mem` rows 0..S-1 overwritten in place
    (rows past S keep what was there), and pass 0's logits."""
    A, S = yy.shape[0], text.shape[0]
    kv = torch.zeros(L, 2, ref.H, VALLF_MAX_AUDIO, ref.hd, dtype=torch.float64)
    res, lg0, _ = ref.prefill_kv(text, yy)
    for li, (k, v, _, _) in enumerate(res):
        kv[li, 0, :, :A], kv[li, 1, :, :A] = store(k), store(v)
    for li, (k, v, _, _) in enumerate(ref.memory_kv(text)):
        mem[li, 0, :, :S], mem[li, 1, :, :S] = store(k), store(v)
    return kv, lg0


@pytest.mark.parametrize("name,extra", [("f_fp32_hd4", {}), ("f_bf16_hd16", {}), ("f_fp32_hd4", dict(norm_first=False)),
                                        ("f_fp32_hd4", dict(add_prenet=True))])
def test_step_ref_f_is_the_oracle(name, extra):
    c = dict(VALLF_CASES[name], **extra)
    d, H = c["d"], c["H"]
    sd, utts = vallf_inputs(c, VALLF_SEED, Q_SHARPEN)
    ref = StepRefF(sd, d, H, L, c.get("norm_first", True), c.get("add_prenet", False), 1, True, bf16=False)
    mem = torch.zeros(L, 2, H, VALLF_MAX_TEXT, ref.hd, dtype=torch.float64)
    for text, prompt, forced in (utts[4], utts[3][:1] + utts[0][1:]):  # S 8 with 129 prompt rows; S 65 with the bos row alone
        S = text.shape[0]
        trace = {}
        vo.inference_f(ref.oracle, text[None], torch.tensor([S]), prompt[None, :, None], top_k=1, trace=trace, forced=forced)
        want = torch.stack(trace["ar_logits"])
        assert want.dtype == torch.float64 and want.shape == (forced.shape[0] + 1, 1025)
        yy = torch.cat([torch.tensor([1025]), prompt])
        A = yy.shape[0]
        kv, lg0 = _own_state(ref, text, yy, mem, lambda x: x)
        got = [lg0]
        for p in range(1, forced.shape[0] + 1):
            t = A - 1 + p
            got.append(ref.forward(int(forced[p - 1]), t, kv, mem, t, S, own_newest=True)["logits"])
        err = float((torch.stack(got) - want).abs().max())
        assert err <= 1e-9, f"{name} {extra} S={S} A={A}: {err:.3g}"


# fp64 at d 1024 is too slow here: the same schedule at d 256, 4 heads of 64 as on the GPU
STAND_IN = {"f_bf16_d1024": dict(precision="bf16", d=256, H=4)}


@pytest.mark.parametrize("name", list(VALLF_CASES))
def test_wrong_answers_are_far_from_the_right_one(name):
    c = STAND_IN.get(name, VALLF_CASES[name])
    d, H, bf16 = c["d"], c["H"], c["precision"] == "bf16"
    sd, utts = vallf_inputs(c, VALLF_SEED, Q_SHARPEN)
    ref = StepRefF(sd, d, H, L, c.get("norm_first", True), c.get("add_prenet", False), 1, True, bf16)
    store = (lambda x: x.to(torch.bfloat16).double()) if bf16 else (lambda x: x)
    mem = torch.zeros(L, 2, H, VALLF_MAX_TEXT, ref.hd, dtype=torch.float64)
    nearest = {w: (float("inf"), None) for w in WRONG_F}
    for ui, (text, prompt, forced) in enumerate(utts):
        S = text.shape[0]
        assert S == VALLF_TEXT_LENS[ui]
        yy = torch.cat([torch.tensor([1025]), prompt])
        A = yy.shape[0]
        kv, _ = _own_state(ref, text, yy, mem, store)
        wrong = wrong_f(S, ui == 0)
        for p in range(1, forced.shape[0] + 1):
            t = A - 1 + p
            tok = int(forced[p - 1])
            r = ref.forward(tok, t, kv, mem, t, S, own_newest=True)
            tol = C_LOGIT * U32 * r["head_abs"]
            ok = tol > 0  # (the zeroed EOS row of the head)
            for w, lg in ref.forward(tok, t, kv, mem, t, S, wrong).items():
                sep = float(((lg - r["logits"]).abs()[ok] / tol[ok]).max())
                if sep < nearest[w][0]:
                    nearest[w] = (sep, (S, A, p))
            kv[:, :, :, t] = store(kv[:, :, :, t])
    print(f"\n{name}: nearest wrong answers " + ", ".join(f"{w} {s:.3g}@{at}" for w, (s, at) in nearest.items()))
    bad = {w: v for w, v in nearest.items() if v[0] < SEP + 1}
    assert not bad, f"{name}: wrong answers within {SEP + 1} bounds of the right one (S, rows, pass): {bad}"


def test_wrong_answer_schedule():
    assert mem_split_ranges(129) == [(0, 17), (17, 34), (34, 51), (51, 68), (68, 85), (85, 102), (102, 119), (119, 129)]
    assert mem_split_ranges(5) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]  # three empty splits
    assert mem_split_ranges(8) == [(j, j + 1) for j in range(8)] and len(mem_split_ranges(9)) == 5
    assert mem_rows(5, "mem_drop_split") == [0, 1, 3, 4] and mem_rows(9, "mem_drop_split") == [0, 1, 2, 3, 6, 7, 8]
    assert mem_rows(3, "mem_one_more") == [0, 1, 2, 3] and mem_rows(3, "mem_last_twice") == [0, 1, 2, 2]
    assert mem_rows(3, "mem_drop_first") == [1, 2] and mem_rows(3, "mem_drop_last") == [0, 1]
    assert wrong_f(129, True) == [w for w in WRONG_F if w != "mem_one_more"] and wrong_f(5, False) == list(WRONG_F)
    # one key: nothing may be dropped, and the key twice is the right answer itself
    assert [w for w in wrong_f(1, False) if w.startswith("mem_")] == ["mem_one_more", "mem_other_layer"]
    for S in VALLF_TEXT_LENS:
        for w in wrong_f(S, False):
            if w.startswith("mem_"):
                rows = mem_rows(S, w)
                assert rows and max(rows) < VALLF_MAX_TEXT and (rows != list(range(S)) or w == "mem_other_layer")
    assert max(VALLF_TEXT_LENS) == VALLF_TEXT_LENS[0]  # every later text is shorter: row S holds an earlier text's key


def test_rounding_rule_on_the_cross_attention_keys():
    p = "ar_decoder.layers.1."
    low = [p + "multihead_attn.in_proj_weight", p + "multihead_attn.out_proj.weight", p + "self_attn.in_proj_weight",
           p + "linear2.weight", "ar_predict_layer.weight"]
    full = [p + "multihead_attn.in_proj_bias", p + "multihead_attn.out_proj.bias", p + "norm3.weight", p + "norm3.bias",
            "ar_text_prenet.14.weight", "ar_text_prenet.1.weight", "ar_audio_prenet.0.weight", "ar_text_position.alpha",
            "ar_text_embedding.word_embeddings.weight", "nar_decoder.layers.0.norm3.project_layer.weight"]
    assert all(is_matrix_key(k) for k in low) and not any(is_matrix_key(k) for k in full)
    c = dict(VALLF_CASES["f_fp32_hd4"], add_prenet=True)
    sd, utts = vallf_inputs(c, VALLF_SEED, Q_SHARPEN)
    assert p + "multihead_attn.in_proj_weight" in sd and p + "norm3.bias" in sd and "ar_text_prenet.14.weight" in sd
    rounded, exact = engine_state_dict(sd, True), engine_state_dict(sd, False)
    for k, v in sd.items():
        if not torch.is_floating_point(v):
            continue
        assert torch.equal(exact[k], v.double())
        want = v.to(torch.bfloat16).double() if is_matrix_key(k) else v.double()
        assert torch.equal(rounded[k], want), k
    assert not torch.equal(rounded[p + "multihead_attn.in_proj_weight"], exact[p + "multihead_attn.in_proj_weight"])
    # bf16_miss on a memory row: 0 for the rounding of the fp64 value, for the other neighbour the distance from the midpoint
    ref = StepRefF(sd, c["d"], c["H"], L, True, True, 1, True, bf16=True)
    k = ref.memory_kv(utts[1][0])[1][0].reshape(-1)
    got = k.to(torch.bfloat16).double()
    assert float(bf16_miss(got, k).max()) == 0.0
    lo, hi = bf16_bracket(k)
    other = torch.where(got.abs() == lo, hi, lo) * torch.sign(k)
    mid = (lo + hi) / 2
    assert torch.allclose(bf16_miss(other, k), (k.abs() - mid).abs(), rtol=0, atol=1e-18)
    assert float(bf16_miss(other, k).min()) >= 0.0 and float(bf16_miss(other, k).max()) <= float(((hi - lo) / 2).max())
