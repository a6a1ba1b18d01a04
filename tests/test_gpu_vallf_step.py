"""GPU: the VALL-F batch-1 decode step (enqueue_ar_step with e->vallf, 8 launches per layer) and the row path under it, pass by pass
against the fp64 reference of tests/ar_step_ref.py (StepRefF).

Each case builds ONE engine with synthetic weights (the q rows of every self-attention and cross-attention in_proj scaled by
Q_SHARPEN, so that both softmaxes are peaked) and runs nine utterances on it back to back, texts of 129, 5, 64, 65, 8, 9, 1, 47 and
63 keys (every shorter text after a longer one, so the memory holds stale rows; empty splits; the 8-split and 64-key tile edges)
over bos + P = 1, 63, 64, 65, 130 prompt rows (ragged and full 64-query tiles of cross_attn_rows_kernel), each teacher-forced for
12 passes.  After every utterance it reads the traced logits, the KV cache ("ar_kv") and the text memory ("ar_mem").  The reference
reads the engine's own cache rows and memory rows, so every checked pass stands on its own:

  (a) the memory rows 0..S-1 of every layer (memory_kv + kv_scatter_kernel at the max_text stride) within C_PREFILL units of
      u (sum |w| |h| + |b|) of the fp64 K / V of the embedded text, u = 2^-8 on bf16 engines, 2^-24 on fp32 ones: a row GEMM of
      the form of the prefill rows;
  (b) the prefill cache rows of every layer, and pass 0's logits (the last prefill row through the final norm and the head, which
      is what probes the last layer's row-path cross-attention), against an fp64 forward of the prompt over the fp64 memory, in
      the same units and bound: the logits row is the same kind of product of the row path's output as the next layer's K / V
      row, its budget u sum |w| |h| of the head;
  (c) every decode pass: logits within C_LOGIT units of 2^-24 sum |w| |h| of the head, the newest cache row of every layer within
      C_KV (bf16: ar_step_ref.bf16_miss), as tests/test_gpu_ar_step.py;
  (d) every wrong answer of ar_step_ref.wrong_f at least SEP bounds from the engine's logits: the self-attention ones of the VALL-E
      test, and on the memory a key dropped at either end, the last key twice, the middle non-empty split dropped, row S included
      (a stale key of an earlier text), the other layer's memory.  tests/test_vallf_step_ref_cpu.py shows that the reference's
      own right answer is SEP + 1 bounds from each;
  (e) after the nine utterances the first one again gives bitwise the logits and the memory rows it gave the first time.

The step's shape is asserted from the kernels per pass of the captured graph: 8 L + 2, + 3 with the audio prenet.

Worst values measured on the MI355X (units as above; bounds: memory / prefill / pass 0 C_PREFILL = 1.25 bf16, 12 fp32; logits
C_LOGIT = 3.5; newest rows C_KV = 2.5), and the nearest wrong answer of the case in bounds:
  case             memory  prefill  pass 0  logits  newest  nearest wrong answer
  f_bf16_d1024     0.164   0.199    0.0986  0.535   0.208   1.11e+03 (newest_twice)
  f_fp32_d512      5.61    5.15     1.78    0.779   0.939   844      (drop_oldest)
  f_bf16_hd32      0.319   0.405    0.169   1.25    0.224   1.51e+03 (mem_drop_last, mem_last_twice)
  f_bf16_hd16      0.319   0.392    0.164   1.10    0.244   1.73e+03 (mem_last_twice)
  f_fp32_hd8       4.17    4.87     2.06    1.48    1.32    2.63e+03 (drop_oldest)
  f_fp32_hd4       4.25    4.79     2.32    2.31    1.73    4.84e+03 (drop_oldest)
  f_bf16_postnorm  0.250   0.295    0.156   0.916   0.223   958      (newest_twice)
  f_bf16_prenet    0.239   0.297    0.118   0.781   0.334   2.11e+03 (stale_newest)
The nearest wrong answers on the memory: mem_drop_first 1.8e+03, mem_drop_last 1.51e+03, mem_last_twice 1.51e+03, mem_drop_split
1.57e+04, mem_one_more 2.15e+03, mem_other_layer 2.79e+05.  Every constant is tests/test_gpu_ar_step.py's, unchanged."""
import pytest
import torch

from ar_step_ref import (U16, U32, VALLF_CASES, VALLF_L, VALLF_MAX_AUDIO, VALLF_MAX_TEXT, VALLF_PASSES, VALLF_SEED, WRONG_F, StepRefF,
                         bf16_miss, vallf_config, vallf_inputs, wrong_f)
from test_gpu_ar_step import C_KV, C_LOGIT, C_PREFILL, Q_SHARPEN, SEP, _units

pytestmark = pytest.mark.gpu

L = VALLF_L


def _run(e, text, prompt, forced):
    """One utterance on the engine: (traced logits (n + 1, 1025), cache, memory), each float64 copies of what the engine holds."""
    e.ar_prefill(text, prompt)
    e.ar_decode(top_k=1, forced=forced)
    toks, _, n_pass = e.ar_result()
    assert torch.equal(toks, forced) and n_pass == forced.shape[0] + 1
    return e.read("ar_logits", (n_pass, 1025)).double(), e.read_ar_kv().double(), e.read_ar_mem()


@pytest.mark.parametrize("name", list(VALLF_CASES))
def test_vallf_step_matches_fp64_pass_by_pass(name):
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.engine import Engine, VxError

    c = VALLF_CASES[name]
    d, H, precision = c["d"], c["H"], c["precision"]
    bf16 = precision == "bf16"
    u, c_pf = (U16 if bf16 else U32), C_PREFILL[precision]
    cfg = vallf_config(c)
    sd, utts = vallf_inputs(c, VALLF_SEED, Q_SHARPEN)
    ref = StepRefF(sd, d, H, L, cfg.norm_first, cfg.add_prenet, 1, True, bf16)
    fails = []
    worst = dict(mem=0.0, prefill=0.0, pass0=0.0, logits=0.0, newest=0.0)
    seps = {w: (float("inf"), None) for w in WRONG_F}

    def note(key, units, bound, what):
        worst[key] = max(worst[key], units)
        if not units <= bound:
            fails.append(f"{what}: {units:.4g} units (bound {bound})")

    e = Engine(cfg, precision, max_text=VALLF_MAX_TEXT, max_audio=VALLF_MAX_AUDIO, trace_logits=True)
    try:
        e.load_state_dict(sd)
        runs = [_run(e, *utt) for utt in utts]
        kernels = e.timings()["step_kernels"]
        first_again = _run(e, *utts[0])
        raw = first_again[2]
        with pytest.raises(VxError, match="out of range"):  # the tap ends where the memory ends
            e.read("ar_mem", (1,), raw.dtype, offset_bytes=raw.numel() * raw.element_size())
    finally:
        e.close()
    want = 8 * L + 2 + (3 if cfg.add_prenet else 0)
    assert kernels == want, f"{name}: {kernels} kernels per pass, the VALL-F step has {want}"
    assert raw.shape == (L, 2, H, VALLF_MAX_TEXT, d // H) and raw.dtype == (torch.bfloat16 if bf16 else torch.float32)

    for ui, ((text, prompt, forced), (logits, kv, mem)) in enumerate(zip(utts, runs)):
        mem = mem.double()
        S = text.shape[0]
        yy = torch.cat([torch.tensor([1025]), prompt])
        A = yy.shape[0]
        at = f"utterance {ui} (S={S}, {A} prompt rows)"
        # (a) the text memory
        for li, (k, v, ka, va) in enumerate(ref.memory_kv(text)):
            for which, r, ab in ((0, k, ka), (1, v, va)):
                note("mem", _units((mem[li, which, :, :S] - r).abs(), u * ab), c_pf, f"{at} memory layer {li} {'KV'[which]}")
        # (b) the prefill rows and pass 0
        rows, lg0, head0 = ref.prefill_kv(text, yy)
        for li, (k, v, ka, va) in enumerate(rows):
            for which, r, ab in ((0, k, ka), (1, v, va)):
                note("prefill", _units((kv[li, which, :, :A] - r).abs(), u * ab), c_pf, f"{at} prefill layer {li} {'KV'[which]}")
        note("pass0", _units((logits[0] - lg0).abs(), u * head0), c_pf, f"{at} pass 0 logits")
        # (c), (d) the decode passes
        wrong = wrong_f(S, ui == 0)
        for p in range(1, VALLF_PASSES + 1):
            t = A - 1 + p  # VALL-F: the cache holds audio rows only, row = audio position
            tok = int(forced[p - 1])
            r = ref.forward(tok, t, kv, mem, t, S)
            got = logits[p]
            note("logits", _units((got - r["logits"]).abs(), U32 * r["head_abs"]), C_LOGIT, f"{at} pass {p} logits")
            for li in range(L):
                for which, key in ((0, "k"), (1, "v")):
                    g, rr = kv[li, which, :, t], r[key][li]
                    miss = bf16_miss(g, rr) if bf16 else (g - rr).abs()
                    note("newest", _units(miss, U32 * r[key + "_abs"][li]), C_KV, f"{at} pass {p} layer {li} newest {'KV'[which]}")
            tol = C_LOGIT * U32 * r["head_abs"]
            for w, lg in ref.forward(tok, t, kv, mem, t, S, wrong).items():
                sep = _units((lg - got).abs(), tol)
                if sep < seps[w][0]:
                    seps[w] = (sep, (ui, p))
                if sep < SEP:
                    fails.append(f"{at} pass {p} wrong answer {w}: {sep:.3g} bounds")
    # (e) the first utterance again
    S0 = utts[0][0].shape[0]
    if not torch.equal(first_again[0], runs[0][0]):
        fails.append(f"the first utterance run again: logits differ by {float((first_again[0] - runs[0][0]).abs().max()):.3g}")
    if not torch.equal(first_again[2][:, :, :, :S0].float(), runs[0][2][:, :, :, :S0].float()):
        fails.append("the first utterance run again: memory rows differ")
    print(f"\n{name}: memory {worst['mem']:.3g} units, prefill rows {worst['prefill']:.3g}, pass 0 logits {worst['pass0']:.3g} "
          f"(bound {c_pf}); logits {worst['logits']:.3g} (bound {C_LOGIT}), newest rows {worst['newest']:.3g} (bound {C_KV}); "
          "nearest wrong answers (utterance, pass) " + ", ".join(f"{w} {s:.3g}@{at}" for w, (s, at) in seps.items()))
    assert not fails, f"{name}: {len(fails)} failures: " + "; ".join(fails[:40])


def test_ar_mem_is_a_vallf_tap():
    """A VALL-E engine has no text memory: the name is refused, as vx_buffer_bytes refuses it for the configuration."""
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.config import ModelConfig
    from valle_amd.engine import Engine, VxError

    e = Engine(ModelConfig(decoder_dim=64, nhead=16, num_decoder_layers=1, num_quantizers=1), "fp32", max_text=8, max_audio=8)
    try:
        with pytest.raises(VxError, match="unknown buffer 'ar_mem'"):
            e.read("ar_mem", (1,))
    finally:
        e.close()
