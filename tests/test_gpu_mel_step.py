"""GPU: the mel-spectrogram Transformer's decode step and encoder, pass by pass against the fp64 references of tests/mel_step_ref.py
(MelStepRef: ar_step_ref.StepRefF's decoder layers between this model's input row and head; meltf_ref.MelRef's encoder).

Each case (mel_step_cases.MEL_CASES, L = 2, synthetic weights, the q rows of every attention scaled by Q_SHARPEN) builds ONE engine
and runs texts of 129, 5, 64, 65 and 1 ids on it back to back, so that the memory holds stale rows behind every shorter text.
Each text is teacher-forced for 12 frames through the cached step (decode_forced) and once through the row pass (teacher_forced).
After every decode the test reads the frames, the stop logits, the cache ("ar_kv") and the memory ("ar_mem").  The step reference
reads the engine's own cache rows and memory rows, so every pass stands alone:

  (a) memory rows 0..S-1 of every decoder layer against the fp64 encoder (embedding or encoder prenet, L encoder layers, final
      norm, the layer's cross in_proj), within C_MEM units of u (sum |w| |h| + |b|) of the cross in_proj, u = 2^-8 on bf16 engines
      and 2^-24 on fp32 ones.  The rows stand behind an L-layer encoder, not behind an embedding as the VALL-F memory does, so the
      constant is this test's own: 4 x the worst measured (table below);
  (b) every decode pass: frame and stop logit within C_LOGIT units of 2^-24 (sum |w| |h| + |b|) of the head, the newest cache row
      of every layer within C_KV (bf16: ar_step_ref.bf16_miss), as tests/test_gpu_vallf_step.py;
  (c) the row pass's predict / stop_logits against the cached step's, per row, within C_PREFILL units of u x the head's sum: the
      budget test_gpu_vallf_step.py gives the row path's last row against the step's head;
  (d) every wrong answer of ar_step_ref.wrong_f (mel_step_ref.wrong_step) at least SEP bounds from the engine's frame and stop
      logit, and every wrong answer of the encoder (mel_step_ref.wrong_enc: the last text row unseen by the encoder's
      self-attention, a causal mask, encoder.norm dropped, the norm sites of three-per-layer arithmetic) at least SEP bounds from
      the engine's memory rows.  tests/test_mel_step_cpu.py shows the references' own right answers SEP + 1 bounds from each;
  (e) the first text again gives bitwise the frames, stop logits and memory rows it gave the first time;
  (f) the captured step has the VALL-F step's 8 launches per layer plus the opening launch (step_kernels).

C_LOGIT, C_KV, C_PREFILL, SEP and Q_SHARPEN are tests/test_gpu_ar_step.py's, unchanged.  Worst values measured on the MI355X
(profiles/mel_step_parity.json, written where VX_MEL_STEP_PARITY_OUT names a file), and the nearest wrong answer of the step
(bounds of C_LOGIT) and of the encoder (bounds of C_MEM):
  case               memory  C_MEM  frame / stop  newest  row pass  nearest step wrong answer   nearest encoder wrong answer
  m_bf16_d1024       0.211   1.57   0.551         0.239   0.0828    1.66e+03 (mem_last_twice)   6.6 (enc_norm_sites_3)
  m_fp32_d192        5.11    20.4   1.07          1.19    3.71      3.4e+03  (mem_drop_first)   1.3e+04 (enc_last_unseen)
  m_bf16_d256_hd64   0.392   1.57   0.965         0.235   0.191     927      (mem_one_more)     10 (enc_norm_sites_3)
  m_fp32_hd4_prenet  4.78    20.4   2.09          1.68    4.28      9.73e+03 (mem_last_twice)   1.2e+04 (enc_last_unseen)
  m_bf16_postnorm    0.291   1.57   0.895         0.33    0.118     1.55e+03 (mem_last_twice)   6.8 (enc_last_unseen)
On bf16 engines the encoder's wrong answers are near: a memory row's unit, 2^-8 sum |w| |h|, is about a tenth of the row itself, so
a row from entirely different inputs is 20 - 50 units away (mel_step_ref.wrong_enc says what follows for one key of many)."""
import pytest
import torch

import mel_step_cases as MC
import mel_step_ref as R
from ar_step_ref import U16, U32, bf16_miss
from test_gpu_ar_step import C_KV, C_LOGIT, C_PREFILL, Q_SHARPEN, SEP

pytestmark = pytest.mark.gpu

L = MC.MEL_L
# (a): 4 x the worst measured over the five cases: bf16 0.392 units of 2^-8 (m_bf16_d256_hd64), fp32 5.11 units of 2^-24
# (m_fp32_d192).  Two encoder layers stand in front of these rows where the VALL-F memory (C_PREFILL: 1.25 / 12) has an embedding.
C_MEM = {"bf16": 1.57, "fp32": 20.4}


def step_kernels(num_layers: int) -> int:
    """Kernels per pass of the captured mel step: the VALL-F step's 8 launches per layer plus the opening launch.  The VALL-F
    step's own count is 8 L + 2, its other two being the sampler and the head; the mel step has neither - the opening kernel stands
    where the sampler does and computes the 101 head rows of the pass before."""
    return 8 * num_layers + 1


def _run(e, text, forced):
    e.encode(text)
    e.decode_forced(forced)
    frames, reason, stops = e.result()
    assert frames.shape == (MC.MEL_PASSES, R.MEL_BINS) and stops.shape == (MC.MEL_PASSES,) and reason == "max_frames"
    return torch.cat([frames.double(), stops.double()[:, None]], 1), e.read_kv().double(), e.read_mem()


@pytest.mark.parametrize("name", list(MC.MEL_CASES))
def test_mel_step_matches_fp64_pass_by_pass(name):
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.engine import MelEngine, VxError

    c = MC.MEL_CASES[name]
    d, H, precision = c["d"], c["H"], c["precision"]
    bf16 = precision == "bf16"
    u = U16 if bf16 else U32
    cfg = MC.mel_config(c)
    sd, utts = MC.mel_inputs(c, Q_SHARPEN)
    ref = MC.mel_ref(c, sd)
    fails = []
    worst = dict(mem=0.0, logits=0.0, newest=0.0, rows=0.0)
    seps = {}

    def note(key, units, bound, what):
        worst[key] = max(worst[key], units)
        if not units <= bound:
            fails.append(f"{what}: {units:.4g} units (bound {bound})")

    def far(w, sep, at, what):
        if sep < seps.get(w, (float("inf"), None))[0]:
            seps[w] = (sep, at)
        if not sep >= SEP:
            fails.append(f"{what} wrong answer {w}: {sep:.3g} bounds")

    e = MelEngine(cfg, precision, max_text=MC.MEL_MAX_TEXT, max_frames=MC.MEL_MAX_FRAMES)
    try:
        e.load_state_dict(sd)
        runs, rowp = [], []
        for text, forced in utts:
            runs.append(_run(e, text, forced))
            p, s = e.teacher_forced(text, forced)
            rowp.append(torch.cat([p.double(), s.double()[:, None]], 1))
        kernels = int(e.timings()["kernels_per_step"])
        again = _run(e, *utts[0])
        raw = again[2]
        xh = e.read("xh", (d,))
        with pytest.raises(VxError, match="out of range"):
            e.read("xh", (1,), offset_bytes=d * 4)
        with pytest.raises(VxError, match="unknown buffer"):
            e.read("ar_logits", (1,))
    finally:
        e.close()
    assert kernels == step_kernels(L), f"{name}: {kernels} kernels per pass, the mel step has {step_kernels(L)}"
    assert raw.shape == (L, 2, H, MC.MEL_MAX_TEXT, d // H) and raw.dtype == (torch.bfloat16 if bf16 else torch.float32)
    assert bool(torch.isfinite(xh).all())

    for ui, ((text, forced), (got, kv, mem)) in enumerate(zip(utts, runs)):
        mem = mem.double()
        S = text.shape[0]
        at = f"text {ui} (S={S})"
        # (a) the memory, and the encoder's wrong answers on it
        right = ref.memory_kv(text)
        for li, (k, v, ka, va) in enumerate(right):
            for which, r, ab in ((0, k, ka), (1, v, va)):
                note("mem", R.units((mem[li, which, :, :S] - r).abs(), u * ab), C_MEM[precision], f"{at} memory layer {li} {'KV'[which]}")
        for w in R.wrong_enc(S, ref.norm_first, bf16):
            sep = 0.0
            for li, ((_, _, ka, va), (wk, wv, _, _)) in enumerate(zip(right, ref.memory_kv(text, w))):
                sep = max(sep, R.units((wk - mem[li, 0, :, :S]).abs(), C_MEM[precision] * u * ka),
                          R.units((wv - mem[li, 1, :, :S]).abs(), C_MEM[precision] * u * va))
            far(w, sep, ui, at)
        # (b), (c), (d) the decode passes
        for p in range(MC.MEL_PASSES):
            frame = forced[p - 1] if p else torch.zeros(R.MEL_BINS)
            r = ref.step(frame, p, kv, mem, S)
            note("logits", R.units((got[p] - r["logits"]).abs(), U32 * r["head_abs"]), C_LOGIT, f"{at} pass {p} frame / stop")
            for li in range(L):
                for which, key in ((0, "k"), (1, "v")):
                    g, rr = kv[li, which, :, p], r[key][li]
                    miss = bf16_miss(g, rr) if bf16 else (g - rr).abs()
                    note("newest", R.units(miss, U32 * r[key + "_abs"][li]), C_KV, f"{at} pass {p} layer {li} newest {'KV'[which]}")
            note("rows", R.units((rowp[ui][p] - got[p]).abs(), u * r["head_abs"]), C_PREFILL[precision], f"{at} row {p} row pass against step")
            tol = C_LOGIT * U32 * r["head_abs"]
            for w, lg in ref.step(frame, p, kv, mem, S, R.wrong_step(S, ui == 0, p)).items():
                far(w, R.units((lg - got[p]).abs(), tol), (ui, p), f"{at} pass {p}")
    # (e) the first text again
    S0 = utts[0][0].shape[0]
    if not torch.equal(again[0], runs[0][0]):
        fails.append(f"the first text run again: frames / stop logits differ by {float((again[0] - runs[0][0]).abs().max()):.3g}")
    if not torch.equal(again[2][:, :, :, :S0].float(), runs[0][2][:, :, :, :S0].float()):
        fails.append("the first text run again: memory rows differ")
    print(f"\n{name}: memory {worst['mem']:.3g} units (bound {C_MEM[precision]}); frame / stop {worst['logits']:.3g} (bound {C_LOGIT}), "
          f"newest rows {worst['newest']:.3g} (bound {C_KV}), row pass against step {worst['rows']:.3g} (bound {C_PREFILL[precision]}); "
          "nearest wrong answers " + ", ".join(f"{w} {s:.3g}@{a}" for w, (s, a) in seps.items()))
    MC.parity_note(f"mel_step/{name}", dict(worst, nearest_wrong={w: s for w, (s, a) in seps.items()}))
    assert not fails, f"{name}: {len(fails)} failures: " + "; ".join(fails[:40])
