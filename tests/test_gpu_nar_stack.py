"""GPU: the NAR stages through run_stack (vall-e_amd/csrc/engine.hip) against the fp64 reference of tests/nar_stack_ref.py, on
every dispatch of the row path's split-K construction.

Each case builds a synthetic bf16 engine (two layers, num_quantizers = 3: two stages, so the AdaLN stage index and the chaining
of the stage embeddings are both exercised; prefix_mode 1 with P > 0), runs vx_nar_ex teacher-forced with stage_logits, and
asserts through vx_op_rows_plan with the device's CU count the slice plan (out-projection, FFN2) the case exists for:

  d / H      M = S2 + P + T   plan    why
  1024 / 16  1000             4 / 4   ragged eighth row tile
  1024 / 16  1153             2 / 2   the benchmark's 1025-row regime
  1024 / 16  2100             1 / 1   no slabs: the residual is added in the GEMM epilogue, nothing to fold
  1024 / 16  70               4 / 4   one row tile; QKV / FFN1 on the wave-tile kernel
  128 / 2    300              2 / 4   out-projection slices of 64 k (one ring stage), FFN2 slices of 128
  256 / 4    129              4 / 4   slices of 64 / 256, one row in the second tile
  512 / 8    257              4 / 4   a third width
  512 / 8    257, post-norm   4 / 4   fold with xout, closing norm, no final norm

The test's own state dict is scaled so that the wrong answers separate: the out-projection and FFN2 biases (N(0, 0.02) and
U(+-0.03)) by BIAS_SCALE, to order 1 like the biases of the op-level tests (at their own size a missing bias moves the logits by
less than the bf16 activations do); the q rows of every in_proj by Q_SHARPEN as in test_gpu_ar_step.py (a near-uniform softmax
averages the values away, and with them every K slice of the out-projection and the prompt's codebooks); the out-projection
weights by W_OUT_SCALE; nar_audio_position.alpha is POS_ALPHA.

Per case and stage:
  stage logits, every generated row, within C_LOGIT units of 2^-8 (|h_f| |W_head|^T), h_f the reference's final-norm row (the
      convention of test_gpu_ar_step.py; the constant covers the bf16 activations of the two layers in front);
  nar_x of the last stage (the residual stream the stack leaves, fold-only pass included) within C_X units of 2^-8 x the
      per-element sum over the layers of |att| |W_out|^T + |b_out| + |ff| |W_2|^T + |b_2|;
  every wrong answer of nar_stack_ref.WRONG at least SEP bounds from the engine's logits, in every stage ('drop_out_slice_l1'
      drops one of the plan's out-projection slices; four slices where the plan has none);
  the same call twice gives bitwise equal logits.

Worst errors measured on the MI355X (units as above) and the bounds at about 4x:
  width d   logits (worst case)            nar_x    -> C_LOGIT  C_X     nearest wrong answer (bounds)
  128       0.384                          0.308       1.55     1.25    15.5 (pos_shift)
  256       0.273                          0.181       1.1      0.75    11.0 (no_prompt_cb)
  512       0.290 (post-norm; pre 0.208)   0.187       1.2      0.75    6.56 (post-norm, no_out_bias_l0; pre-norm 7.42)
  1024      0.134 (M = 1153)               0.100       0.55     0.4     10.8 (M = 1000, no_prompt_cb)
The bounds are per width: both units sum |w| |h| over d terms while the rounding errors add like sqrt(d), so the measured
figures fall with d, and so do the distances of the wrong answers in the same units.  One bound for all widths (1.55, set by
d = 128) would leave the d = 1024 cases 3.8 bounds from 'no_prompt_cb' and the post-norm case 5.1 from 'no_out_bias_l0'."""
import pytest
import torch

from nar_stack_ref import WRONG, NarRef

pytestmark = pytest.mark.gpu

C_LOGIT = {128: 1.55, 256: 1.1, 512: 1.2, 1024: 0.55}  # per width d
C_X = {128: 1.25, 256: 0.75, 512: 0.75, 1024: 0.4}
SEP = 4.0
BIAS_SCALE = 60.0
Q_SHARPEN = 4.0
W_OUT_SCALE = 3.0
POS_ALPHA = 3.0
U16 = 2.0 ** -8
L, Q = 2, 3

CASES = {
    "d1024_m1000": dict(d=1024, H=16, M=1000, plan=(4, 4)),
    "d1024_m1153": dict(d=1024, H=16, M=1153, plan=(2, 2)),
    "d1024_m2100": dict(d=1024, H=16, M=2100, plan=(1, 1)),
    "d1024_m70": dict(d=1024, H=16, M=70, plan=(4, 4)),
    "d128_m300": dict(d=128, H=2, M=300, plan=(2, 4)),
    "d256_m129": dict(d=256, H=4, M=129, plan=(4, 4)),
    "d512_m257": dict(d=512, H=8, M=257, plan=(4, 4)),
    "d512_m257_postnorm": dict(d=512, H=8, M=257, plan=(4, 4), norm_first=False),
}


def case_inputs(c, seed):
    """(cfg, state dict, text (S2,), codes (P + T, Q), P): a third of the rows prompt, so that the prompt's own codebooks weigh
    in the attention of the generated rows"""
    from valle_amd.config import ModelConfig
    from valle_amd.weights import synthetic_state_dict

    cfg = ModelConfig(decoder_dim=c["d"], nhead=c["H"], num_decoder_layers=L, prefix_mode=1, num_quantizers=Q,
                      norm_first=c.get("norm_first", True))
    sd = synthetic_state_dict(cfg, seed)
    for li in range(L):
        sd[f"nar_decoder.layers.{li}.self_attn.in_proj_weight"][:c["d"]] *= Q_SHARPEN
        sd[f"nar_decoder.layers.{li}.self_attn.out_proj.weight"] *= W_OUT_SCALE
        sd[f"nar_decoder.layers.{li}.self_attn.out_proj.bias"] *= BIAS_SCALE
        sd[f"nar_decoder.layers.{li}.linear2.bias"] *= BIAS_SCALE
    sd["nar_audio_position.alpha"].fill_(POS_ALPHA)
    M = c["M"]
    S2 = min(24, M // 5)
    P = M // 3
    g = torch.Generator().manual_seed(seed)
    text = torch.randint(3, 100, (S2,), generator=g)
    codes = torch.randint(0, 1024, (M - S2, Q), generator=g)
    return cfg, sd, text, codes, P


def _units(err, scale):
    return float((err / scale).max())


def test_cases_cover_every_plan():
    """a condition on the table: together the cases run 4 / 4, 2 / 2, 1 / 1 and 2 / 4 slices (each case asserts its own below)"""
    assert {c["plan"] for c in CASES.values()} >= {(4, 4), (2, 2), (1, 1), (2, 4)}


@pytest.mark.parametrize("name", list(CASES))
def test_nar_stages_match_fp64_layer_by_layer(name):
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.engine import Engine, op_rows_plan

    c = CASES[name]
    d, M = c["d"], c["M"]
    plan = op_rows_plan(M, d)
    assert plan == (1,) + c["plan"], f"{name}: the stack plans {plan} here, the case exists for {c['plan']}"
    cfg, sd, text, codes, P = case_inputs(c, seed=23)
    S2, T = text.shape[0], codes.shape[0] - P
    e = Engine(cfg, "bf16", max_text=32, max_audio=M)
    try:
        e.load_state_dict(sd)
        args = (text, codes[:P].contiguous(), codes[P:, 0].contiguous())
        _, lg = e.nar(*args, forced_codes=codes[P:].contiguous(), stage_logits=True)
        nar_x = e.read("nar_x", (M, d))
        _, lg2 = e.nar(*args, forced_codes=codes[P:].contiguous(), stage_logits=True)
    finally:
        e.close()
    assert lg.shape == (Q - 1, T, 1024)
    assert torch.equal(lg.view(torch.int32), lg2.view(torch.int32)), f"{name}: two calls differ"

    ref = NarRef(cfg, sd, "cuda", pe_rows=max(4000, 32 + M))
    text_d, codes_d = text.cuda(), codes.cuda()
    slices = c["plan"][0] if c["plan"][0] > 1 else 4
    fails, worst_lg, seps = [], 0.0, {w: float("inf") for w in WRONG}
    for stage in range(Q - 1):
        r = ref.forward(text_d, codes_d, P, stage)
        got = lg[stage].cuda().double()
        assert torch.isfinite(got).all(), name
        units = _units((got - r["logits"]).abs(), U16 * r["head_abs"])
        worst_lg = max(worst_lg, units)
        if units > C_LOGIT[d]:
            fails.append(f"stage {stage} logits: {units:.4g} units")
        tol = C_LOGIT[d] * U16 * r["head_abs"]
        for w in WRONG:
            sep = _units((ref.forward(text_d, codes_d, P, stage, w, slices)["logits"] - got).abs(), tol)
            seps[w] = min(seps[w], sep)
            if sep < SEP:
                fails.append(f"stage {stage} wrong answer {w}: {sep:.3g} bounds")
    gx = nar_x.cuda().double()
    assert torch.isfinite(gx).all(), name
    units_x = _units((gx - r["x"]).abs(), U16 * r["x_abs"])  # r: the last stage
    if units_x > C_X[d]:
        fails.append(f"nar_x: {units_x:.4g} units")
    print(f"\n{name}: plan {plan[1]} / {plan[2]}, logits {worst_lg:.3g} units (bound {C_LOGIT[d]}), nar_x {units_x:.3g} (bound {C_X[d]}); "
          "nearest wrong answers (bounds) " + ", ".join(f"{w} {s:.3g}" for w, s in seps.items()))
    assert not fails, f"{name}: " + "; ".join(fails)
