"""No GPU: vets the references and the cases of tests/mel_step_ref.py / mel_step_cases.py before the GPU tests rely on them.

  * every wrong answer of the kernel-level tests (test_gpu_mel_open.py, test_gemm_simple_ragged) lies at least SEP + 1 bounds from
    the reference's own right answer on the chosen inputs, so that a kernel within one bound of the right answer is at least SEP
    bounds from every wrong one;
  * the chosen widths cross every edge of the opening kernel's slicing (per, the last slice's length, empty workgroups);
  * the exact-integer cases are exact in fp32;
  * the stop rule's restatement gives the table of the cases file, row by row;
  * the step reference (ar_step_ref.StepRefF's layers between this model's input row and head) on its own cache, over the encoder
    reference's memory, equals meltf_ref.MelRef.teacher_forced to 1e-9 on every case of test_gpu_mel_step.py, and every wrong
    answer of the step and of the encoder lies SEP + 1 bounds from the right one."""
import math

import pytest
import torch

import mel_step_cases as MC
import mel_step_ref as R

# test_gpu_ar_step.py's constants (the module imports nothing that needs a GPU)
from ar_step_ref import U16
from test_gpu_ar_step import C_LOGIT, Q_SHARPEN, SEP


@pytest.mark.parametrize("d", list(MC.OPEN_WIDTHS))
def test_open_widths_cross_the_launcher_edges(d):
    per, last, empty = MC.OPEN_WIDTHS[d]
    got_per, sl = R.open_slices(d)
    lens = [hi - lo for lo, hi in sl]
    nonempty = [n for n in lens if n]
    assert got_per == per == math.ceil(d / R.MEL_GRID) and per <= 64
    assert nonempty[-1] == last and lens.count(0) == empty
    assert sum(lens) == d and all(0 <= lo <= hi <= d for lo, hi in sl)
    assert d % 8 == 0 and d <= 1024


def test_open_widths_cover_each_kind_of_slicing():
    w = MC.OPEN_WIDTHS
    assert any(e > 0 for _, _, e in w.values())                     # workgroups that own nothing
    assert any(l < p and e == 0 for p, l, e in w.values())          # a ragged last slice
    assert any(p == 64 and l < 64 for p, l, e in w.values())        # full 64-row slices and a ragged one
    assert any(p == 64 and l == 64 for p, l, e in w.values())       # the full grid
    assert any(d % 256 and d > 256 for d in w)                      # a head chunk that ends inside a 256-channel group
    assert any(d < 256 and d % 4 == 0 for d in w)                   # threads past d in the norm


@pytest.mark.parametrize("mlp", MC.OPEN_PRENETS)
@pytest.mark.parametrize("d", list(MC.OPEN_WIDTHS))
def test_open_wrong_answers_are_separated_from_the_reference(d, mlp):
    inp = MC.open_inputs(d, mlp)
    head, hs = R.open_head(inp)
    for row in MC.OPEN_ROWS:
        frame = head[: R.MEL_BINS] if row >= 0 else torch.zeros(R.MEL_BINS, dtype=torch.float64)
        x, xs = R.open_x(inp, frame, row + 1)
        wrong = R.open_wrong(inp, row, frame)
        assert {"last_row_unwritten", "last_row_from_before", "pe_row"} <= set(wrong)
        assert (row < 0) or {"head_d_minus_4", "stop_from_row_99", "other_site_norm", "k0_minus_4"} <= set(wrong)
        for name, (kind, w) in wrong.items():
            right, scale = (head, hs) if kind == "head" else (x, xs)
            sep = R.units((w - right).abs(), C_LOGIT * R.U32 * scale)
            assert sep >= SEP + 1, (d, mlp, row, name, sep)


@pytest.mark.parametrize("mlp", MC.OPEN_PRENETS)
@pytest.mark.parametrize("d", list(MC.OPEN_WIDTHS))
def test_open_exact_prenet_is_exact_in_fp32(d, mlp):
    inp = MC.open_exact_inputs(d, mlp)
    for n in range(MC.OPEN_CAP):
        f = inp["forced"][n]
        y64, scale = R.open_prenet(inp, f)
        y32, _ = R.open_prenet(inp, f, dtype=torch.float32)
        assert float(scale.max()) < 2 ** 24 and torch.equal(y32.double(), y64) and torch.equal(y64, y64.round())
        if mlp:  # the hidden layers' worst partial sums
            h1 = inp["W1"].double().abs() @ f.double().abs() + inp["b1"].double().abs()
            h2 = inp["W2"].double().abs() @ h1 + inp["b2"].double().abs()
            assert float(h2.max()) < 2 ** 24
        # the position product rounds: the bitwise check can tell fadd(prenet, fmul(alpha, pe)) from a fused multiply-add
        x32 = R.open_x_exact32(inp, f, 3)
        fused = (y64 + inp["alpha"].double()[0] * inp["pe"].double()[3]).float()
        assert x32.dtype == torch.float32 and (d < 64 or not torch.equal(x32, fused))


def test_open_rule_table():
    assert set(MC.OPEN_RULE) == set(MC.OPEN_RULE_WANT)
    for name, (stop, st, max_frames, n_forced) in MC.OPEN_RULE.items():
        after, append, go = R.open_rule(st, stop, max_frames, n_forced)
        want = MC.OPEN_RULE_WANT[name]
        assert tuple(after[k] for k in ("row", "pass", "n_gen", "done", "stop_reason")) == want, name
        assert append == (want[2] == st["n_gen"] + 1) and go == (want[0] == st["row"] + 1), name
        assert st["row"] + 1 < MC.OPEN_PE_ROWS and st["n_gen"] < MC.OPEN_CAP  # the launch stays inside the test buffers
    assert R.open_rule(MC.OPEN_RULE["length_edge_below"][1], -1.0, 50, 0)[0]["row"] == 10 * 1  # row + 1 == 10 S: no length stop
    assert math.isnan(MC.OPEN_RULE["nan"][0]) and math.copysign(1.0, MC.OPEN_RULE["minus_zero"][0]) < 0
    assert torch.tensor(MC.OPEN_RULE["smallest_positive"][0], dtype=torch.float32).view(torch.int32).item() == 1


def _own_run(ref, text, forced, mem):
    """The step reference on its own cache: every pass's (101,) row and its head_abs, and the cache."""
    kv = torch.zeros(MC.MEL_L, 2, ref.H, MC.MEL_MAX_TEXT + MC.MEL_MAX_FRAMES + 2, ref.hd, dtype=torch.float64)
    rows, scales = [], []
    for p in range(forced.shape[0]):
        frame = forced[p - 1] if p else torch.zeros(R.MEL_BINS)
        r = ref.step(frame, p, kv, mem, text.shape[0], own_newest=True)
        rows.append(r["logits"])
        scales.append(r["head_abs"])
    return torch.stack(rows), torch.stack(scales), kv


@pytest.mark.parametrize("name", list(MC.MEL_CASES))
def test_step_reference_equals_melref_and_wrong_answers_are_separated(name):
    """The cached step reference over the encoder reference's memory equals MelRef.teacher_forced (every row recomputed under the
    causal mask) to 1e-9; every wrong answer of the step and of the encoder lies at least SEP + 1 bounds from the right one."""
    from test_gpu_mel_step import C_MEM

    c = MC.MEL_CASES[name]
    sd, utts = MC.mel_inputs(c, Q_SHARPEN)
    ref = MC.mel_ref(c, sd)
    u = (U16 if c["precision"] == "bf16" else R.U32) * C_MEM[c["precision"]]
    mem = torch.zeros(MC.MEL_L, 2, ref.H, MC.MEL_MAX_TEXT, ref.hd, dtype=torch.float64)  # as the engine's: longer texts leave rows
    for ui, (text, forced) in enumerate(utts):
        S = text.shape[0]
        right = ref.memory_kv(text)
        for li, (k, v, _, _) in enumerate(right):
            mem[li, 0, :, :S], mem[li, 1, :, :S] = k, v
        rows, scales, kv = _own_run(ref, text, forced, mem)
        predict, stop = ref.mel.teacher_forced(text, forced)
        assert float((rows[:, : R.MEL_BINS] - predict).abs().max()) <= 1e-9 and float((rows[:, R.MEL_BINS] - stop).abs().max()) <= 1e-9
        for p in (0, 1, 2, MC.MEL_PASSES - 1):
            frame = forced[p - 1] if p else torch.zeros(R.MEL_BINS)
            wrong = R.wrong_step(S, ui == 0, p)
            assert (p == 0) or set(wrong) >= {"drop_oldest", "drop_newest", "newest_twice", "stale_newest", "drop_split", "mem_other_layer"}
            for w, lg in ref.step(frame, p, kv, mem, S, wrong).items():
                sep = R.units((lg - rows[p]).abs(), C_LOGIT * R.U32 * scales[p])
                assert sep >= SEP + 1, (name, ui, p, w, sep)
        for w in R.wrong_enc(S, ref.norm_first, c["precision"] == "bf16"):
            sep = 0.0
            for (k, v, ka, va), (wk, wv, _, _) in zip(right, ref.memory_kv(text, w)):
                sep = max(sep, R.units((wk - k).abs(), u * ka), R.units((wv - v).abs(), u * va))
            assert sep >= SEP + 1, (name, ui, w, sep)
    assert set(R.wrong_enc(129, True, False)) == set(R.WRONG_ENC) and "enc_no_final_norm" not in R.wrong_enc(129, False, False)
    assert set(R.wrong_enc(5, True, True)) == set(R.WRONG_ENC) and min(MC.MEL_TEXT_LENS[1:2]) <= R.ENC_FEW_KEYS  # a text that shows it


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", MC.GEMM_SHAPES)
def test_gemm_wrong_answers_are_separated_from_the_reference(shape, bf16):
    A, W, b = MC.gemm_inputs(shape, bf16)
    if bf16:
        assert torch.equal(A, A.to(torch.bfloat16).float()) and torch.equal(W, W.to(torch.bfloat16).float())
    for variant in MC.GEMM_VARIANTS:
        bias, relu = (b if variant != "plain" else None), variant == "relu"
        right, scale = R.gemm(A, W, bias, relu)
        wrong = R.gemm_wrong(A, W, bias, relu)
        assert set(wrong) == {"drop_last_k", "last_col_from_before", "k_rounded_up"}
        for name, w in wrong.items():
            sep = R.units((w - right).abs(), MC.C_GEMM_SIMPLE * R.U32 * scale)
            assert sep >= SEP + 1, (shape, variant, name, sep)


def test_gemm_shapes_reach_the_guards():
    assert any(N % 64 for _, N, _ in MC.GEMM_SHAPES) and any(K % 32 for _, _, K in MC.GEMM_SHAPES)
    assert any(M % 64 and N % 64 and K % 32 for M, N, K in MC.GEMM_SHAPES)
    assert any(K % 32 and K % 8 for _, _, K in MC.GEMM_SHAPES)  # the k guard falls inside a loader's run of 8


def test_gemm_exact_shape_is_exact_in_fp32():
    A, W, b = MC.gemm_inputs(MC.GEMM_EXACT_SHAPE, False)
    assert torch.equal(A, A.to(torch.bfloat16).float()) and torch.equal(W, W.to(torch.bfloat16).float())  # bf16 holds them too
    for variant in MC.GEMM_VARIANTS:
        bias, relu = (b if variant != "plain" else None), variant == "relu"
        right, scale = R.gemm(A, W, bias, relu)
        assert float(scale.max()) + 16 < 2 ** 24 and torch.equal(right, right.round())
        c32 = A @ W.t()
        c32 = c32 + bias if bias is not None else c32
        assert torch.equal((c32.clamp_min(0) if relu else c32).double(), right)
