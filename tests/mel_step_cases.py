"""The cases of the mel Transformer's kernel and step tests, shared by tests/test_mel_step_cpu.py (which vets them without a GPU) and
tests/test_gpu_mel_open.py, tests/test_gpu_mel_step.py, test_gpu_kernels.py::test_gemm_simple_ragged (which compare): seeded inputs,
computed once per case and left unchanged."""
import torch

import mel_step_ref as R

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def parity_note(key: str, value):
    """The GPU tests' measured figures: adds one entry to the JSON file VX_MEL_STEP_PARITY_OUT names, if it names one
    (profiles/mel_step_parity.json is the output of such a run on the MI355X)."""
    import json
    import os

    path = os.environ.get("VX_MEL_STEP_PARITY_OUT")
    if not path:
        return
    data = {}
    if os.path.isfile(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


# ---- mel_open_kernel ---------------------------------------------------------------------------------------------------------------
# d -> (per, rows of the last non-empty slice, workgroups that own nothing): every clamp of the launcher's slicing is crossed
OPEN_WIDTHS = {8: (1, 1, 8), 64: (4, 4, 0), 192: (12, 12, 0), 200: (13, 5, 0), 1000: (63, 55, 0), 1016: (64, 56, 0), 1024: (64, 64, 0)}
OPEN_PRENETS = (False, True)  # linear (K0 = 100), MLP (K0 = 256)
OPEN_PE_ROWS = 12
OPEN_ROWS = (-1, 0, 1, OPEN_PE_ROWS - 2)
OPEN_CAP = 8  # frame rows and stop slots of the test buffers


def open_inputs(d: int, mlp: bool):
    """fp32 operands of one launch: a residual row with a mean and a spread, two norm sites, a head and a prenet at the scale of
    trained layers, a random position table (every channel of every row differs)."""
    def make():
        g = torch.Generator().manual_seed(1000 * d + int(mlp))
        rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
        K0 = R.MEL_PRENET_H if mlp else R.MEL_BINS
        i = dict(xh=rn(d) * 3.0 + 0.5, gamma=1.0 + rn(d, scale=0.2), beta=rn(d, scale=0.2), gamma2=1.0 + rn(d, scale=0.2),
                 beta2=rn(d, scale=0.2), Wh=rn(R.MEL_HEAD, d, scale=d ** -0.5), bh=rn(R.MEL_HEAD, scale=0.3),
                 W0=rn(d, K0, scale=K0 ** -0.5), b0=rn(d, scale=0.3), alpha=torch.tensor([0.8125 + 2.0 ** -12]),
                 pe=rn(OPEN_PE_ROWS, d), forced=rn(OPEN_CAP, R.MEL_BINS), W1=None, b1=None, W2=None, b2=None)
        if mlp:
            i.update(W1=rn(K0, R.MEL_BINS, scale=0.1), b1=rn(K0, scale=0.3), W2=rn(K0, K0, scale=K0 ** -0.5), b2=rn(K0, scale=0.3))
            i["b2"][-4:] = i["b2"][-4:].abs() + 2.0  # the last four hidden units stay active: a load clamped at K0 - 4 must show
        i["bh"][R.MEL_BINS] -= float(R.open_head(i)[0][R.MEL_BINS]) + 1.0  # stop logit about -1: the decode goes on by itself
        return i
    return _once(("open", d, mlp), make)


def open_exact_inputs(d: int, mlp: bool):
    """open_inputs with a prenet that is exact in fp32: forced frames and biases integers in [-2, 2], prenet weights in {-1, 0, 1}.
    |layer 1| <= 202, |layer 2| <= 256 x 202 + 2, |any partial sum of the last layer| <= 256 x 51714 + 2 < 2^24: every product
    and every partial sum of any order is an integer fp32 holds.  alpha and pe stay arbitrary fp32 values, so the position product
    rounds once and the sum once."""
    def make():
        g = torch.Generator().manual_seed(2000 * d + int(mlp))
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        K0 = R.MEL_PRENET_H if mlp else R.MEL_BINS
        i = dict(open_inputs(d, mlp))
        i.update(W0=ri(-1, 1, d, K0), b0=ri(-2, 2, d), forced=ri(-2, 2, OPEN_CAP, R.MEL_BINS))
        if mlp:  # the MLP's rows reach the thousands: alpha at that scale, or the product's rounding would never show in the sum
            i.update(W1=ri(-1, 1, K0, R.MEL_BINS), b1=ri(-2, 2, K0), W2=ri(-1, 1, K0, K0), b2=ri(-2, 2, K0),
                     alpha=torch.tensor([1000.123]))
        return i
    return _once(("open_exact", d, mlp), make)


def with_stop(inp, value: float):
    """The inputs with the stop logit set exactly: stop_layer's row zeroed, the value in its bias."""
    i = dict(inp)
    i["Wh"], i["bh"] = inp["Wh"].clone(), inp["bh"].clone()
    i["Wh"][R.MEL_BINS] = 0.0
    i["bh"][R.MEL_BINS] = value
    return i


NAN = float("nan")
# name -> (stop value, state in, max_frames, n_forced); the expected state after is mel_step_ref.open_rule's, and
# OPEN_RULE_WANT below states it once more by hand for the rows of the rule's table
_ST = lambda row, n_gen, S, done=0: dict(row=row, **{"pass": row}, n_gen=n_gen, S=S, done=done, stop_reason=0)
OPEN_RULE = {
    "plus_zero": (0.0, _ST(3, 3, 2), 50, 0),
    "minus_zero": (-0.0, _ST(3, 3, 2), 50, 0),
    "nan": (NAN, _ST(3, 3, 2), 50, 0),
    "smallest_positive": (2.0 ** -149, _ST(3, 3, 2), 50, 0),
    "length_edge_below": (-1.0, _ST(9, 5, 1), 50, 0),        # row + 1 == 10 S
    "length_edge": (-1.0, _ST(10, 5, 1), 50, 0),             # row + 1 == 10 S + 1
    "length_and_logit": (1.0, _ST(10, 5, 1), 50, 0),
    "length_and_max_frames": (-1.0, _ST(10, 5, 1), 5, 0),
    "logit_and_max_frames": (1.0, _ST(3, 3, 2), 3, 0),
    "max_frames": (-1.0, _ST(3, 3, 2), 3, 0),
    "forced_continues": (-1.0, _ST(2, 2, 2), 50, 5),
    "forced_last": (-1.0, _ST(4, 4, 2), 50, 5),
    "forced_ignores_logit_and_length": (1.0, _ST(10, 2, 1), 1, 5),
    "done": (1.0, _ST(3, 3, 2, done=1), 50, 0),
}
# name -> (row, pass, n_gen, done, stop_reason) after the launch
OPEN_RULE_WANT = {
    "plus_zero": (4, 4, 4, 0, R.STOP_NONE),
    "minus_zero": (4, 4, 4, 0, R.STOP_NONE),
    "nan": (4, 4, 4, 0, R.STOP_NONE),
    "smallest_positive": (3, 4, 3, 1, R.STOP_LOGIT),
    "length_edge_below": (10, 10, 6, 0, R.STOP_NONE),
    "length_edge": (10, 11, 5, 1, R.STOP_LENGTH),
    "length_and_logit": (10, 11, 5, 1, R.STOP_LENGTH),
    "length_and_max_frames": (10, 11, 5, 1, R.STOP_LENGTH),
    "logit_and_max_frames": (3, 4, 3, 1, R.STOP_LOGIT),
    "max_frames": (3, 4, 3, 1, R.STOP_MAX_FRAMES),
    "forced_continues": (3, 3, 3, 0, R.STOP_NONE),
    "forced_last": (4, 5, 5, 1, R.STOP_MAX_FRAMES),
    "forced_ignores_logit_and_length": (11, 11, 3, 0, R.STOP_NONE),
    "done": (3, 3, 3, 1, R.STOP_NONE),
}
OPEN_RULE_WIDTHS = (8, 200)  # the rule is the same code at every width: the smallest, and a ragged one


# ---- the decode step and the encoder on an engine ------------------------------------------------------------------------------------
MEL_CASES = {
    "m_bf16_d1024": dict(precision="bf16", d=1024, H=16),                  # head_dim 64: the MFMA row path
    "m_fp32_d192": dict(precision="fp32", d=192, H=12),                    # per = 12; head_dim 16
    "m_bf16_d256_hd64": dict(precision="bf16", d=256, H=4),
    "m_fp32_hd4_prenet": dict(precision="fp32", d=64, H=16, add_prenet=True),
    "m_bf16_postnorm": dict(precision="bf16", d=512, H=8, norm_first=False),
}
MEL_L = 2
MEL_SEED = 11
MEL_TEXT_LENS = (129, 5, 64, 65, 1)  # every shorter text after a longer one (stale memory rows); the 64-key tile edge; one key
MEL_PASSES = 12
MEL_MAX_TEXT, MEL_MAX_FRAMES = 160, 16
# The q rows of the encoder's self-attention, as test_gpu_ar_step.Q_SHARPEN for the decoder's.  Sharper (16) was tried: one key of
# 129 then moves a bf16 memory row by 5 units instead of 2, but the engine's own rounding error on those rows grows as much
# (1.22 units measured against 0.39), so nothing is gained in bounds.
ENC_Q_SHARPEN = 4.0


def mel_config(c):
    from valle_amd.config import MelConfig

    return MelConfig(d_model=c["d"], nhead=c["H"], num_layers=MEL_L, norm_first=c.get("norm_first", True),
                     add_prenet=c.get("add_prenet", False))


def mel_inputs(c, q_sharpen: float):
    """(state dict, [(text (S,), forced frames (MEL_PASSES, 100))]) of a case: synthetic weights with the q rows of every
    attention's in_proj scaled by q_sharpen (the decoder's two, as the VALL-F step test) and those of the encoder's by ENC_Q_SHARPEN; the forced frames
    at the scale of log-mel frames."""
    def make():
        from valle_amd.weights import mel_synthetic_state_dict

        sd = mel_synthetic_state_dict(mel_config(c), MEL_SEED, stop_bias=-1.0)
        d = c["d"]
        for li in range(MEL_L):
            sd[f"decoder.layers.{li}.self_attn.in_proj_weight"][:d] *= q_sharpen
            sd[f"decoder.layers.{li}.multihead_attn.in_proj_weight"][:d] *= q_sharpen
            sd[f"encoder.layers.{li}.self_attn.in_proj_weight"][:d] *= ENC_Q_SHARPEN
        g = torch.Generator().manual_seed(MEL_SEED)
        for li in range(MEL_L):  # norms as unlike each other as trained ones: a norm read at another site must show
            for n in (1, 2):
                sd[f"encoder.layers.{li}.norm{n}.weight"] = 0.5 + torch.rand(d, generator=g)
                sd[f"encoder.layers.{li}.norm{n}.bias"] = 0.3 * torch.randn(d, generator=g)
        utts = [(torch.randint(3, 100, (S,), generator=g), torch.randn(MEL_PASSES, R.MEL_BINS, generator=g)) for S in MEL_TEXT_LENS]
        return sd, utts
    return _once(("mel", tuple(sorted(c.items())), q_sharpen), make)


def mel_ref(c, sd):
    return R.MelStepRef(sd, c["d"], c["H"], MEL_L, c.get("norm_first", True), c.get("add_prenet", False), c["precision"] == "bf16",
                        pe_rows=max(4000, MEL_MAX_TEXT + MEL_MAX_FRAMES + 2))


# ---- gemm_simple_kernel --------------------------------------------------------------------------------------------------------------
# (M, N, K): the teacher-forced head (N = 101), both decoder prenets (K = 100), ragged M, N and K together
GEMM_SHAPES = ((1, 101, 64), (60, 101, 192), (96, 101, 1024), (33, 256, 100), (65, 200, 100), (7, 8, 100), (5, 1000, 256))
GEMM_EXACT_SHAPE = (64, 64, 32)
GEMM_VARIANTS = ("plain", "bias", "relu")
# Bound in units of 2^-24 sum |a| |w|.  Not test_gpu_ar_step.C_LOGIT (3.5): gemm_simple_kernel sums each output in ONE fp32 fmaf
# chain over k = 0 .. K - 1, where the decode step's GEMVs (which C_LOGIT was measured on) split a row over the lanes of a wave
# and add the partial sums as a tree, so every rounding here meets a partial sum of up to the whole row.  A host emulation of that
# single chain (numpy, fp32 after every fused step) on these inputs gives the kernel's own figures to four digits: worst 3.902
# units at (60, 101, 192) fp32, where the MI355X measured 3.902; bf16 operands (products exact in fp32) 2.97.  4 x measured:
C_GEMM_SIMPLE = 15.6


def gemm_inputs(shape, bf16: bool):
    """(A (M, K), W (N, K), bias (N,)) fp32, holding bf16 values when bf16; the exact shape: integers, |partial sums| <= 32 K + 16."""
    def make():
        M, N, K = shape
        g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K)
        if shape == GEMM_EXACT_SHAPE:
            ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
            return ri(-4, 4, M, K), ri(-8, 8, N, K), ri(-16, 16, N)
        A, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
        if bf16:
            A, W = A.to(torch.bfloat16).float(), W.to(torch.bfloat16).float()
        return A, W, b
    return _once(("gemm", shape, bf16), make)
