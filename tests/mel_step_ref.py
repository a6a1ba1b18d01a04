"""fp64 references of the code only the mel-spectrogram Transformer runs (vall-e_amd/csrc/meltf.hip mel_open_kernel, the encoder side
of engine.hip mel_encode_rows, gemm_simple_kernel at the ragged shapes of the teacher-forced head and the prenets), for
tests/test_gpu_mel_open.py, tests/test_gpu_mel_step.py, test_gemm_simple_ragged and tests/test_mel_step_cpu.py.

Every reference takes the values the kernel reads (fp32, or the bf16 roundings an engine stores) and computes in float64.  Next to
each right answer stands its error unit's scale, sum |w| |h| + |b|, and the nearest wrong answers a faulty kernel would give."""
import torch
import torch.nn.functional as F

import meltf_ref as MR
from ar_step_ref import WRONG_MEM, StepRefF, engine_state_dict

U32 = 2.0 ** -24
MEL_BINS, MEL_HEAD, MEL_PRENET_H, MEL_GRID = 100, 101, 256, 16
STOP_NONE, STOP_LOGIT, STOP_LENGTH, STOP_MAX_FRAMES = 0, 1, 2, 3


def units(err: torch.Tensor, scale: torch.Tensor) -> float:
    """max err / scale; a NaN error counts as infinitely far; where scale is 0 only err == 0 passes."""
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    m = scale > 0
    if bool((err[~m] != 0).any()):
        return float("inf")
    return float((err[m] / scale[m]).max()) if bool(m.any()) else 0.0


# ---- mel_open_kernel ---------------------------------------------------------------------------------------------------------------
def open_slices(d: int):
    """(per, [(lo, hi)] of the MEL_GRID workgroups): the launcher's split of the d prenet rows."""
    per = (d + MEL_GRID - 1) // MEL_GRID
    return per, [(min(b * per, d), min(min(b * per, d) + per, d)) for b in range(MEL_GRID)]


def _dbl(inp):
    return {k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}


def open_head(inp, gamma="gamma", beta="beta", chans=None):
    """Final LayerNorm of xh and the 101 head rows -> (out (101,), scale (101,) = sum |w| |h| + |b|).  chans: the dot products
    run over the first ``chans`` channels only (a wrong answer)."""
    i = _dbl(inp)
    d = i["xh"].numel()
    h = F.layer_norm(i["xh"], (d,), i[gamma], i[beta], 1e-5)
    W = i["Wh"]
    if chans is not None:
        W, h = W[:, :chans], h[:chans]
    return W @ h + i["bh"], W.abs() @ h.abs() + i["bh"].abs()


def open_prenet(inp, frame, k_in=None, dtype=torch.float64):
    """decoder_prenet(frame) -> (y (d,), scale (d,)) of its last layer; k_in: that layer reads its first k_in inputs only."""
    i = {k: (v.to(dtype) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    h = frame.to(dtype)
    if inp.get("W1") is not None:
        h = F.relu(i["W1"] @ h + i["b1"])
        h = F.relu(i["W2"] @ h + i["b2"])
    W0 = i["W0"]
    if k_in is not None:
        W0, h = W0[:, :k_in], h[:k_in]
    return W0 @ h + i["b0"], W0.abs() @ h.abs() + i["b0"].abs()


def open_x(inp, frame, pos: int, k_in=None):
    """The next input row decoder_prenet(frame) + alpha pe[pos] -> (x (d,), scale (d,))."""
    y, sc = open_prenet(inp, frame, k_in)
    p = inp["alpha"].double()[0] * inp["pe"].double()[pos]
    return y + p, sc + p.abs()


def open_x_exact32(inp, frame, pos: int):
    """The next input row where the prenet is exact in fp32 (open_exact_inputs): fadd(prenet, fmul(alpha, pe)), two roundings."""
    y, _ = open_prenet(inp, frame, dtype=torch.float32)
    return y + inp["alpha"][0] * inp["pe"][pos]


def open_rule(st, stop: float, max_frames: int, n_forced: int):
    """The kernel's book-keeping on the state words -> (state after, appended, go).  transformer.py:376-383: the stop rule is
    tested before the append; the length rule stands in front of the logit's; teacher forcing ignores both."""
    st = dict(st)
    st.setdefault("stop_reason", 0)
    if st["done"]:
        return st, False, False
    reason, append, go = STOP_NONE, False, True
    if st["row"] >= 0:
        if n_forced > 0:
            append = True
            if st["n_gen"] + 1 >= n_forced:
                reason = STOP_MAX_FRAMES
        elif st["row"] + 1 > 10 * st["S"]:
            reason = STOP_LENGTH
        elif stop > 0:  # false for NaN and for either zero
            reason = STOP_LOGIT
        elif st["n_gen"] >= max_frames:
            reason = STOP_MAX_FRAMES
        else:
            append = True
        go = append and reason == STOP_NONE
        st["pass"] += 1
        if append:
            st["n_gen"] += 1
        if reason != STOP_NONE:
            st["done"], st["stop_reason"] = 1, reason
    if go:
        st["row"] += 1
    return st, append, go


def open_wrong(inp, row: int, frame):
    """The nearest wrong answers of one launch at position ``row`` with the fed-back ``frame`` (100,): name -> ("head", (101,)) or
    ("x", (d,)).  Head ones exist for row >= 0 only (row -1 computes no head); K0 - 4 inputs mean nothing for the linear prenet on
    the all-zero frame of row -1 (every input is zero); pe[row] does not exist at row -1, where pe[1] stands for it."""
    d = inp["xh"].numel()
    mlp = inp.get("W1") is not None
    K0 = MEL_PRENET_H if mlp else MEL_BINS
    out = {}
    if row >= 0:
        head, _ = open_head(inp)
        out["head_d_minus_4"] = ("head", open_head(inp, chans=d - 4)[0])
        h = head.clone()
        h[MEL_BINS] = h[MEL_BINS - 1]
        out["stop_from_row_99"] = ("head", h)
        out["other_site_norm"] = ("head", open_head(inp, "gamma2", "beta2")[0])
    x, _ = open_x(inp, frame, row + 1)
    a = x.clone()
    a[d - 1] = float("nan")
    out["last_row_unwritten"] = ("x", a)
    a = x.clone()
    a[d - 1] = x[d - 2]
    out["last_row_from_before"] = ("x", a)
    out["pe_row"] = ("x", open_x(inp, frame, row if row >= 0 else 1)[0])
    if mlp or row >= 0:
        out["k0_minus_4"] = ("x", open_x(inp, frame, row + 1, k_in=K0 - 4)[0])
    return out


# ---- gemm_simple_kernel --------------------------------------------------------------------------------------------------------------
def gemm(A, W, bias=None, relu=False):
    """fp64 products of the stored values -> (C (M, N), scale (M, N) = sum |a| |w|)."""
    A, W = A.double(), W.double()
    c = A @ W.t()
    if bias is not None:
        c = c + bias.double()
    return (F.relu(c) if relu else c), A.abs() @ W.abs().t()


def gemm_wrong(A, W, bias=None, relu=False):
    """name -> C (M, N): the k = K - 1 term dropped; column N - 1 taken from N - 2; K rounded up to 128, reading on into the next
    row of both operands (behind the last row, the first rows again)."""
    (M, K), N = A.shape, W.shape[0]
    out = {"drop_last_k": gemm(A[:, : K - 1], W[:, : K - 1], bias, relu)[0]}
    c = gemm(A, W, bias, relu)[0].clone()
    c[:, N - 1] = c[:, N - 2]
    out["last_col_from_before"] = c
    Kp = (K + 127) // 128 * 128 if K % 128 else K + 128
    flat = lambda t: torch.cat([t.double().reshape(-1)] * (2 + Kp // t.numel()))
    fa, fw = flat(A), flat(W)
    Ap = torch.stack([fa[m * K: m * K + Kp] for m in range(M)])
    Wp = torch.stack([fw[n * K: n * K + Kp] for n in range(N)])
    out["k_rounded_up"] = gemm(Ap, Wp, bias, relu)[0]
    return out


# ---- the decode step and the encoder of an engine ----------------------------------------------------------------------------------
class MelStepRef(StepRefF):
    """StepRefF for a mel engine: the decoder layers are the VALL-F step's (StepRefF.forward as it is); the input row is
    decoder_prenet(frame) + alpha pe[row] and the head is 101 rows with a bias, behind decoder.norm (pre-norm) or the last norm3
    (post-norm, applied by the layer itself).  ``token`` of StepRefF.forward is the fed-back frame (100,)."""

    def __init__(self, sd, d: int, nhead: int, num_layers: int, norm_first: bool = True, add_prenet: bool = False, bf16: bool = True,
                 pe_rows: int = 4000):
        from oracle import valle_oracle as vo
        from valle_amd.weights import sine_table

        self.sd = engine_state_dict(sd, bf16)
        self.d, self.H, self.L = d, nhead, num_layers
        self.hd = d // nhead
        self.norm_first, self.add_prenet = norm_first, add_prenet
        self.pe = sine_table(pe_rows, d).double()
        self.layers = [vo._DecLayer(self.sd, f"decoder.layers.{i}", False) for i in range(num_layers)]
        self.in_abs = [(L.in_w.abs(), L.in_b.abs()) for L in self.layers]
        self.cin_abs = [(L.cin_w[d:].abs(), L.cin_b[d:].abs()) for L in self.layers]
        self.head = torch.cat([self.sd["predict_layer.weight"], self.sd["stop_layer.weight"]])
        self.head_b = torch.cat([self.sd["predict_layer.bias"], self.sd["stop_layer.bias"]])
        self.head_abs = self.head.abs()
        self.oracle = self  # StepRefF.forward asks its oracle for the final norm only
        self.mel = MR.MelRef(self.sd, d, nhead, num_layers, norm_first, add_prenet, torch.float64, pe=self.pe)

    def ar_final_norm(self, x):
        return MR._ln(x, self.sd, "decoder.norm") if self.norm_first else x

    def embed(self, frame, pos: int):
        inp = {"W0": self.sd["decoder_prenet.6.weight" if self.add_prenet else "decoder_prenet.weight"],
               "b0": self.sd["decoder_prenet.6.bias" if self.add_prenet else "decoder_prenet.bias"], "W1": None}
        if self.add_prenet:
            inp.update(W1=self.sd["decoder_prenet.0.weight"], b1=self.sd["decoder_prenet.0.bias"],
                       W2=self.sd["decoder_prenet.3.weight"], b2=self.sd["decoder_prenet.3.bias"])
        return open_prenet(inp, frame)[0] + self.sd["decoder_position.alpha"][0] * self.pe[pos]

    def step(self, frame, row: int, kv, mem, S: int, variant=None, own_newest: bool = False):
        """One decode pass on input row ``row`` (cache row ``row``) -> StepRefF.forward's result with the head's bias added:
        "logits" (101,) = [frame | stop logit], "head_abs" = sum |w| |h| + |b|; a list of variants -> {name: (101,)}."""
        r = self.forward(frame.double(), row, kv, mem, row, S, variant, own_newest)
        if isinstance(variant, (list, tuple)):
            return {k: v + self.head_b for k, v in r.items()}
        r["logits"] = r["logits"] + self.head_b
        r["head_abs"] = r["head_abs"] + self.head_b.abs()
        return r

    # -- the encoder side: one reference, with the wrong answers a faulty mel_encode_rows would give
    def encode(self, text, variant=None):
        """(S, d) rows the decoder layers' cross in_proj reads: embedding or encoder prenet, + alpha pe, L encoder layers, the final
        norm.  variant None is MelRef.encode itself.  "enc_last_unseen": no query sees the last text row as a key; "enc_causal":
        a causal mask; "enc_no_final_norm" (pre-norm only); "enc_norm_sites_3": the layers' 2 L norms read at the sites of
        three-per-layer arithmetic, 3 li + {0, 2} into the stack's norms in order, wrapping."""
        if variant is None:
            return self.mel.encode(text)
        sd, H = self.sd, self.H
        x = self._embed_text(text)
        flat = [f"encoder.layers.{i}.norm{k}" for i in range(self.L) for k in (1, 2)]
        for i in range(self.L):
            p = f"encoder.layers.{i}"
            n1, n2 = (flat[(3 * i) % len(flat)], flat[(3 * i + 2) % len(flat)]) if variant == "enc_norm_sites_3" else (p + ".norm1", p + ".norm2")
            causal = variant == "enc_causal"
            keys = (lambda h: h[:-1]) if variant == "enc_last_unseen" else (lambda h: h)
            if self.norm_first:
                h = MR._ln(x, sd, n1)
                x = x + MR._mha(sd, p + ".self_attn", h, keys(h), H, causal)
                x = x + MR._ff(sd, p, MR._ln(x, sd, n2))
            else:
                x = MR._ln(x + MR._mha(sd, p + ".self_attn", x, keys(x), H, causal), sd, n1)
                x = MR._ln(x + MR._ff(sd, p, x), sd, n2)
        if self.norm_first and variant != "enc_no_final_norm":
            x = MR._ln(x, sd, "encoder.norm")
        return x

    def _embed_text(self, text):
        """MelRef.encode with no layer and no final norm: the rows that enter the encoder stack."""
        m = self.mel
        L, nf = m.L, m.norm_first
        m.L, m.norm_first = 0, False
        try:
            return m.encode(text)
        finally:
            m.L, m.norm_first = L, nf

    def memory_kv(self, text, variant=None):
        """Every decoder layer's cross K / V of the encoded text: per layer (k, v, k_abs, v_abs), each (H, S, hd); *_abs =
        sum |w| |h| + |b| of the cross in_proj's row."""
        x = self.encode(text, variant)
        S, H, hd, d = text.shape[0], self.H, self.hd, self.d
        res = []
        for li, L in enumerate(self.layers):
            wa, ba = self.cin_abs[li]
            k, v = (x @ L.cin_w[d:].t() + L.cin_b[d:]).view(S, 2, H, hd).permute(1, 2, 0, 3)
            ka, va = (x.abs() @ wa.t() + ba).view(S, 2, H, hd).permute(1, 2, 0, 3)
            res.append((k, v, ka, va))
        return res

    def memory(self, text, rows: int, variant=None):
        """memory_kv as the engine's tap holds it: (L, 2, H, rows, hd), rows past S zero."""
        S = text.shape[0]
        mem = torch.zeros(self.L, 2, self.H, rows, self.hd, dtype=torch.float64)
        for li, (k, v, _, _) in enumerate(self.memory_kv(text, variant)):
            mem[li, 0, :, :S], mem[li, 1, :, :S] = k, v
        return mem


WRONG_ENC = ("enc_last_unseen", "enc_causal", "enc_no_final_norm", "enc_norm_sites_3")


ENC_FEW_KEYS = 8


def wrong_enc(S: int, norm_first: bool, bf16: bool):
    """The encoder's wrong answers that mean something on a text of S ids: one text row has no other key to lose and no mask to
    feel; a post-norm encoder has no final norm.  On bf16 engines "enc_last_unseen" is judged on texts of at most ENC_FEW_KEYS
    ids: one key of S carries about 1 / S of a row, and a bf16 memory row's unit, 2^-8 sum |w| |h|, is about a tenth of the row's
    own magnitude (the sum of magnitudes exceeds the magnitude of the sum by about sqrt(d)), so that a row computed from entirely
    different inputs lies only 20 - 50 units away and one key of 64 or more 2 - 7: less than any bound on those rows could tell
    from rounding.  fp32 engines show it on every text, 1e5 units away."""
    out = [w for w in WRONG_ENC if norm_first or w != "enc_no_final_norm"]
    out = [w for w in out if S > 1 or w not in ("enc_last_unseen", "enc_causal")]
    return [w for w in out if not (bf16 and S > ENC_FEW_KEYS and w == "enc_last_unseen")]


def wrong_step(S: int, first: bool, row: int):
    """ar_step_ref.wrong_f for decode row ``row``: at row 0 the cache holds the newest key alone, so the self-attention's wrong
    answers (a key dropped, row - 1 for row) do not exist; the memory's do."""
    from ar_step_ref import wrong_f

    return [w for w in wrong_f(S, first) if row > 0 or w in WRONG_MEM]
