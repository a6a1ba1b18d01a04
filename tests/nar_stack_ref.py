"""fp64 reference of the NAR stages as the engine's row stack runs them (vall-e_amd/csrc/engine.hip nar_run / run_stack), layer by
layer, for tests/test_gpu_nar_stack.py.

The operands are the values the engine stores (ar_step_ref.engine_state_dict: the matrices vx_set_weight converts rounded to
bf16, everything else fp32) inside the oracle model of score_ref.oracle; every operation then runs in float64, on whichever
device the state dict was moved to.  What this file adds to those pieces is the layer loop written out, so that it can also return

  the budgets   head_abs = |h_f| |W_head|^T of the logits (h_f: the row the predict layer reads) and x_abs = the per-element
                sum over the layers of |att| |W_out|^T + |b_out| + |ff| |W_2|^T + |b_2| (what the two N = d GEMMs of every layer
                add to the residual stream: the out-projection and FFN2, whose split-K slabs the next LayerNorm folds);
  wrong answers one named mistake of the fold / stage bookkeeping applied, everything else unchanged (WRONG).

Teacher-forced like vx_nar_ex with forced_codes: stage i sees the given codes of codebooks 0..i (score_ref.nar_score_logits is
the same forward through the oracle's own nar_stack; the two agree to fp64 rounding: tests/test_nar_stack_ref_cpu.py)."""
import math

import torch
import torch.nn.functional as F

from ar_step_ref import engine_state_dict
from oracle import valle_oracle as vo
from score_ref import oracle

WRONG = (
    "no_out_bias_l0",     # out-projection bias of layer 0 missing (the fold's pbias)
    "no_ffn2_bias_last",  # FFN2 bias of the last layer missing (the fold-only pass after the last layer)
    "drop_out_slice_l1",  # one K slice of layer 1's out-projection missing (a slab not folded)
    "other_stage_ada",    # the other stage's AdaLN vectors, in every norm
    "pos_shift",          # the audio position table shifted by one row
    "no_prompt_cb",       # prompt embeddings of codebooks >= 1 left out
)


class NarRef:
    def __init__(self, cfg, sd, device, pe_rows: int = 4000):
        from valle_amd.weights import sine_table

        esd = {k: v.to(device) for k, v in engine_state_dict(sd, bf16=True).items()}
        self.m = oracle(cfg, esd, torch.float64)
        self.cfg, self.sd, self.dev = cfg, self.m.sd, device
        self.d, self.H, self.Q = self.m.dn, self.m.nar_nhead, self.m.Q
        self.pe = sine_table(pe_rows, self.d).double().to(device)  # the table the engine is given (Engine.load_state_dict)

    def _stage_emb(self, stage):
        return self.sd[f"nar_stage_embeddings.{stage}.word_embeddings.weight"]

    def _attention(self, qkv):
        n, H, hd = qkv.shape[0], self.H, self.d // self.H
        q, k, v = (t.reshape(n, H, hd).transpose(0, 1) for t in qkv.chunk(3, dim=-1))  # (H, n, hd); no mask in the NAR stages
        p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(hd), dim=-1)
        return (p @ v).transpose(0, 1).reshape(n, self.d)

    def inputs(self, text, codes, P, stage, variant=None):
        """[text | prompt + generated] rows of stage `stage` (valle.py:1063-1123 with the given codes of the earlier stages)"""
        sd, Q = self.sd, self.Q
        emb = lambda j: sd[f"nar_audio_embeddings.{j}.word_embeddings.weight"]  # noqa: E731
        assert self.cfg.prefix_mode == 1 and not self.cfg.add_prenet
        y = F.embedding(codes[:, 0], emb(0)).clone()
        if variant != "no_prompt_cb":
            for j in range(1, Q):
                y[:P] += F.embedding(codes[:P, j], emb(j))
        for i in range(stage):
            y[P:] += F.embedding(codes[P:, i + 1], emb(i + 1))
        S, A = text.shape[0], codes.shape[0]
        x = F.embedding(text, sd["nar_text_embedding.word_embeddings.weight"]) + sd["nar_text_position.alpha"] * self.pe[:S]
        off = 1 if variant == "pos_shift" else 0
        return torch.cat([x, y + sd["nar_audio_position.alpha"] * self.pe[off:off + A]], 0)

    @torch.no_grad()
    def forward(self, text, codes, P, stage, variant=None, slices=4):
        """One stage.  text (S,), codes (A, Q) on the reference's device.  Returns dict(logits (T, 1024), x (M, d) = the residual
        stream the stack leaves; and, for variant None, head_abs (T, 1024), x_abs (M, d)).  `slices`: how many K slices the
        out-projection has in 'drop_out_slice_l1' (the second one is dropped)."""
        assert variant is None or variant in WRONG
        m, sd, d = self.m, self.sd, self.d
        S = text.shape[0]
        e = self._stage_emb(1 - stage if variant == "other_stage_ada" else stage)
        x = self.inputs(text, codes, P, stage, variant)
        budget = variant is None
        x_abs = torch.zeros_like(x) if budget else None
        last = len(m.nar_layers) - 1
        for li, L in enumerate(m.nar_layers):
            h = L.norm(0, x, e) if m.norm_first else x
            att = self._attention(F.linear(h, L.in_w, L.in_b))
            o = F.linear(att, L.out_w, None if (variant == "no_out_bias_l0" and li == 0) else L.out_b)
            if variant == "drop_out_slice_l1" and li == 1:
                k0, k1 = d // slices, 2 * (d // slices)
                o = o - att[:, k0:k1] @ L.out_w[:, k0:k1].T
            x = x + o
            if not m.norm_first:
                x = L.norm(0, x, e)
            ff = F.relu(F.linear(L.norm(1, x, e) if m.norm_first else x, L.w1, L.b1))
            x = x + F.linear(ff, L.w2, None if (variant == "no_ffn2_bias_last" and li == last) else L.b2)
            if not m.norm_first:
                x = L.norm(1, x, e)
            if budget:
                x_abs += att.abs() @ L.out_w.abs().T + L.out_b.abs() + ff.abs() @ L.w2.abs().T + L.b2.abs()
        hf = x[S + P:]
        if m.norm_first:  # post-norm stacks have no final norm (valle.py:242-246)
            g = lambda n: sd[f"nar_decoder.norm.{n}"]  # noqa: E731
            hf = vo.ada_layer_norm(hf, e, g("project_layer.weight"), g("project_layer.bias"), g("norm.weight"), g("norm.bias"))
        head = sd[f"nar_predict_layers.{stage}.weight"]
        out = {"logits": hf @ head.T, "x": x}
        if budget:
            out["head_abs"] = hf.abs() @ head.abs().T
            out["x_abs"] = x_abs
        return out
