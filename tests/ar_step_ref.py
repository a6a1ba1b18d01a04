"""fp64 reference of one batch-1 AR decode pass (vall-e_amd/csrc/engine.hip enqueue_ar_step / enqueue_ar_step_tp), for
tests/test_gpu_ar_step.py.

The operands are the values the engine stores: on bf16 engines the matrices vx_set_weight converts (in_proj, out_proj, linear1,
linear2, ar_predict_layer) are rounded to bf16, everything else (embeddings, biases, norms, prenets, the fp32 sine table) stays
fp32; then every operation runs in float64.  Attention reads the ENGINE's own cache rows 0..t, row t (the newest key) included,
so that errors cannot compound from pass to pass and the check does not depend on how the cache was rounded.

``StepRef.forward`` also computes the nearest wrong answers the same way: one key fewer (the oldest or the newest row dropped),
the newest key counted twice, row t - 1 in place of row t, and one kernel split's key range dropped.

``StepRefF`` is the VALL-F form (enqueue_ar_step with e->vallf: the cross-attention block between the self-attention and the
feed-forward block).  Its cross-attention reads the ENGINE's own text memory ("ar_mem") rows 0..S-1, and it adds the wrong answers
of WRONG_MEM: a text key dropped at either end, the last one twice, one split's range dropped, row S (what an earlier, longer text
left behind) included, and another layer's memory."""
import math

import torch
import torch.nn.functional as F

from oracle import valle_oracle as vo

U32 = 2.0 ** -24  # unit roundoff of fp32
U16 = 2.0 ** -8   # unit roundoff of bf16

WRONG = ("drop_oldest", "drop_newest", "newest_twice", "stale_newest", "drop_split")


def is_matrix_key(k: str) -> bool:
    """The keys vx_set_weight stores in bf16 on bf16 engines (engine.hip is_matrix_key: a suffix test, so a VALL-F layer's
    multihead_attn.in_proj_weight / multihead_attn.out_proj.weight count like the self_attn ones; every bias, norm, embedding,
    prenet and AdaLN project_layer stays fp32)."""
    if "project_layer" in k:
        return False
    return k.endswith(("in_proj_weight", "out_proj.weight", "linear1.weight", "linear2.weight")) or \
        k.startswith(("ar_predict_layer", "nar_predict_layers"))


def engine_state_dict(sd, bf16: bool):
    """fp64 copies of the values the engine holds."""
    out = {}
    for k, v in sd.items():
        if not torch.is_floating_point(v):
            out[k] = v
            continue
        v = v.detach().float()
        if bf16 and is_matrix_key(k):
            v = v.to(torch.bfloat16).float()
        out[k] = v.double()
    return out


def split_ranges(kind: str, t: int):
    """Key ranges [j0, j1) of the kernel splits at newest row t.  'tp': tp_attn_kernel, 16 splits of the n_old = t older rows (the
    newest row is added by split 15); 'plain': attn_decode_kernel / attn_decode_small_kernel, 8 splits of the t + 1 rows."""
    n, ns = (t, 16) if kind == "tp" else (t + 1, 8)
    chunk = (n + ns - 1) // ns
    return [(j * chunk, min(n, (j + 1) * chunk)) for j in range(ns) if j * chunk < n]


def key_rows(t: int, variant, kind: str):
    """Cache rows one attention reads (duplicates count twice) at newest row t."""
    rows = list(range(t + 1))
    if variant is None:
        return rows
    if variant == "drop_oldest":
        return rows[1:]
    if variant == "drop_newest":
        return rows[:-1]
    if variant == "newest_twice":
        return rows + [t]
    if variant == "stale_newest":
        return rows[:-1] + [t - 1]
    if variant == "drop_split":
        sp = split_ranges(kind, t)
        j0, j1 = sp[len(sp) // 2]
        return [r for r in rows if not (j0 <= r < j1)]
    raise ValueError(variant)


def bf16_miss(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """How far the fp64 value ref lies outside the rounding interval of the bf16 value got: 0 where got is ref's bf16 rounding;
    for the other neighbour, ref's distance from the midpoint between the two (and near zero, where the engine's fp32 value may
    round to a bf16 value of the other sign, |got - ref| less half the spacing at ref)."""
    lo, hi = bf16_bracket(ref)
    return ((got - ref).abs() - (hi - lo) / 2).clamp(min=0)


def bf16_bracket(ref: torch.Tensor):
    """The bf16 magnitudes lo <= |ref| < hi next to |ref| (float64)."""
    a = ref.abs()
    lo = (a.float().view(torch.int32) & -65536).view(torch.float32)
    lo = torch.where(lo.double() > a, (lo.view(torch.int32) - 65536).view(torch.float32), lo)
    hi = (lo.view(torch.int32) + 65536).view(torch.float32)
    return lo.double(), hi.double()


class StepRef:
    def __init__(self, sd, d: int, nhead: int, num_layers: int, norm_first: bool = True, add_prenet: bool = False,
                 prefix_mode: int = 0, prepend_bos: bool = False, bf16: bool = True, pe_rows: int = 4000):
        from valle_amd.weights import sine_table

        self.sd = engine_state_dict(sd, bf16)
        self.d, self.H, self.L = d, nhead, num_layers
        self.hd = d // nhead
        self.norm_first, self.add_prenet = norm_first, add_prenet
        self.pe = sine_table(pe_rows, d).double()  # the table the engine is given (Engine.load_state_dict)
        self.layers = [vo._Layer(self.sd, f"ar_decoder.layers.{i}", False) for i in range(num_layers)]
        self.in_abs = [(L.in_w.abs(), L.in_b.abs()) for L in self.layers]
        self.head = self.sd["ar_predict_layer.weight"]
        self.head_abs = self.head.abs()
        self.oracle = vo.OracleModel(self.sd, d, nhead, num_layers, prefix_mode, prepend_bos, 1, 1.0, norm_first, add_prenet)

    def embed(self, token: int, pos: int) -> torch.Tensor:
        """The step's input row: audio embedding (through the audio prenet) plus alpha x the sine row of audio position pos."""
        e = self.sd["ar_audio_embedding.word_embeddings.weight"][token]
        if self.add_prenet:
            e = vo.audio_prenet(self.sd, "ar_audio_prenet", e[None])[0]
        return e + self.sd["ar_audio_position.alpha"][0] * self.pe[pos]

    def forward(self, token: int, pos: int, kv: torch.Tensor, t: int, variant=None, kind: str = "plain"):
        """One pass: ``token`` at audio position ``pos``, whose K / V the engine wrote into cache row ``t``.  kv: (L, 2, H, rows, hd)
        float64, the engine's cache.  ``variant``: None or one of WRONG (``kind`` names the kernel whose splits drop_split
        follows).  Returns dict(logits (1025,), head_abs (1025,) = sum |w| |h| of the head, and per layer k / v = the reference's
        own newest row (H, hd) with k_abs / v_abs = sum |w| |h| + |b| of it)."""
        H, hd, d = self.H, self.hd, self.d
        rows = None if variant is None else torch.tensor(key_rows(t, variant, kind))
        x = self.embed(token, pos)
        out = {"k": [], "v": [], "k_abs": [], "v_abs": []}
        for li, L in enumerate(self.layers):
            h = vo.layer_norm(x, *L.n[0]) if self.norm_first else x
            q, k, v = (L.in_w @ h + L.in_b).view(3, H, hd)
            if variant is None:
                wa, ba = self.in_abs[li]
                _, ka, va = (wa @ h.abs() + ba).view(3, H, hd)
                out["k"].append(k)
                out["v"].append(v)
                out["k_abs"].append(ka)
                out["v_abs"].append(va)
                K, V = kv[li, 0, :, : t + 1], kv[li, 1, :, : t + 1]
            else:
                K, V = kv[li, 0][:, rows], kv[li, 1][:, rows]  # (H, n, hd)
            s = torch.einsum("hc,hnc->hn", q, K) / math.sqrt(hd)
            a = torch.einsum("hn,hnc->hc", torch.softmax(s, dim=-1), V).reshape(d)
            x = x + L.out_w @ a + L.out_b
            if self.norm_first:
                x = x + L.w2 @ F.relu(L.w1 @ vo.layer_norm(x, *L.n[1]) + L.b1) + L.b2
            else:
                x = vo.layer_norm(x, *L.n[0])
                x = vo.layer_norm(x + L.w2 @ F.relu(L.w1 @ x + L.b1) + L.b2, *L.n[1])
        hf = self.oracle.ar_final_norm(x)
        out["logits"] = self.head @ hf
        out["head_abs"] = self.head_abs @ hf.abs()
        return out

    def prefill_kv(self, text: torch.Tensor, yy: torch.Tensor):
        """fp64 forward of [text | audio prefix] under the reference's AR mask.  Per layer (k, v, k_abs, v_abs), each (H, rows, hd);
        *_abs = sum |w| |h| + |b| of the row."""
        m = self.oracle
        S, A = text.shape[0], yy.shape[0]
        x = torch.cat([m.ar_text(text), m.ar_audio(yy)], dim=0).double()
        mask = vo.ar_mask(S, A)
        res = []
        H, hd, n = self.H, self.hd, S + A
        for li, L in enumerate(self.layers):
            h = vo.layer_norm(x, *L.n[0]) if self.norm_first else x
            wa, ba = self.in_abs[li]
            ab = (h.abs() @ wa.t() + ba).view(n, 3, H, hd).permute(1, 2, 0, 3)
            x, (k, v) = vo.encoder_layer(L, x, H, mask, None, self.norm_first)
            res.append((k, v, ab[1], ab[2]))
        return res


# ---- VALL-F: the step with a cross-attention block over the text memory -------------------------------------------------------------
WRONG_MEM = ("mem_drop_first", "mem_drop_last", "mem_last_twice", "mem_drop_split", "mem_one_more", "mem_other_layer")
WRONG_F = WRONG + WRONG_MEM


def mem_split_ranges(S: int):
    """Text-key ranges [j0, j1) of the non-empty splits of attn_decode_kernel / attn_decode_small_kernel with fixed_ctx: 8 splits
    of chunk = ceil(S / 8) keys; a split with j0 >= S is empty."""
    chunk = (S + 7) // 8
    return [(j * chunk, min(S, (j + 1) * chunk)) for j in range(8) if j * chunk < S]


def mem_rows(S: int, variant):
    """Text-memory rows one cross-attention reads (duplicates count twice) for a text of S keys."""
    rows = list(range(S))
    if variant is None or variant == "mem_other_layer":
        return rows
    if variant == "mem_drop_first":
        return rows[1:]
    if variant == "mem_drop_last":
        return rows[:-1]
    if variant == "mem_last_twice":
        return rows + [S - 1]
    if variant == "mem_drop_split":
        sp = mem_split_ranges(S)
        j0, j1 = sp[len(sp) // 2]
        return [r for r in rows if not (j0 <= r < j1)]
    if variant == "mem_one_more":
        return rows + [S]
    raise ValueError(variant)


def wrong_f(S: int, first: bool):
    """The wrong answers that mean something for a text of S keys.  Left out: mem_one_more on an engine's first utterance (row S
    holds nothing yet); at S = 1 the drop and split variants (no key would be left) and mem_last_twice (one key has softmax weight
    1 whatever its multiplicity, so the answer is identically the right one)."""
    out = [w for w in WRONG_F if not (first and w == "mem_one_more")]
    if S == 1:
        out = [w for w in out if w not in ("mem_drop_first", "mem_drop_last", "mem_drop_split", "mem_last_twice")]
    return out


class StepRefF(StepRef):
    """StepRef for a VALL-F engine (decoder layers, valle_oracle._DecLayer / OracleModelF); cache rows are audio rows only."""

    def __init__(self, sd, d: int, nhead: int, num_layers: int, norm_first: bool = True, add_prenet: bool = False,
                 prefix_mode: int = 0, prepend_bos: bool = False, bf16: bool = True, pe_rows: int = 4000):
        from valle_amd.weights import sine_table

        self.sd = engine_state_dict(sd, bf16)
        self.d, self.H, self.L = d, nhead, num_layers
        self.hd = d // nhead
        self.norm_first, self.add_prenet = norm_first, add_prenet
        self.pe = sine_table(pe_rows, d).double()
        self.layers = [vo._DecLayer(self.sd, f"ar_decoder.layers.{i}", False) for i in range(num_layers)]
        self.in_abs = [(L.in_w.abs(), L.in_b.abs()) for L in self.layers]
        self.cin_abs = [(L.cin_w[d:].abs(), L.cin_b[d:].abs()) for L in self.layers]
        self.head = self.sd["ar_predict_layer.weight"]
        self.head_abs = self.head.abs()
        self.oracle = vo.OracleModelF(self.sd, d, nhead, num_layers, prefix_mode=prefix_mode, prepend_bos=prepend_bos,
                                      num_quantizers=1, norm_first=norm_first, add_prenet=add_prenet)

    def _attend(self, q, K, V):
        """q (H, hd), K / V (H, n, hd) -> (d,)"""
        s = torch.einsum("hc,hnc->hn", q, K) / math.sqrt(self.hd)
        return torch.einsum("hn,hnc->hc", torch.softmax(s, dim=-1), V).reshape(self.d)

    def _ff(self, L, h):
        return F.relu(h @ L.w1.t() + L.b1) @ L.w2.t() + L.b2

    def forward(self, token: int, pos: int, kv: torch.Tensor, mem: torch.Tensor, t: int, S: int, variant=None,
                own_newest: bool = False):
        """One pass: ``token`` at audio position ``pos``, whose K / V the engine wrote into cache row ``t``.  kv: (L, 2, H, rows, hd)
        float64, the engine's cache; mem: (L, 2, H, max_text, hd) float64, the engine's text memory, of which the cross-attention
        reads rows 0..S-1.  ``variant``: None, one of WRONG_F, or a list of them: the list runs as one batch of rows and returns
        {name: logits}.  Otherwise returns StepRef.forward's dict.  own_newest: row t of ``kv`` is first filled with the
        reference's own K / V (in place), so that a run can stand on the reference's cache alone."""
        H, hd, d = self.H, self.hd, self.d
        many = isinstance(variant, (list, tuple))
        vs = list(variant) if many else [variant]
        s_rows = [torch.tensor(key_rows(t, v if v in WRONG else None, "plain")) for v in vs]
        m_rows = [torch.tensor(mem_rows(S, v if v in WRONG_MEM else None)) for v in vs]
        x = self.embed(token, pos)[None].repeat(len(vs), 1)
        out = {"k": [], "v": [], "k_abs": [], "v_abs": []}
        for li, L in enumerate(self.layers):
            h = vo.layer_norm(x, *L.n[0]) if self.norm_first else x
            qkv = (h @ L.in_w.t() + L.in_b).view(len(vs), 3, H, hd)
            if None in vs:
                i = vs.index(None)
                wa, ba = self.in_abs[li]
                _, ka, va = (wa @ h[i].abs() + ba).view(3, H, hd)
                out["k"].append(qkv[i, 1])
                out["v"].append(qkv[i, 2])
                out["k_abs"].append(ka)
                out["v_abs"].append(va)
                if own_newest:
                    kv[li, 0, :, t], kv[li, 1, :, t] = qkv[i, 1], qkv[i, 2]
            a = torch.stack([self._attend(qkv[i, 0], kv[li, 0][:, r], kv[li, 1][:, r]) for i, r in enumerate(s_rows)])
            x = x + a @ L.out_w.t() + L.out_b
            x = vo.layer_norm(x, *L.n[0]) if not self.norm_first else x
            h = vo.layer_norm(x, *L.n[1]) if self.norm_first else x
            q = (h @ L.cin_w[:d].t() + L.cin_b[:d]).view(len(vs), H, hd)
            a = []
            for i, r in enumerate(m_rows):
                lm = (li + 1) % self.L if vs[i] == "mem_other_layer" else li
                a.append(self._attend(q[i], mem[lm, 0][:, r], mem[lm, 1][:, r]))
            x = x + torch.stack(a) @ L.cout_w.t() + L.cout_b
            if self.norm_first:
                x = x + self._ff(L, vo.layer_norm(x, *L.n[2]))
            else:
                x = vo.layer_norm(x, *L.n[1])
                x = vo.layer_norm(x + self._ff(L, x), *L.n[2])
        hf = self.oracle.ar_final_norm(x)
        logits = hf @ self.head.t()
        if many:
            return {v: logits[i] for i, v in enumerate(vs)}
        out["logits"] = logits[0]
        out["head_abs"] = self.head_abs @ hf[0].abs()
        return out

    def memory_kv(self, text: torch.Tensor):
        """fp64 K and V of every layer's text memory from the embedded text (OracleModelF.ar_text: embedding, text prenet, alpha x
        the sine row).  Per layer (k, v, k_abs, v_abs), each (H, S, hd); *_abs = sum |w| |h| + |b| of the row."""
        x = self.oracle.ar_text(text).double()
        S, H, hd, d = text.shape[0], self.H, self.hd, self.d
        res = []
        for li, L in enumerate(self.layers):
            wa, ba = self.cin_abs[li]
            k, v = (x @ L.cin_w[d:].t() + L.cin_b[d:]).view(S, 2, H, hd).permute(1, 2, 0, 3)
            ka, va = (x.abs() @ wa.t() + ba).view(S, 2, H, hd).permute(1, 2, 0, 3)
            res.append((k, v, ka, va))
        return res

    def prefill_kv(self, text: torch.Tensor, yy: torch.Tensor):
        """fp64 forward of the audio prefix under the causal mask, every layer cross-attending to the fp64 memory of ``text``.
        Returns (per layer (k, v, k_abs, v_abs) as StepRef.prefill_kv, logits (1025,) of the last row = pass 0, head_abs)."""
        m = self.oracle
        A, H, hd = yy.shape[0], self.H, self.hd
        memx = m.ar_text(text).double()
        x = m.ar_audio(yy).double()
        mask = torch.triu(torch.ones(A, A, dtype=torch.bool), diagonal=1)
        res = []
        for li, L in enumerate(self.layers):
            h = vo.layer_norm(x, *L.n[0]) if self.norm_first else x
            wa, ba = self.in_abs[li]
            ab = (h.abs() @ wa.t() + ba).view(A, 3, H, hd).permute(1, 2, 0, 3)
            a, (k, v) = vo.self_attention(h, L.in_w, L.in_b, L.out_w, L.out_b, H, mask)
            res.append((k, v, ab[1], ab[2]))
            x = x + a
            x = vo.layer_norm(x, *L.n[0]) if not self.norm_first else x
            h = vo.layer_norm(x, *L.n[1]) if self.norm_first else x
            x = x + vo.cross_attention(h, memx, L.cin_w, L.cin_b, L.cout_w, L.cout_b, H)
            if self.norm_first:
                x = x + self._ff(L, vo.layer_norm(x, *L.n[2]))
            else:
                x = vo.layer_norm(x, *L.n[1])
                x = vo.layer_norm(x + self._ff(L, x), *L.n[2])
        hf = m.ar_final_norm(x[-1])
        return res, self.head @ hf, self.head_abs @ hf.abs()


# The cases and the utterance schedule of tests/test_gpu_vallf_step.py, shared with tests/test_vallf_step_ref_cpu.py
VALLF_CASES = {
    "f_bf16_d1024": dict(precision="bf16", d=1024, H=16),
    "f_fp32_d512": dict(precision="fp32", d=512, H=8),
    "f_bf16_hd32": dict(precision="bf16", d=256, H=8),
    "f_bf16_hd16": dict(precision="bf16", d=256, H=16),
    "f_fp32_hd8": dict(precision="fp32", d=128, H=16),
    "f_fp32_hd4": dict(precision="fp32", d=64, H=16),
    "f_bf16_postnorm": dict(precision="bf16", d=512, H=8, norm_first=False),
    "f_bf16_prenet": dict(precision="bf16", d=512, H=8, add_prenet=True),
}
VALLF_L = 2
VALLF_SEED = 11
VALLF_TEXT_LENS = (129, 5, 64, 65, 8, 9, 1, 47, 63)  # every shorter text after a longer one; empty splits; split and tile edges
VALLF_PROMPT_ROWS = (1, 63, 64, 65, 130)             # bos + P, cycled over the utterances: ragged and full 64-query tiles
VALLF_PASSES = 12
VALLF_MAX_TEXT, VALLF_MAX_AUDIO = 160, 160


def vallf_config(c):
    from valle_amd.config import ModelConfig

    return ModelConfig(model_name="VALL-F", decoder_dim=c["d"], nhead=c["H"], num_decoder_layers=VALLF_L, prefix_mode=1,
                       prepend_bos=True, num_quantizers=1, norm_first=c.get("norm_first", True),
                       add_prenet=c.get("add_prenet", False))


def vallf_inputs(c, seed: int, q_sharpen: float):
    """(state dict, utterances) of a case: synthetic weights with the q rows of every self-attention and cross-attention in_proj
    scaled by q_sharpen (both softmaxes peaked, a single key matters); utterances = [(text (S,), prompt (P,), forced (n,))] in
    the order of VALLF_TEXT_LENS, P = VALLF_PROMPT_ROWS[i % 5] - 1 (the engine prepends bos)."""
    from valle_amd.weights import synthetic_state_dict

    sd = synthetic_state_dict(vallf_config(c), seed)
    d = c["d"]
    for li in range(VALLF_L):
        sd[f"ar_decoder.layers.{li}.self_attn.in_proj_weight"][:d] *= q_sharpen
        sd[f"ar_decoder.layers.{li}.multihead_attn.in_proj_weight"][:d] *= q_sharpen
    g = torch.Generator().manual_seed(seed)
    utts = []
    for i, S in enumerate(VALLF_TEXT_LENS):
        P = VALLF_PROMPT_ROWS[i % len(VALLF_PROMPT_ROWS)] - 1
        utts.append((torch.randint(3, 100, (S,), generator=g), torch.randint(0, 1024, (P,), generator=g),
                     torch.randint(0, 1024, (VALLF_PASSES,), generator=g)))
    return sd, utts
