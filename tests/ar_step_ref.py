"""fp64 reference of one batch-1 AR decode pass (vall-e_amd/csrc/engine.hip enqueue_ar_step / enqueue_ar_step_tp), for
tests/test_gpu_ar_step.py.

The operands are the values the engine stores: on bf16 engines the matrices vx_set_weight converts (in_proj, out_proj, linear1,
linear2, ar_predict_layer) are rounded to bf16, everything else (embeddings, biases, norms, prenets, the fp32 sine table) stays
fp32; then every operation runs in float64.  Attention reads the ENGINE's own cache rows 0..t, row t (the newest key) included,
so that errors cannot compound from pass to pass and the check does not depend on how the cache was rounded.

``StepRef.forward`` also computes the nearest wrong answers the same way: one key fewer (the oldest or the newest row dropped),
the newest key counted twice, row t - 1 in place of row t, and one kernel split's key range dropped."""
import math

import torch
import torch.nn.functional as F

from oracle import valle_oracle as vo

U32 = 2.0 ** -24  # unit roundoff of fp32
U16 = 2.0 ** -8   # unit roundoff of bf16

WRONG = ("drop_oldest", "drop_newest", "newest_twice", "stale_newest", "drop_split")


def is_matrix_key(k: str) -> bool:
    """The keys vx_set_weight stores in bf16 on bf16 engines (engine.hip is_matrix_key)."""
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
