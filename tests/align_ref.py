"""fp64 restatement of alignment (vx_align, vx_op_attn_text_rows, vx_op_mono_path), built from the oracle's own pieces
(oracle/valle_oracle.py, imported, not changed), as score_ref.py is for scoring.

    text_attention(m, text, codes, P)   per layer and head, the softmax probability the row that predicts frame P + i puts on
                                        every text token: (L, H, T, S), and the row's largest |score|: (L, H, T)
    head_map(q, k, ...)                 the same quantity for one attention on given q / k (the kernel tests)
    mono_path(a)                        best monotonic path through a (T, Sw) map: (path or None, score)
    path_score(a, path)                 sum_t log(max(a[t, path[t]], FLT_MIN))

What is restated is what the reference's attention module returns with need_weights=True (valle/modules/activation.py:205-251 ->
F.multi_head_attention_forward): softmax(q k^T / sqrt(hd) + mask) per head; test_align_cpu.py holds it against that call."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import valle_oracle as vo

import score_ref as sr

FLT_MIN = float(np.finfo(np.float32).tiny)


def _probs(q, k, nhead, masked):
    """q (N, d), k (M, d), masked (N, M) bool or None -> (softmax probabilities (H, N, M), largest |score| per row (H, N)); the
    largest |score| is taken over the keys the row may see."""
    N, d = q.shape
    hd = d // nhead
    qh = q.reshape(N, nhead, hd).transpose(0, 1)
    kh = k.reshape(k.shape[0], nhead, hd).transpose(0, 1)
    s = qh @ kh.transpose(1, 2) / (hd ** 0.5)
    mag = s.abs()
    if masked is not None:
        s = s.masked_fill(masked, float("-inf"))
        mag = mag.masked_fill(masked, 0.0)
    return torch.softmax(s, -1), mag.amax(-1)


@torch.no_grad()
def text_attention(m, text: torch.Tensor, codes: torch.Tensor, P: int):
    """m: an oracle model (score_ref.oracle).  Returns (probs (L, H, T, S), smax (L, H, T)), T = A - P: for row i, the input row
    that predicts frame P + i (vx_score's layout, the EOS row left out).  q / k are recomputed from each layer's input - the norm
    first for pre-norm, the input as it is for post-norm - and the stack advances with the oracle's own layer functions."""
    bos = int(m.prepend_bos)
    yy = codes[:, 0]
    if bos:
        yy = F.pad(yy, (1, 0), value=sr.EOS + 1)
    first = P if bos else P - 1
    assert first >= 0, "P = 0 needs prepend_bos"
    T, S, d, H = codes.shape[0] - P, text.shape[0], m.d, m.nhead
    probs, smax = [], []
    if isinstance(m, vo.OracleModelF):
        A = yy.shape[0]
        x, mem = m.ar_audio(yy), m.ar_text(text)
        tgt_mask = torch.triu(torch.ones(A, A, dtype=torch.bool), diagonal=1)
        mem_pad = torch.zeros(S, dtype=torch.bool)
        for L in m.ar_layers:
            if m.norm_first:  # transformer.py:536-546: the cross-attention block reads norm2 of x after the self-attention block
                x1 = x + vo.self_attention(L.norm(0, x, None), L.in_w, L.in_b, L.out_w, L.out_b, H, tgt_mask)[0]
                qin = L.norm(1, x1, None)
            else:             # 547-560: x is normalised after the self-attention block and goes in as it is
                qin = L.norm(0, x + vo.self_attention(x, L.in_w, L.in_b, L.out_w, L.out_b, H, tgt_mask)[0], None)
            q = F.linear(qin, L.cin_w[:d], L.cin_b[:d])
            k = F.linear(mem, L.cin_w[d : 2 * d], L.cin_b[d : 2 * d])
            p, mg = _probs(q[first : first + T], k, H, None)
            probs.append(p)
            smax.append(mg)
            x = vo.decoder_layer(L, x, mem, H, tgt_mask, mem_pad, None, m.norm_first)
    else:
        x = torch.cat([m.ar_text(text), m.ar_audio(yy)], 0)
        mask = vo.ar_mask(S, yy.shape[0])
        rows = slice(S + first, S + first + T)
        for L in m.ar_layers:
            inp = L.norm(0, x, None) if m.norm_first else x
            qkv = F.linear(inp, L.in_w, L.in_b)
            p, mg = _probs(qkv[rows, :d], qkv[:, d : 2 * d], H, mask[rows])
            probs.append(p[:, :, :S])
            smax.append(mg)
            x, _ = vo.encoder_layer(L, x, H, mask, None, m.norm_first)
    return torch.stack(probs), torch.stack(smax)


def head_map(q, k, text_len: int, causal: bool, row0: int = 0):
    """One attention on given operands, in their own dtype promoted as given: q (H, rows, hd), k (H, keys, hd) -> probabilities
    (H, rows, text_len).  causal: row i sees keys [0, text_len + row0 + i + 1); else all `text_len` keys (k holds exactly them)."""
    H, rows, hd = q.shape
    s = q @ k.transpose(1, 2) / (hd ** 0.5)
    if causal:
        j = torch.arange(k.shape[1])[None, :]
        lim = (text_len + row0 + torch.arange(rows) + 1)[:, None]
        s = s.masked_fill((j >= lim)[None], float("-inf"))
    else:
        assert k.shape[1] == text_len
    return torch.softmax(s, -1)[:, :, :text_len]


def mono_path(a):
    """The best monotonic path through a (T, Sw): j(0) = 0, j(T-1) = Sw - 1, j(t+1) - j(t) in {0, 1}, maximal
    sum_t log(max(a[t, j(t)], FLT_MIN)), in numpy fp64; on equal predecessors the path stays in its column.  Returns (path
    (T,) int64, score), or (None, -inf) when T < Sw."""
    a = np.asarray(a, dtype=np.float64)
    T, Sw = a.shape
    if T < Sw:
        return None, float("-inf")
    la = np.log(np.maximum(a, FLT_MIN))
    D = np.full(Sw, -np.inf)
    D[0] = la[0, 0]
    bp = np.zeros((T, Sw), dtype=np.uint8)
    for t in range(1, T):
        adv = np.concatenate([[-np.inf], D[:-1]])
        mv = adv > D
        bp[t] = mv
        D = np.where(mv, adv, D) + la[t]
    path = np.empty(T, dtype=np.int64)
    j = Sw - 1
    for t in range(T - 1, 0, -1):
        path[t] = j
        j -= int(bp[t, j])
    path[0] = j
    return path, float(D[Sw - 1])


def path_score(a, path) -> float:
    a = np.asarray(a, dtype=np.float64)
    path = np.asarray(path, dtype=np.int64)
    return float(np.log(np.maximum(a[np.arange(a.shape[0]), path], FLT_MIN)).sum())


def valid_path(path, T: int, Sw: int) -> bool:
    path = np.asarray(path, dtype=np.int64)
    step = np.diff(path)
    return path.shape == (T,) and path[0] == 0 and path[-1] == Sw - 1 and bool(((step == 0) | (step == 1)).all())
