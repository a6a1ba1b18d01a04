"""fp64 restatement of scoring (vx_score, vx_op_nll_rows): the per-row terms of the reference's validation numbers
(VALLE.forward: F.cross_entropy and MulticlassAccuracy(top_k), valle.py:827-881 for the AR decoder, 886-950 for a NAR stage),
teacher-forced on the inference prompt layout, built from the oracle's own pieces (oracle/valle_oracle.py, imported, not changed).

    nll_rank_argmax(logits, targets)      one logits matrix -> (nll fp64, rank, argmax)
    oracle(cfg, sd, dtype)                OracleModel / OracleModelF on the state_dict cast to dtype (fp64: the reference of the
                                          tests; fp32: what the margin rule measures the reference's own rounding with)
    score_logits(m, text, codes, P)       (AR logits (T+1, 1025), [NAR stage logits (T, 1024)] * (Q-1))
    score(m, text, codes, P)              dict of per-row results + the logits
    decided(logits, targets, tol)         rows whose rank cannot change under a logits error of tol per entry
"""
import torch
import torch.nn.functional as F

from oracle import valle_oracle as vo

EOS = vo.NUM_AUDIO_TOKENS  # 1024


def nll_rank_argmax(logits: torch.Tensor, targets: torch.Tensor):
    """logits (rows, V) of any float type, targets (rows,) int64 in [0, V) -> nll (rows,) fp64 = logsumexp(row) - row[target]
    (a -inf target entry gives +inf), rank (rows,) int64 = entries strictly greater than the target's (ties count for the
    target), argmax (rows,) int64 = first index of the maximum.  Comparisons run on the values as given (exact in fp64)."""
    lg = logits.double()
    tv = lg.gather(1, targets.reshape(-1, 1))
    m = lg.amax(1, keepdim=True)
    lse = m + torch.log(torch.exp(lg - m).sum(1, keepdim=True))  # exp(-inf) = 0
    nll = torch.where(torch.isinf(tv) & (tv < 0), torch.full_like(tv, float("inf")), lse - tv)[:, 0]
    rank = (lg > tv).sum(1)
    argmax = (lg == m).int().argmax(1)  # first True
    return nll, rank, argmax


def decided(logits: torch.Tensor, targets: torch.Tensor, tol) -> torch.Tensor:
    """(rows,) bool: the margin rule of test_gpu_engine.py's teacher-forced tests, stated for a rank instead of an argmax: with
    every logit off by at most tol (a number or a (rows,) tensor), an entry can move across the target's value only if it lies
    within 2 tol of it.  True where no other entry does, so the rank (and, at rank 0, the argmax) is fixed."""
    lg = logits.double()
    gap = (lg - lg.gather(1, targets.reshape(-1, 1))).abs()
    gap.scatter_(1, targets.reshape(-1, 1), float("inf"))
    tol = torch.as_tensor(tol, dtype=torch.float64)
    return gap.amin(1) > 2 * tol


def oracle(cfg, sd, dtype=torch.float64):
    """The oracle model of a ModelConfig on the state_dict cast to dtype (integer tensors stay)."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    kw = dict(prefix_mode=cfg.prefix_mode, prepend_bos=cfg.prepend_bos, num_quantizers=cfg.num_quantizers,
              nar_scale_factor=cfg.scale_factor, norm_first=cfg.norm_first, add_prenet=cfg.add_prenet)
    cls = vo.OracleModelF if cfg.is_vallf else vo.OracleModel
    return cls(sd, cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers, **kw)


def _dtype(m):
    return m.sd["ar_predict_layer.weight"].dtype


@torch.no_grad()
def ar_score_logits(m, text: torch.Tensor, codes: torch.Tensor, P: int) -> torch.Tensor:
    """(T+1, 1025): the logits of the rows that predict codes[P, 0] ... codes[A-1, 0], EOS, from ONE pass over
    [text | (BOS) codes[:, 0]] under the reference mask (valle.py:863-877; VALL-F: text as memory, valle.py:598-632)."""
    bos = int(m.prepend_bos)
    yy = codes[:, 0]
    if bos:
        yy = F.pad(yy, (1, 0), value=EOS + 1)  # valle.py:1006-1007
    first = P if bos else P - 1
    assert first >= 0, "P = 0 needs prepend_bos"
    T = codes.shape[0] - P
    S = text.shape[0]
    if isinstance(m, vo.OracleModelF):
        h = m.ar_stack(m.ar_audio(yy), m.ar_text(text), torch.zeros(S, dtype=torch.bool))
    else:
        h = m.ar_stack(torch.cat([m.ar_text(text), m.ar_audio(yy)], 0), vo.ar_mask(S, yy.shape[0]))[S:]
    return m.ar_logits(h[first : first + T + 1])


@torch.no_grad()
def nar_score_logits(m, text_nar: torch.Tensor, codes: torch.Tensor, P: int):
    """[(T, 1024)] * (Q-1): OracleModel.nar / OracleModelF.nar (valle.py:1063-1134 / 650-708) with every stage fed the GIVEN
    codes of the earlier stages instead of its own argmax (what vx_nar_ex's forced_codes does); text_nar is already trimmed."""
    sd, Q = m.sd, m.Q
    vf = isinstance(m, vo.OracleModelF)
    emb = lambda j: sd[f"nar_audio_embeddings.{j}.word_embeddings.weight"]
    prompts, S = codes[:P], text_nar.shape[0]
    y_emb = F.embedding(codes[:, 0], emb(0)).clone()
    x = F.embedding(text_nar, sd["nar_text_embedding.word_embeddings.weight"])
    if m.add_prenet:
        x = vo.text_prenet(sd, "nar_text_prenet", x)
    x = vo.add_position(x, sd["nar_text_position.alpha"])
    if m.prefix_mode != 0:
        for j in range(1, Q):
            y_emb[:P] += F.embedding(prompts[:, j], emb(j))
    out = []
    for i in range(Q - 1):
        y_pos = vo.audio_prenet(sd, "nar_audio_prenet", y_emb) if m.add_prenet else y_emb
        y_pos = vo.add_position(y_pos, sd["nar_audio_position.alpha"])
        h = m.nar_stack(y_pos, x, i)[P:] if vf else m.nar_stack(torch.cat([x, y_pos], 0), i)[S + P:]
        out.append(F.linear(h, sd[f"nar_predict_layers.{i}.weight"]))
        if i < Q - 2:
            if m.prefix_mode == 0:
                y_emb[:P] += F.embedding(prompts[:, i + 1], emb(i + 1))
            y_emb[P:] += F.embedding(codes[P:, i + 1], emb(i + 1))
    return out


def score(m, text: torch.Tensor, codes: torch.Tensor, P: int, text_nar=None, ar: bool = True, nar: bool = True) -> dict:
    """The whole score of one utterance on oracle model m: ar_logits / ar_targets / ar_nll / ar_rank / ar_argmax and, for Q > 1,
    nar_logits (Q-1, T, 1024) / nar_targets (Q-1, T) / nar_nll / nar_rank / nar_argmax."""
    r = {}
    if ar:
        lg = ar_score_logits(m, text, codes, P)
        tg = torch.cat([codes[P:, 0], torch.tensor([EOS])])
        nll, rank, am = nll_rank_argmax(lg, tg)
        r.update(ar_logits=lg, ar_targets=tg, ar_nll=nll, ar_rank=rank, ar_argmax=am)
    if nar and m.Q > 1:
        lgs = nar_score_logits(m, text if text_nar is None else text_nar, codes, P)
        tg = codes[P:, 1:].t().contiguous()
        res = [nll_rank_argmax(l, t) for l, t in zip(lgs, tg)]
        r.update(nar_logits=torch.stack(lgs), nar_targets=tg, nar_nll=torch.stack([a[0] for a in res]),
                 nar_rank=torch.stack([a[1] for a in res]), nar_argmax=torch.stack([a[2] for a in res]))
    return r
