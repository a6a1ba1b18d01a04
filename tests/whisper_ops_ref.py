"""Plain torch restatements of the Whisper token loop's kernels (whisper_kernels.hpp: wsp_skinny_gemm, wsp_decode_attn,
wsp_head_reduce, wsp_embed) at a given dtype, the launcher's rules (whisper.hip: launch_skinny, launch_decode_attn) restated in
Python, and the deliberate mistakes test_whisper_ops_cpu.py applies.  Nothing here knows how the kernels sum."""
import math

import torch
import torch.nn.functional as F

import whisper_ref as R

SK_MT, SK_KC, MAX_KEYS, STRIDE = 8, 2048, 4096, 256  # WSP_SK_MT, WSP_SK_KC, WSP_MAX_KEYS, the workgroup's 256 threads
ACT_NONE, ACT_GELU = 0, 1
SUPPRESS, BEGIN_SUPPRESS = 1, 2

GEMM_MUTATIONS = ("last_chunk_dropped", "chunk0_reused", "column_clip_off_by_one", "row8_from_row0")
ATTN_MUTATIONS = ("key256_skipped", "stale_cache_row", "quarter_off_by_one")
HEAD_MUTATIONS = ("higher_index_on_tie", "begin_suppress_always", "lse_over_suppressed")


# ---- the launcher's rules -----------------------------------------------------------------------------------------------------------
def cpw(N):
    """Columns per workgroup of wsp_skinny_gemm, as launch_skinny chooses them."""
    return min(64, max(8, N // 512 // 8 * 8))


def chunks(K):
    return -(-K // SK_KC)


def row_tiles(M):
    return -(-M // SK_MT)


def lds_bytes(K):
    return SK_MT * min(K, SK_KC) * 4


def per_quarter(T):
    """Keys per wave of wsp_decode_attn's second phase."""
    return (T + 3) // 4


# ---- the skinny GEMM ----------------------------------------------------------------------------------------------------------------
def gemm(x, W, bias, res, act, dtype, mut=()):
    """act(x W^T + bias) + res at `dtype`: F.linear, the exact (erf) GELU."""
    x, W = x.to(dtype), W.to(dtype)
    M, K = x.shape
    N = W.shape[0]
    if "last_chunk_dropped" in mut:
        keep = (chunks(K) - 1) * SK_KC
        x, W = x[:, :keep], W[:, :keep]
    if "chunk0_reused" in mut:  # the second chunk's activations are the first chunk's
        kn = min(K, 2 * SK_KC) - SK_KC
        x = x.clone()
        x[:, SK_KC:SK_KC + kn] = x[:, :kn]
    if "row8_from_row0" in mut:
        x = x.clone()
        x[8] = x[0]
    y = F.linear(x, W, None if bias is None else bias.to(dtype))
    if act == ACT_GELU:
        y = F.gelu(y)
    if res is not None:
        y = y + res.to(dtype)
    if "column_clip_off_by_one" in mut:  # the last column of every workgroup is never stored: what was in `out` stays (zeros here)
        y = y.clone()
        y[:, cpw(N) - 1::cpw(N)] = 0.0 if res is None else res.to(dtype)[:, cpw(N) - 1::cpw(N)]
    return y


# ---- decode attention ---------------------------------------------------------------------------------------------------------------
def attn(q, K, V, dtype, knew=None, vnew=None, mut=()):
    """One (utterance, head): q (64), K and V (T, 64) -> (64).  With knew / vnew the last key and value are the step's own (K[-1] and
    V[-1] hold what the cache row held before)."""
    q, K, V = q.to(dtype), K.to(dtype).clone(), V.to(dtype).clone()
    T = K.shape[0]
    if knew is not None and "stale_cache_row" not in mut:
        K[T - 1], V[T - 1] = knew.to(dtype), vnew.to(dtype)
    p = torch.softmax((K @ q) * 0.125, dim=0)
    if "key256_skipped" in mut and T > 256:
        s = (K @ q) * 0.125
        s[256] = float("-inf")
        p = torch.softmax(s, dim=0)
    if "quarter_off_by_one" in mut and T > 1:  # the last key of the first quarter falls between two waves
        p = p.clone()
        p[per_quarter(T) - 1] = 0.0
    return p @ V


# ---- the head -----------------------------------------------------------------------------------------------------------------------
def suppress_lists(smap):
    return [i for i, b in enumerate(smap) if b & SUPPRESS], [i for i, b in enumerate(smap) if b & BEGIN_SUPPRESS]


def head_step(row, smap, prompt, n_prompt, max_new, forced, state, eos, max_target, mut=()):
    """One utterance's step as include/vallex.h states it.  state = dict(cur, pos, count, finished) -> (new state, None or
    dict(g, token, logprob, stop))."""
    st = dict(state)
    if st["finished"]:
        return st, None
    pos = st["pos"]
    if pos + 1 < n_prompt:
        st["cur"], st["pos"] = prompt[pos + 1], pos + 1
        return st, None
    g = pos + 1 - n_prompt
    sup, beg = suppress_lists(smap)
    f = None if forced is None else forced[g]
    rmut = tuple(m for m in mut if m == "begin_suppress_always")
    tok, lp, _ = R.step_outputs(row, g, sup, beg, forced=f, mut=rmut)
    proc = R.process_row(row.double(), g, sup, beg, rmut)
    if "higher_index_on_tie" in mut and f is None:
        tok = int((proc == proc.max()).nonzero()[-1])
        lp = float(proc[tok]) - (float(proc.max()) + math.log(float(torch.exp(proc - proc.max()).sum())))
    if "lse_over_suppressed" in mut:
        top = float(proc.max())
        lp = float(proc[tok]) - (top + math.log(float(torch.exp(row.double() - top).sum())))
    st["count"] = g + 1
    if forced is None and tok == eos:
        stop = R.STOP_EOS
    elif g + 1 >= max_new:
        stop = R.STOP_MAX_NEW
    elif pos + 2 >= max_target:
        stop = R.STOP_MAX_TARGET
    else:
        stop = 0
    if stop:
        st["finished"] = 1
    else:
        st["cur"], st["pos"] = tok, pos + 1
    return st, dict(g=g, token=tok, logprob=lp, stop=stop)


def embed(tok_emb, pos_emb, cur, pos):
    return tok_emb[cur.long()] + pos_emb[pos.long()]
