"""GPU: the Whisper token loop's kernels (whisper_kernels.hpp: wsp_skinny_gemm, wsp_decode_attn, wsp_head_reduce, wsp_embed) on caller
data, through the launchers the recogniser uses (vx_op_wsp_*, valle_amd.whisper.op_wsp_*), at the shapes the released checkpoints
run and the model-level cases of test_gpu_whisper.py cannot reach.  This file only compares: the cases, the fp64 references and the
floors are whisper_ops_cases.py's, and test_whisper_ops_cpu.py proves on the host that the exact cases are exact, that every launcher
rule is crossed and that every deliberate mistake is seen.

Exact cases (small integers, any order of summation gives the same fp32 bits): bitwise equality, no tolerance.  Real-valued cases:
yardstick fp64, floor the same operation in torch fp32 on the host, bound kernel max-abs error <= 4 x floor (the project's rule); err,
floor and ratio are printed before they are asserted and written to the file VX_WSP_OPS_PARITY_OUT names
(profiles/whisper_ops_parity.json comes from there).  Every output buffer sits between NaN guards that must survive.

1. skinny GEMM: cpw 8 / 16 / 64, one / two / three K chunks, 1 .. 8 row tiles with ragged last ones, bias, GELU, a residual aliased to
   the output; row m of an M = 64 call is bitwise the M = 1 call of that row;
2. decode attention, cross and self mode: a dominant key at 0, 255, 256, per - 1, per, T - 1 for T up to 4096, the uniform mean, eight
   utterances of different T in one launch; the appended row replaces the poison and nothing else in the cache changes;
3. the head for V = 101 .. 51865: ties, both suppress lists, forced tokens, every state transition in one batched call;
4. embed."""
import json
import os

import pytest
import torch

import whisper_ops_cases as OC
import whisper_ops_ref as OR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
_PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    yield
    out = os.environ.get("VX_WSP_OPS_PARITY_OUT")
    if out and _PARITY:
        with open(out, "w") as f:
            json.dump(_PARITY, f, indent=1, sort_keys=True)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _guarded(shape, fill=None):
    """A device tensor of `shape` between two NaN guards -> (the whole buffer, the view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _record(kind, name, err, floor):
    ratio = err / floor if floor else float("inf")
    print(f"{kind} {name}: kernel {err:.3e}, floor {floor:.3e}, ratio {ratio:.2f}")
    _PARITY.setdefault(kind, {})[name] = {"err": err, "floor": floor, "ratio": ratio}
    return ratio


# ---- 1. skinny GEMM -------------------------------------------------------------------------------------------------------------------
def _run_gemm(i, bias, res, act):
    from valle_amd.whisper import op_wsp_gemm

    M, N = i["x"].shape[0], i["W"].shape[0]
    buf, out = _guarded((M, N), i["res"] if res else None)  # the residual is aliased to the output
    op_wsp_gemm(i["x"].to(DEV), i["W"].to(DEV), i["bias"].to(DEV) if bias else None, out if res else None, out, act)
    torch.cuda.synchronize()
    assert _guards_intact(buf), "a write outside the output"
    return out.cpu()


@pytest.mark.parametrize("shape", OC.GEMM_EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_exact(shape):
    i = OC.gemm_exact_inputs(shape)
    for bias, res in OC.GEMM_EXACT_VARIANTS:
        got, want = _run_gemm(i, bias, res, OR.ACT_NONE), OC.gemm_exact_want(shape, bias, res).float()
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
        assert bad.numel() == 0, f"{shape} bias {bias} residual {res}: {bad.shape[0]} outputs differ, the first at {bad[0].tolist()}"


@pytest.mark.parametrize("name", list(OC.GEMM_REAL))
def test_gemm_real(name):
    M, N, K, act, res = OC.GEMM_REAL[name]
    got = _run_gemm(OC.gemm_real_inputs(name), True, res, act)
    assert bool(torch.isfinite(got).all())
    err, floor = float((got.double() - OC.gemm_real_want(name)).abs().max()), OC.gemm_real_floor(name)
    _record("gemm", name, err, floor)
    assert err <= OC.TOL_FACTOR * floor


def test_gemm_rows_are_bitwise_their_solo_call():
    """The ragged-batch property of the recogniser rests on this: a row's bits do not depend on the rows beside it."""
    from valle_amd.whisper import op_wsp_gemm

    name = OC.GEMM_SOLO_ROWS_CASE
    M, N, K, act, _ = OC.GEMM_REAL[name]
    i = OC.gemm_real_inputs(name)
    x, W, b = i["x"].to(DEV), i["W"].to(DEV), i["bias"].to(DEV)
    full = op_wsp_gemm(x, W, b, None, torch.empty(M, N, device=DEV), act)
    assert M == 64
    for m in range(M):
        solo = op_wsp_gemm(x[m:m + 1].contiguous(), W, b, None, torch.empty(1, N, device=DEV), act)
        assert _bits(solo[0], full[m]), f"row {m}"
    for m0, rows in ((0, 9), (7, 17), (55, 9)):  # ragged calls: the row lands in another tile and another slot
        part = op_wsp_gemm(x[m0:m0 + rows].contiguous(), W, b, None, torch.empty(rows, N, device=DEV), act)
        assert _bits(part, full[m0:m0 + rows]), (m0, rows)


# ---- 2. decode attention --------------------------------------------------------------------------------------------------------------
def _run_attn(i, Ts, rows_per_utt, max_keys):
    """One launch over a case's inputs.  The cache is laid out as the recogniser's: row = [keys of every head | values of every
    head], utterance u's rows at u rows_per_utt.  Returns the output (n, H, 64) and asserts that nothing but the appended rows of a
    self-attention step changes in the cache, guards included."""
    from valle_amd.whisper import op_wsp_decode_attn

    n, Tm = i["K"].shape[0], i["K"].shape[1]
    H, d = OC.ATTN_H, OC.ATTN_H * OC.HD
    self_mode = "knew" in i
    assert Tm <= rows_per_utt
    cache = torch.full((n, rows_per_utt, 2 * d), 7.5)  # rows past an utterance's keys: never read, never written
    cache[:, :Tm, :d], cache[:, :Tm, d:] = i["K"].reshape(n, Tm, d), i["V"].reshape(n, Tm, d)
    cbuf, cview = _guarded(tuple(cache.shape), cache)
    obuf, out = _guarded((n, d))
    before = cbuf.clone()
    ldq = 3 * d if self_mode else d
    qrow = torch.full((n, ldq), float("nan"))  # as the recogniser's q | k | v row
    qrow[:, :d] = i["q"].reshape(n, d)
    kv = cview.view(-1)
    if self_mode:
        qrow[:, d:2 * d], qrow[:, 2 * d:] = i["knew"].reshape(n, d), i["vnew"].reshape(n, d)
        qdev = qrow.to(DEV)
        # knew and vnew with the row stride of q: views of the same rows would not be contiguous, so they get rows of their own
        knew, vnew = torch.full((n, ldq), float("nan"), device=DEV), torch.full((n, ldq), float("nan"), device=DEV)
        knew[:, :d], vnew[:, :d] = i["knew"].reshape(n, d).to(DEV), i["vnew"].reshape(n, d).to(DEV)
        pos = torch.tensor([t - 1 for t in Ts], dtype=torch.int32, device=DEV)
        op_wsp_decode_attn(qdev, kv, kv[d:], out, 2 * d, H, rows_per_utt, max_keys, knew=knew, vnew=vnew, pos=pos)
    else:
        assert len(set(Ts)) == 1
        op_wsp_decode_attn(qrow.to(DEV), kv, kv[d:], out, 2 * d, H, rows_per_utt, max_keys, keys=Ts[0])
    torch.cuda.synchronize()
    assert _guards_intact(obuf), "a write outside the output"
    expect = before[GUARD:-GUARD].view(n, rows_per_utt, 2 * d).clone()
    if self_mode:
        for u, t in enumerate(Ts):
            expect[u, t - 1, :d], expect[u, t - 1, d:] = i["knew"][u].reshape(d).to(DEV), i["vnew"][u].reshape(d).to(DEV)
    assert _guards_intact(cbuf) and _bits(cview, expect), "the cache changed outside the appended rows, or the appended row is wrong"
    return out.cpu().view(n, H, OC.HD)


@pytest.mark.parametrize("self_mode", (False, True), ids=("cross", "self"))
@pytest.mark.parametrize("T", OC.ATTN_DOMINANT_T)
def test_attention_dominant_key(T, self_mode):
    i = OC.attn_dominant_inputs(T, self_mode)
    n = i["q"].shape[0]
    got = _run_attn(i, (T,) * n, min(T + 3, OR.MAX_KEYS), T)  # max_keys = T: the partial outputs end where the LDS ends
    for u in range(n):
        for h in range(OC.ATTN_H):
            assert _bits(got[u, h], i["want"][u, h]), f"T {T}, dominant key {int(i['dom'][u, h])} (utterance {u}, head {h})"


@pytest.mark.parametrize("self_mode", (False, True), ids=("cross", "self"))
@pytest.mark.parametrize("T", OC.ATTN_UNIFORM_T)
def test_attention_uniform_mean(T, self_mode):
    i = OC.attn_uniform_inputs(T, self_mode)
    got = _run_attn(i, (T,) * i["q"].shape[0], T, OR.MAX_KEYS)
    assert _bits(got, i["want"])


@pytest.mark.parametrize("name", list(OC.ATTN_REAL))
def test_attention_real(name):
    i = OC.attn_real_inputs(name)
    Tm = max(i["T"])
    got = _run_attn(i, i["T"], Tm, Tm)
    assert bool(torch.isfinite(got).all())
    err, floor = float((got.double() - OC.attn_real_want(name)).abs().max()), OC.attn_real_floor(name)
    _record("attention", name, err, floor)
    assert err <= OC.TOL_FACTOR * floor


# ---- 3. the head ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", (False, True), ids=("greedy", "forced"))
@pytest.mark.parametrize("V", OC.HEAD_V)
def test_head(V, forced):
    from valle_amd.whisper import op_wsp_head

    c, want = OC.head_case(V), OC.head_want(V, forced)
    n, S = len(c["rows"]), OC.HEAD_OUT_STRIDE
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    state = [i32([s[k] for s in c["state"]]) for k in ("cur", "pos", "count", "finished")]
    tok = torch.full((n, S), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((n, S), float("nan"), dtype=torch.float32, device=DEV)
    cnt, stop = torch.full((n,), -7, dtype=torch.int32, device=DEV), torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lbuf, logits = _guarded((n, V), c["logits"])
    op_wsp_head(logits, torch.tensor(c["smap"], dtype=torch.uint8, device=DEV), i32(c["prompt"]), i32([s["n_prompt"] for s in c["state"]]),
                i32([s["max_new"] for s in c["state"]]), i32(OC.head_forced(c)) if forced else None, state, (tok, lp, cnt, stop), c["eos"],
                c["max_target"])
    torch.cuda.synchronize()
    assert _bits(logits.cpu(), c["logits"]) and _guards_intact(lbuf)
    state = [s.cpu().tolist() for s in state]
    tok, lp, cnt, stop = tok.cpu(), lp.cpu(), cnt.cpu().tolist(), stop.cpu().tolist()
    for u, what in enumerate(c["rows"]):
        st, out = want[u]
        assert dict(cur=state[0][u], pos=state[1][u], count=state[2][u], finished=state[3][u]) == st, (what, st)
        written = [] if out is None else [out["g"]]
        for g in range(S):
            if g not in written:
                assert int(tok[u, g]) == -7 and bool(torch.isnan(lp[u, g])), f"{what}: slot {g} was written"
        if out is None:  # inside the prompt, or finished before: no output at all
            assert cnt[u] == -7 and stop[u] == -7, what
            continue
        g, v = out["g"], out["logprob"]
        assert int(tok[u, g]) == out["token"], (what, int(tok[u, g]), out["token"])
        assert cnt[u] == g + 1 and stop[u] == out["stop"], (what, cnt[u], stop[u], out)
        got = float(lp[u, g])
        assert got == v if v == float("-inf") else abs(got - v) <= OC.LOGPROB_REL * max(1.0, abs(v)), (what, got, v)


# ---- 4. embed -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", OC.EMBED_D)
def test_embed(d):
    from valle_amd.whisper import op_wsp_embed

    i = OC.embed_inputs(d)
    got = op_wsp_embed(i["tok"].to(DEV), i["pos_table"].to(DEV), i["cur"].to(DEV), i["pos"].to(DEV))
    assert _bits(got.cpu(), OR.embed(i["tok"], i["pos_table"], i["cur"], i["pos"]))
