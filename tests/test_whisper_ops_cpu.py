"""No GPU: what test_gpu_whisper_ops.py stands on (the cases of whisper_ops_cases.py, the references of whisper_ops_ref.py).

1. the launcher's rules restated in whisper_ops_ref are the ones written in whisper.hip and whisper_kernels.hpp, and the case list
   crosses every one of them: cpw 8, 16 and 64, one chunk of exactly 64 KiB, a short last chunk, three chunks, more than one row tile
   and ragged ones, more than 256 keys, the 4096-key ceiling, more than 256 logits;
2. the torch fp32 evaluation of every case passes what the GPU test asks of the kernel: bitwise equality on the exact cases (with the
   K axis reversed too: their bits do not depend on the order of the sum), tokens, stops and log-probabilities on the head;
3. every real-valued floor is taken over at least 4096 (GEMM) / 1024 (attention) outputs;
4. each deliberate mistake moves every real-valued case it applies to by at least 10 x the GPU bound and breaks equality on every
   exact case it applies to;
5. the new entries refuse what the header says they refuse, before any HIP call."""
import ctypes as C
import os
import re

import pytest
import torch

import whisper_ops_cases as OC
import whisper_ops_ref as OR
import whisper_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vall-e_amd", "csrc")


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. rules and edges -----------------------------------------------------------------------------------------------------------
def test_rules_are_the_source_ones():
    hip, hpp = open(os.path.join(CSRC, "whisper.hip")).read(), open(os.path.join(CSRC, "whisper_kernels.hpp")).read()
    assert hip.count("a.cpw = std::min(64, std::max(8, a.N / 512 / 8 * 8));") == 1 and hip.count("cpw =") == 1  # one rule, one place
    assert hip.count("wsp_skinny_gemm<<<") == 1 and hip.count("wsp_decode_attn<<<") == 1                          # one launch each
    assert "(size_t)WSP_SK_MT * kc * sizeof(float)" in hip and "const int kc = std::min(a.K, WSP_SK_KC);" in hip
    for name, val in (("WSP_SK_MT", OR.SK_MT), ("WSP_SK_KC", OR.SK_KC), ("WSP_MAX_KEYS", OR.MAX_KEYS)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", hpp).group(1)) == val
    assert "for (int j = tid; j < T; j += 256)" in hpp and "for (int c = tid; c < a.V; c += 256)" in hpp and "per = (T + 3) / 4" in hpp
    assert OR.STRIDE == 256
    for N, want in ((24, 8), (1023, 8), (1024, 8), (4095, 8), (8191, 8), (8192, 16), (8200, 16), (32773, 64), (51865, 64), (51866, 64)):
        assert OR.cpw(N) == want, N


def test_every_edge_is_crossed():
    exact = OC.GEMM_EXACT_SHAPES
    real = [v[:3] for v in OC.GEMM_REAL.values()]
    for shapes in (exact, exact + tuple(real)):
        assert {OR.cpw(N) for _, N, _ in shapes} == {8, 16, 64}
    assert any(OR.cpw(N) == 16 and OR.chunks(K) > 1 and OR.row_tiles(M) > 1 and M % 8 for M, N, K in exact)  # multi-pass, multi-chunk, ragged rows
    assert any(OR.cpw(N) == 64 and N % 2 == 1 and N % 64 for M, N, K in exact)                                  # odd N, ragged last workgroup
    for shapes in (exact, real):
        assert any(OR.chunks(K) == 1 and OR.lds_bytes(K) == 65536 for _, _, K in shapes)  # exactly 64 KiB of LDS
        assert any(OR.chunks(K) == 2 and K % OR.SK_KC for _, _, K in shapes)            # a short second chunk
        assert any(OR.chunks(K) == 3 and K % OR.SK_KC for _, _, K in shapes)            # a short last chunk after two full ones
        assert any(OR.chunks(K) >= 2 for _, _, K in shapes)
        assert any(OR.row_tiles(M) > 1 and M % OR.SK_MT for M, _, _ in shapes) and any(M == 64 for M, _, _ in shapes)
    assert any(M == 9 for M, _, _ in exact) and any(M == 17 for M, _, _ in exact) and any(M == 1 for M, _, _ in exact)
    assert (9, 51865, 384) in real and all(K % 4 == 0 and M <= 64 for M, _, K in list(exact) + real)
    # attention: the second stride, quarters above 64 keys a wave, the ceiling
    assert max(OC.ATTN_DOMINANT_T) == OR.MAX_KEYS == max(OC.ATTN_UNIFORM_T)
    for Ts in (OC.ATTN_DOMINANT_T, OC.ATTN_SELF_T, OC.ATTN_CROSS_KEYS):
        assert any(T > OR.STRIDE for T in Ts) and (OR.STRIDE + 1) in Ts
    assert {255, 256, 257} <= set(OC.ATTN_SELF_T) and 1 in OC.ATTN_SELF_T and 1 in OC.ATTN_DOMINANT_T
    for T in OC.ATTN_DOMINANT_T:
        places, per = OC.dominant_places(T), OR.per_quarter(T)
        assert 0 in places and T - 1 in places and (T <= 256 or {255, 256} <= set(places)) and (per >= T or {per - 1, per} <= set(places))
    # the head: one logit a thread at most, exactly 256, the second stride, many strides
    assert {255, 256, 257} <= set(OC.HEAD_V) and min(OC.HEAD_V) < 256 and max(OC.HEAD_V) == 51865
    for V in OC.HEAD_V:
        rows = OC.head_case(V)["rows"]
        assert len(rows) == len(set(rows)) and {"tie_in_stride", "tie_across_threads", "max_suppressed", "begin_suppressed_g0", "begin_suppressed_g1",
                                               "in_prompt", "eos", "max_new_cap", "max_target_cap", "finished"} <= set(rows)
    assert any(d > OR.STRIDE and d % OR.STRIDE for d in OC.EMBED_D)


# ---- 2. the fp32 reference passes the GPU checks -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OC.GEMM_EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_exact_cases_are_exact(shape):
    M, N, K = shape
    i = OC.gemm_exact_inputs(shape)
    for t, lim in ((i["x"], 4), (i["W"], 8), (i["bias"], 16), (i["res"], 16)):
        assert bool((t == t.round()).all()) and float(t.abs().max()) <= lim
    assert 4 * 8 * K + 32 < 2 ** 24  # the largest partial sum of any order, bias and residual included
    for bias, res in OC.GEMM_EXACT_VARIANTS:
        want = OC.gemm_exact_want(shape, bias, res)
        f32 = OC.gemm_exact_want(shape, bias, res, torch.float32)
        assert bool((want == want.round()).all()) and float(want.abs().max()) < 2 ** 24
        assert _bits(f32, want.float()) and torch.equal(f32.double(), want)
        rev = OR.gemm(i["x"].flip(1), i["W"].flip(1), i["bias"] if bias else None, i["res"] if res else None, OR.ACT_NONE, torch.float32)
        assert _bits(rev, f32), "the bits depend on the order of the sum"


@pytest.mark.parametrize("name", list(OC.GEMM_REAL))
def test_gemm_real_cases(name):
    M, N, K, act, res = OC.GEMM_REAL[name]
    want, f32, floor = OC.gemm_real_want(name), OC.gemm_real_want(name, torch.float32), OC.gemm_real_floor(name)
    print(f"{name}: {want.numel()} outputs, max |value| {float(want.abs().max()):.3f}, floor {floor:.3e}")
    assert want.numel() >= 4096 and bool(torch.isfinite(want).all()) and 0.0 < floor < 1e-4
    assert float((f32.double() - want).abs().max()) <= OC.TOL_FACTOR * floor
    assert float(want.std()) > 0.3  # alive after the activation


@pytest.mark.parametrize("self_mode", (False, True), ids=("cross", "self"))
def test_attention_exact_cases_are_exact(self_mode):
    for T in OC.ATTN_DOMINANT_T:
        i = OC.attn_dominant_inputs(T, self_mode)
        n = i["q"].shape[0]
        assert n == len(OC.dominant_places(T)) and i["want"].shape == (n, OC.ATTN_H, OC.HD)
        K = i["K"].clone()
        if self_mode:
            assert bool(torch.isnan(i["K"][:, T - 1]).all()) and bool(torch.isnan(i["V"][:, T - 1]).all())  # the poison
            K[:, T - 1] = i["knew"]
        s = torch.einsum("uthc,uhc->uht", K.double(), i["q"].double()) * 0.125
        for u in range(n):
            for h in range(OC.ATTN_H):
                d = int(i["dom"][u, h])
                others = torch.cat([s[u, h, :d], s[u, h, d + 1:]])
                assert float(s[u, h, d]) == 256.0 and (others.numel() == 0 or float(s[u, h, d] - others.max()) > 200.0)
        assert _bits(OC.attn_reference(i, torch.float32, T=T), i["want"]), T
        assert torch.equal(OC.attn_reference(i, torch.float64, T=T).float(), i["want"]), T  # in fp64 the others weigh 1e-98, not 0
    for T in OC.ATTN_UNIFORM_T:
        i = OC.attn_uniform_inputs(T, self_mode)
        assert T & (T - 1) == 0 and bool((i["want"] * T == (i["want"] * T).round()).all())
        for dtype in (torch.float32, torch.float64):
            assert _bits(OC.attn_reference(i, dtype, T=T).float(), i["want"]), (T, dtype)


@pytest.mark.parametrize("name", list(OC.ATTN_REAL))
def test_attention_real_cases(name):
    i = OC.attn_real_inputs(name)
    want, f32, floor = OC.attn_real_want(name), OC.attn_real_want(name, torch.float32), OC.attn_real_floor(name)
    stds = []
    for u, T in enumerate(i["T"]):
        if T >= 33:
            K = i["K"][u, :T].double().clone()
            if "knew" in i:
                K[T - 1] = i["knew"][u].double()
            stds.append(float((torch.einsum("thc,hc->ht", K, i["q"][u].double()) * 0.125).std()))
    print(f"{name}: {want.numel()} outputs, score std {min(stds):.2f} .. {max(stds):.2f}, floor {floor:.3e}")
    assert want.numel() >= 1024 and bool(torch.isfinite(want).all()) and 0.0 < floor < 1e-4
    assert all(2.0 <= s <= 4.5 for s in stds)  # near 3: a flat softmax hides a wrong key
    assert float((f32.double() - want).abs().max()) <= OC.TOL_FACTOR * floor
    assert sorted(OC.ATTN_REAL["self"]) == sorted(OC.ATTN_SELF_T) and len(i["T"]) == 8


EXPECTED_STOP = {"eos": R.STOP_EOS, "max_new_cap": R.STOP_MAX_NEW, "max_target_cap": R.STOP_MAX_TARGET}


@pytest.mark.parametrize("V", OC.HEAD_V)
def test_head_cases(V):
    c, want = OC.head_case(V), OC.head_want(V)
    sup, beg = OR.suppress_lists(c["smap"])
    assert sup == [1, 2, 7] and beg == [3, c["eos"]]
    by_name = dict(zip(c["rows"], range(len(c["rows"]))))
    for what, u in by_name.items():
        st, out = want[u]
        before = {k: c["state"][u][k] for k in ("cur", "pos", "count", "finished")}
        if what == "finished":
            assert out is None and st == before
        elif what == "in_prompt":
            assert out is None and st == dict(before, cur=c["prompt"][u][1], pos=1)
        else:
            assert out["stop"] == EXPECTED_STOP.get(what, 0), (what, out)
            assert st["finished"] == (1 if out["stop"] else 0) and st["count"] == out["g"] + 1
            assert out["token"] not in sup and (out["g"] > 0 or out["token"] not in beg)
            lp32 = float(torch.tensor(out["logprob"], dtype=torch.float32))
            assert abs(lp32 - out["logprob"]) <= OC.LOGPROB_REL * max(1.0, abs(out["logprob"]))  # an fp32 result can meet the bound
    row = lambda what: c["logits"][by_name[what]]
    out = lambda what: want[by_name[what]][1]
    # the ties are real ties, and the lowest index wins
    for what in ("tie_in_stride", "tie_across_threads", "tie_everywhere"):
        top = (row(what) == row(what).max()).nonzero().flatten().tolist()
        assert len(top) >= 2 and out(what)["token"] == top[0]
        if V > 256 and what == "tie_in_stride":
            assert top[1] - top[0] == 256
        if V > 256 and what == "tie_across_threads":  # a thread below 128 holds the higher index, its partner at w = 128 the lower one
            assert len(top) == 2 and top[1] >= 256 and top[1] % 256 + 128 == top[0]
    assert int(row("max_suppressed").argmax()) == 7 and out("max_suppressed")["token"] == 20
    assert int(row("begin_suppressed_g0").argmax()) == 3 and out("begin_suppressed_g0")["g"] == 0 and out("begin_suppressed_g0")["token"] != 3
    assert out("begin_suppressed_g1")["g"] == 1 and out("begin_suppressed_g1")["token"] == 3
    assert out("eos")["token"] == c["eos"] and out("plain_last_index")["token"] == V - 1
    forced = OC.head_want(V, forced=True)
    for what, u in by_name.items():
        if forced[u][1] is not None:
            f = forced[u][1]
            assert f["token"] == (7 if what == "max_suppressed" else 12) and f["stop"] != R.STOP_EOS
            assert (f["logprob"] == float("-inf")) == (what == "max_suppressed")
            assert f["stop"] == (0 if what == "eos" else EXPECTED_STOP.get(what, 0))


@pytest.mark.parametrize("d", OC.EMBED_D)
def test_embed_cases(d):
    i = OC.embed_inputs(d)
    want = OR.embed(i["tok"], i["pos_table"], i["cur"], i["pos"])
    assert want.shape == (i["n"], d) and want.dtype == torch.float32
    assert int(i["cur"].max()) == i["tok"].shape[0] - 1 and int(i["pos"].max()) == i["pos_table"].shape[0] - 1  # the tables' last rows
    assert torch.equal(want, (i["tok"].double()[i["cur"].long()] + i["pos_table"].double()[i["pos"].long()]).float())  # one rounding
    assert not torch.equal(want[2], want[3])  # same token, another position


# ---- 4. deliberate mistakes --------------------------------------------------------------------------------------------------------
def _gemm_applies(mut, M, N, K):
    return {"last_chunk_dropped": K > OR.SK_KC, "chunk0_reused": K > OR.SK_KC, "column_clip_off_by_one": True, "row8_from_row0": M > 8}[mut]


@pytest.mark.parametrize("mut", OR.GEMM_MUTATIONS)
def test_gemm_mistakes_are_seen(mut):
    seen_exact = seen_real = 0
    for shape in OC.GEMM_EXACT_SHAPES:
        if not _gemm_applies(mut, *shape):
            continue
        for bias, res in ((False, False), (True, True)):
            assert not torch.equal(OC.gemm_exact_want(shape, bias, res, torch.float32, (mut,)), OC.gemm_exact_want(shape, bias, res, torch.float32)), shape
        seen_exact += 1
    for name, (M, N, K, act, res) in OC.GEMM_REAL.items():
        if not _gemm_applies(mut, M, N, K):
            continue
        moved = float((OC.gemm_real_want(name, mut=(mut,)) - OC.gemm_real_want(name)).abs().max())
        ratio = moved / (OC.TOL_FACTOR * OC.gemm_real_floor(name))
        print(f"{mut} on {name}: moves the output by {ratio:.3e} x the GPU bound")
        assert ratio >= OC.MUTATION_FACTOR
        seen_real += 1
    assert seen_exact >= 2 and seen_real >= 2


@pytest.mark.parametrize("mut", OR.ATTN_MUTATIONS)
def test_attention_mistakes_are_seen(mut):
    seen_exact = seen_real = 0
    for self_mode in (False, True):
        if mut == "stale_cache_row" and not self_mode:
            continue
        for T in OC.ATTN_DOMINANT_T:
            if (mut == "key256_skipped" and T <= 256) or (mut == "quarter_off_by_one" and T < 2):
                continue
            i = OC.attn_dominant_inputs(T, self_mode)
            assert not _bits(OC.attn_reference(i, torch.float32, (mut,), T=T), i["want"]), (T, self_mode)
            seen_exact += 1
    for name in OC.ATTN_REAL:
        if mut == "stale_cache_row" and name != "self":
            continue
        if mut == "key256_skipped" and max(OC.ATTN_REAL[name]) <= 256:
            continue
        moved = float((OC.attn_real_want(name, mut=(mut,)) - OC.attn_real_want(name)).abs().max())
        ratio = moved / (OC.TOL_FACTOR * OC.attn_real_floor(name))
        print(f"{mut} on {name}: moves the output by {ratio:.3e} x the GPU bound")
        assert ratio >= OC.MUTATION_FACTOR
        seen_real += 1
    assert seen_exact >= 2 and seen_real >= 1


@pytest.mark.parametrize("mut", OR.HEAD_MUTATIONS)
def test_head_mistakes_are_seen(mut):
    for V in OC.HEAD_V:
        c, want, bad = OC.head_case(V), OC.head_want(V), OC.head_want(V, mut=(mut,))
        tokens = [what for what, a, b in zip(c["rows"], want, bad) if a[1] is not None and a[1]["token"] != b[1]["token"]]
        moved = max(abs(a[1]["logprob"] - b[1]["logprob"]) / (OC.LOGPROB_REL * max(1.0, abs(a[1]["logprob"])))
                    for a, b in zip(want, bad) if a[1] is not None)
        print(f"{mut} at V = {V}: tokens differ on {tokens}, a log-probability moves by {moved:.3e} x its bound")
        if mut == "higher_index_on_tie":
            assert {"tie_in_stride", "tie_across_threads", "tie_everywhere", "max_suppressed"} <= set(tokens)
        elif mut == "begin_suppress_always":
            assert "begin_suppressed_g1" in tokens
        else:
            assert moved >= OC.MUTATION_FACTOR


# ---- 5. the entries ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from valle_amd import engine

    ge.build()
    return engine.load_library()


def test_refusals_before_any_hip_call(lib):
    p = 4096  # never dereferenced: the checks come first
    err = lambda: lib.vx_last_error()
    assert lib.vx_op_wsp_gemm(p, p, None, None, p, 8, 16, 18, 0, None) == 1 and b"K = 18" in err()
    assert lib.vx_op_wsp_gemm(p, p, None, None, p, 65, 16, 16, 0, None) == 1 and b"M = 65" in err()
    assert lib.vx_op_wsp_gemm(p, p, None, None, p, 0, 16, 16, 0, None) == 1 and lib.vx_op_wsp_gemm(p, None, None, None, p, 8, 16, 16, 0, None) == 1
    assert lib.vx_op_wsp_gemm(p, p, None, None, p, 8, 16, 16, 2, None) == 1 and b"act = 2" in err()
    attn = lambda **o: lib.vx_op_wsp_decode_attn(*[dict(dict(q=p, knew=None, vnew=None, kc=p, vc=p, out=p, ld=256, ldq=128, d=128, H=2, n=2, pos=None,
                                                              keys=100, rows=100, max_keys=100, stream=None), **o)[k] for k in
                                                    ("q", "knew", "vnew", "kc", "vc", "out", "ld", "ldq", "d", "H", "n", "pos", "keys", "rows", "max_keys",
                                                     "stream")])
    assert attn(max_keys=4097) == 1 and b"max_keys = 4097" in err()
    assert attn(max_keys=0) == 1 and attn(q=None) == 1 and attn(knew=p) == 1 and attn(knew=p, vnew=p) == 1
    assert attn(keys=101) == 1 and b"keys = 101" in err()
    assert attn(keys=0) == 1 and attn(rows=99) == 1 and attn(d=100) == 1 and attn(ldq=126) == 1 and attn(ld=64) == 1 and attn(n=65) == 1
    head = [p, 2, 101, p, p, 4, p, p, None, p, p, p, p, p, p, p, p, 6, 96, 40, None]
    assert lib.vx_op_wsp_head(*(head[:18] + [101] + head[19:])) == 1 and b"eos = 101" in err()
    assert lib.vx_op_wsp_head(*([None] + head[1:])) == 1 and lib.vx_op_wsp_head(*(head[:1] + [0] + head[2:])) == 1
    assert lib.vx_op_wsp_embed(p, p, p, None, p, 2, 64, 10, 10, None) == 1 and lib.vx_op_wsp_embed(p, p, p, p, p, 65, 64, 10, 10, None) == 1
