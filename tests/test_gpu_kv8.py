"""GPU: fp8 slot caches of the batched decode (kv_cache="fp8", VX_FLAG_KV_FP8).  The caches' bytes must be exactly kv8_quant of
what a bf16 engine's caches hold after the same prefill / step; the logits must follow the host emulation (tests/kv8_ref.py)
within the bf16 tolerance and the plain fp32 oracle within KV8_TOL; streaming must equal static batching bitwise."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, Golden
from kv8_ref import KV8_TOL, kv8_forced_logits, kv8_quant
from test_gpu_batch import BMAX, _few_threads, _setup, _utts

pytestmark = pytest.mark.gpu

L, H, HD = 4, 4, 64  # _setup's model: d = 256


def _caches(eng, kind):
    """the slot caches as (max_batch, L, 2, H, ctx_max, 64) [+ scales (..., 4)]."""
    shape = (eng.max_batch, L, 2, H, eng.max_text + eng.max_audio)
    if kind == "bf16":
        return eng.read("batch_kv", shape + (HD,), dtype=torch.int16).view(torch.bfloat16)
    return eng.read("batch_kv", shape + (HD,), dtype=torch.uint8), eng.read("batch_kv_scale", shape + (HD // 16,), dtype=torch.uint8)


def _check_rows(ref_bf16, got, slot, rows, layers=range(L)):
    codes, scales = got
    for li in layers:
        src = ref_bf16[slot, li, :, :, rows].float()
        qc, qs = kv8_quant(src)
        assert torch.equal(codes[slot, li, :, :, rows], qc), (slot, li)
        assert torch.equal(scales[slot, li, :, :, rows], qs), (slot, li)


def test_cache_bytes_are_kv8_quant_of_the_bf16_cache():
    """Batched prefill, per-slot prefill and one step: every written row of the fp8 caches equals kv8_quant of the bf16 engine's
    row, bit for bit (codes and scales)."""
    _, _, ma = _setup(max_batch=4)
    _, _, mb = _setup(max_batch=4, kv_cache="fp8")
    ea, eb = ma.engine(), mb.engine()
    utts = _utts([(5, 30), (6, 12), (3, 55)])
    texts = [x[0] for x, _, _ in utts]
    proms = [y[0, :, 0].contiguous() for _, _, y in utts]
    lens = [t.numel() + p.numel() for t, p in zip(texts, proms)]
    for e in (ea, eb):
        e.batch_prefill_all(texts, proms)
    a, b = _caches(ea, "bf16"), _caches(eb, "fp8")
    assert torch.isfinite(a[:3, :, :, :, : max(lens)].float()).all()
    for s, n in enumerate(lens):
        _check_rows(a, b, s, slice(0, n))
    # per-slot prefill into other slots (3 gets utterance 0, 1 gets utterance 2)
    for e in (ea, eb):
        e.batch_prefill(3, texts[0], proms[0])
        e.batch_prefill(1, texts[2], proms[2])
    a, b = _caches(ea, "bf16"), _caches(eb, "fp8")
    _check_rows(a, b, 3, slice(0, lens[0]))
    _check_rows(a, b, 1, slice(0, lens[2]))
    # one forced step over slots 0..3: layer 0's new row depends on the token only, not on the cache format
    tok = [torch.tensor([7 + s], device="cuda") for s in range(4)]
    for e in (ea, eb):
        e.batch_decode(4, top_k=1, forced=tok)
    a, b = _caches(ea, "bf16"), _caches(eb, "fp8")
    for s, n in enumerate([lens[0], lens[2], lens[2], lens[0]]):
        _check_rows(a, b, s, slice(n, n + 1), layers=[0])
    # the fp8 engine's slot caches are 0.53x the bf16 ones' bytes: 64 codes + 4 scales per row of 64 bf16 values
    assert b[0].numel() + b[1].numel() == a.numel() * 68 // 64


def test_teacher_forced_logits_against_emulation_and_oracle():
    """d = 256: every pass of three slots, teacher-forced with the oracle's greedy tokens, against the emulated fp8-cache decoder
    (bf16 tolerance, argmax agreement) and the plain fp32 oracle (KV8_TOL)."""
    from oracle import valle_oracle as vo

    cfg, sd, m = _setup(max_batch=4, kv_cache="fp8", trace_logits=True)
    eng = m.engine()
    utts = _utts([(5, 30), (6, 12), (3, 55)])
    om = vo.OracleModel(sd, cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers, 1, False, 8)
    refs = []
    for x, xl, y in utts:
        tr = {}
        with _few_threads():
            codes = vo.inference_cached(om, x, xl, y, None, 1, 1.0, None, trace=tr, skip_nar=True)
        toks = codes[0, :, 0].contiguous()
        with _few_threads():
            emu = kv8_forced_logits(om, x[0], y[0, :, 0].contiguous(), toks, range(toks.numel()))
        refs.append((toks, torch.stack(tr["ar_logits"])[: toks.numel()], emu))
    eng.batch_prefill_all([u[0][0] for u in utts], [u[2][0, :, 0].contiguous() for u in utts])
    eng.batch_decode(3, top_k=1, forced=[r[0].cuda() for r in refs])
    stride = eng.max_audio + 2
    for b, (toks, plain, emu) in enumerate(refs):
        got_toks, reason = eng.batch_result(b)
        assert torch.equal(got_toks, toks) and reason == 4
        n = toks.numel()
        got = eng.read("batch_trace", (n, 1025), offset_bytes=b * stride * 1025 * 4)
        scale = emu.abs().amax(1)
        err_emu = ((got - emu).abs().amax(1) / scale).max().item()
        err_plain = ((got - plain).abs().amax(1) / plain.abs().amax(1)).max().item()
        agree = (got.argmax(1) == emu.argmax(1)).float().mean().item()
        print("slot", b, "passes", n, "err vs emulation %.4f" % err_emu, "vs plain oracle %.4f" % err_plain, "argmax agreement %.3f" % agree)
        assert err_emu <= 0.03, (b, err_emu)
        assert err_plain <= KV8_TOL, (b, err_plain)
        assert agree >= 0.97, (b, agree)


@pytest.mark.parametrize("B,precision,every", [(32, "bf16", 2), (64, "fp8nar", 8)])
def test_full_length_mixed_slots_teacher_forced(B, precision, every):
    """The AR part of test_batch_full_length_mixed_slots_teacher_forced with fp8 slot caches: slot b holds the cfg1 utterance
    (S=47, 753 tokens) when b % every == 0, else the configs[4] one (S=94, 1505 tokens), teacher-forced over its full length.
    Every slot's logits at the probe passes lie within the bf16 tolerance of the emulated fp8-cache decoder's
    (tests/golden/kv8/), argmax exact where the margin allows, and slots of one kind are bitwise equal."""
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.models import VALLE

    names = ["cfg1_topk10", "cfg4_s94_topk10"]
    gs = [Golden(n) for n in names]
    fx = [np.load(os.path.join(GOLDEN, "kv8", n + ".npz")) for n in names]
    kind = [0 if b % every == 0 else 1 for b in range(B)]
    m = VALLE(1024, 16, 12, prefix_mode=1, precision=precision, max_text=128, max_audio=1792, print_eos=False, max_batch=B,
              trace_logits=True, kv_cache="fp8")
    m.load_state_dict(gs[0].state_dict())
    m.to("cuda:0").eval()
    eng = m.engine()
    forced = [gs[k].codes[0, :, 0].contiguous() for k in kind]
    eng.batch_prefill_all([gs[k].x[0] for k in kind], [gs[k].y[0, :, 0].contiguous() for k in kind])
    eng.batch_decode(B, top_k=10, forced=[f.cuda() for f in forced])
    stride = eng.max_audio + 2
    arg = eng.read("batch_argmax", (BMAX, stride), dtype=torch.int32)
    first, worst = {}, 0.0
    for b in range(B):
        k = kind[b]
        toks, reason = eng.batch_result(b)
        assert torch.equal(toks, forced[b]) and reason == 4, b
        steps = [int(s) for s in fx[k]["probe_steps"]]
        rows = torch.stack([eng.read("batch_trace", (1025,), offset_bytes=(b * stride + s) * 1025 * 4) for s in steps])
        if k not in first:
            first[k] = (b, rows)
        b0, rows0 = first[k]
        assert torch.equal(rows, rows0), (b, b0)
        T = forced[b].numel()
        assert torch.equal(arg[b, : T + 1], arg[b0, : T + 1]), (b, b0)
        emu, plain = torch.from_numpy(fx[k]["kv8_logits"]), torch.from_numpy(fx[k]["plain_logits"])
        for s, got, ref, pl in zip(steps, rows, emu, plain):
            tol = 0.03 * float(ref.abs().max())
            err = float((got - ref).abs().max())
            worst = max(worst, err / float(ref.abs().max()))
            assert err <= tol, (b, s, err, tol)
            assert float((got - pl).abs().max()) <= KV8_TOL * float(pl.abs().max()), (b, s)
            top2 = ref.topk(2)[0]
            if float(top2[0] - top2[1]) > 2 * tol:
                assert int(got.argmax()) == int(ref.argmax()) == int(arg[b, s]), (b, s)
    print("B", B, precision, "kv fp8: worst probe error vs emulation %.4f of the row scale" % worst)


def test_stream_matches_static_batching_fp8():
    """inference_stream == inference_batch bitwise with fp8 slot caches (per-slot admission, slots refilled next to live ones)."""
    from test_gpu_stream import SHAPES12, _stream

    cfg, sd, m = _setup(max_batch=4, kv_cache="fp8")
    utts = _utts(SHAPES12)
    seeds = [101 + 7 * i for i in range(12)]
    ref = m.inference_batch(utts, top_k=5, seeds=seeds, batched_prefill=False, batched_nar=False)
    got = _stream(m, utts, top_k=5, seeds=seeds, batched_admit=False, batched_nar=False, poll_steps=4, refill_at=1)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a.shape == b.shape == (1, 16 * utts[i][0].shape[1] + 1, 8), i
        assert torch.equal(a, b), i
    # batched admission next to live slots: same AR codes as the static path's batched prefill of the same groups is not
    # guaranteed (different GEMM row counts), so check shapes, ranges and determinism
    got2 = _stream(m, utts, top_k=5, seeds=seeds, poll_steps=4)
    got3 = _stream(m, utts, top_k=5, seeds=seeds, poll_steps=4)
    for i, (a, b) in enumerate(zip(got2, got3)):
        assert a.shape == ref[i].shape and torch.equal(a, b), i
        assert int(a.min()) >= 0 and int(a.max()) < 1024


def test_fp8_cache_does_not_depend_on_uninitialised_memory():
    """VX_POISON=1 fills fresh allocations with 0xFF (an e4m3 NaN code, a NaN-producing scale): a read of a cache row nothing
    wrote would change the codes.  Static batching and streaming with fp8 slot caches must give the same codes either way."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = (
        "import sys, json, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from test_gpu_batch import _setup, _utts\n"
        "cfg, sd, m = _setup(max_batch=4, kv_cache='fp8')\n"
        "u = _utts([(6, 30), (9, 12), (4, 55), (5, 20), (3, 9)])\n"
        "a = m.inference_batch(u[:3], top_k=5, seeds=[11, 22, 33])\n"
        "b = dict(m.inference_stream(u, top_k=5, seeds=[1, 2, 3, 4, 5], poll_steps=4))\n"
        "print(json.dumps([t.flatten().tolist() for t in a] + [b[i].flatten().tolist() for i in range(5)]))\n"
        % (root, os.path.join(root, "tests")))
    outs = []
    for poison in ("0", "1"):
        env = dict(os.environ, VX_POISON=poison)
        r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]
    assert all(0 <= v < 1024 for seq in outs[1] for v in seq)
