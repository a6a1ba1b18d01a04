"""GPU: continuous batching (vx_batch_open / vx_batch_admit / vx_batch_run, VALLE.inference_stream).  Utterances enter vacant
slots while the other slots keep decoding; every slot must still behave like an independent batch-1 inference() of the
reference, and an admission must leave the slots already live bitwise untouched."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from test_gpu_batch import BMAX, _few_threads, _setup, _utts

pytestmark = pytest.mark.gpu

SHAPES12 = [(3 + (i * 5) % 9, 8 + (i * 13) % 47) for i in range(12)]  # S in [3, 11], P in [8, 54]


def _stream(m, utts, **kw):
    out = {}
    for i, codes in m.inference_stream(utts, **kw):
        assert i not in out, i  # every utterance is yielded once
        out[i] = codes
    assert sorted(out) == list(range(len(utts)))
    return [out[i] for i in range(len(utts))]


def test_stream_matches_static_batching():
    """inference_stream with per-slot admission == inference_batch with per-slot prefill, bitwise, for every utterance: slots are
    refilled mid-decode (ragged lengths, one free slot triggers an admission, stops polled every 4 steps), yet each utterance's
    sampler draws from its own seed and its slot's rows of the shared step do not depend on what the other slots hold."""
    cfg, sd, m = _setup(max_batch=4)
    utts = _utts(SHAPES12)
    seeds = [101 + 7 * i for i in range(12)]
    ref = m.inference_batch(utts, top_k=5, seeds=seeds, batched_prefill=False, batched_nar=False)
    got = _stream(m, utts, top_k=5, seeds=seeds, batched_admit=False, batched_nar=False, poll_steps=4, refill_at=1)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a.shape == b.shape == (1, 16 * utts[i][0].shape[1] + 1, 8), i
        assert torch.equal(a, b), i
    # batched NAR over whichever utterances finished together: the AR codes stay bitwise equal, the NAR stages run at a
    # different row count (GEMM tiling) than the static path's groups
    ref2 = m.inference_batch(utts, top_k=5, seeds=seeds, batched_prefill=False)
    got2 = _stream(m, utts, top_k=5, seeds=seeds, batched_admit=False, nar_group=3, poll_steps=8)
    for i, (a, b) in enumerate(zip(ref2, got2)):
        assert a.shape == b.shape
        assert torch.equal(a[0, :, 0], b[0, :, 0]), i
        assert (a == b).float().mean().item() >= 0.98, i
    # batched admission: same shapes and ranges, every utterance stops by its own length rule
    got3 = _stream(m, utts, top_k=5, seeds=seeds)
    for i, c in enumerate(got3):
        assert c.shape == ref[i].shape and int(c.min()) >= 0 and int(c.max()) < 1024


def _run_all(eng, poll_steps=4):
    """Runs the session until no slot is live; returns {slot: (tokens, reason)}."""
    res = {}
    while True:
        st = eng.batch_run(1, poll_steps)
        if not st:
            return res
        for s in st:
            res[s] = eng.batch_result(s)


def test_slot_mapped_batched_admission():
    """Batched admission into slots {3, 1}, then into {0, 2} while 3 and 1 are mid-decode: first logits within the bf16 rule of
    the per-slot prefill's, teacher-forced per-pass argmax agreement >= 0.97, and the live slots' tokens and logits rows bitwise
    those of a run without the second admission."""
    cfg, sd, m = _setup(max_batch=4, trace_logits=True)
    eng = m.engine()
    stride = eng.max_audio + 2
    u = _utts([(6, 30), (9, 70), (7, 55), (11, 129), (3, 10)])
    A = [u[0], u[1]]  # -> slots 3, 1 (sampled, top-k 5, 40 tokens)
    Bu = [u[2], u[3]]  # -> slots 0, 2 (teacher-forced, 24 tokens)
    pacer = u[4]       # slot 2 first: stops after 6 forced tokens and frees it
    forced = [torch.randint(0, 1024, (24,), generator=torch.Generator().manual_seed(5 + i)).cuda() for i in range(2)]
    t = lambda us: [x[0][0] for x in us]
    p = lambda us: [x[2][0, :, 0].contiguous() for x in us]

    def session(second, batched=True):
        eng.batch_open()
        eng.batch_admit([2], t([pacer]), p([pacer]), top_k=1, forced=[torch.arange(6).cuda()], batched=False)
        eng.batch_admit([3, 1], t(A), p(A), top_k=5, seeds=[31, 11], max_new_tokens=40, batched=batched)
        lg_a = eng.read("batch_logits", (BMAX, 1088))[[3, 1], :1025].clone()
        assert eng.batch_run(1, 2) == [2]  # the pacer stops, 3 and 1 are mid-decode
        eng.batch_result(2)
        lg_b = None
        if second:
            eng.batch_admit([0, 2], t(Bu), p(Bu), top_k=1, forced=forced, batched=batched)
            lg_b = eng.read("batch_logits", (BMAX, 1088))[[0, 2], :1025].clone()
        res = _run_all(eng)
        arg = eng.read("batch_argmax", (BMAX, stride), dtype=torch.int32)
        trace = {s: eng.read("batch_trace", (40, 1025), offset_bytes=s * stride * 1025 * 4) for s in (3, 1)}
        return lg_a, lg_b, res, arg, trace

    lg_a0, _, res0, _, tr0 = session(False)
    lg_a, lg_b, res, arg, tr = session(True)
    lg_a_ref, lg_b_ref, res_ref, arg_ref, _ = session(True, batched=False)
    for s in (3, 1):  # the live slots: bitwise as without the admission
        assert torch.equal(res[s][0], res0[s][0]) and res[s][1] == res0[s][1] == 4, s
        assert res[s][0].numel() == 40
        assert torch.equal(tr[s], tr0[s]), s
    assert torch.equal(lg_a, lg_a0)
    for got, want in ((lg_a, lg_a_ref), (lg_b, lg_b_ref)):  # batched vs per-slot prefill
        for r in range(2):
            err = float((got[r] - want[r]).abs().max())
            assert err <= 0.03 * float(want[r].abs().max()), (r, err)
    for z, s in enumerate((0, 2)):
        assert torch.equal(res[s][0], forced[z].cpu()) and res[s][1] == 4
    agree = (arg[[0, 2], :24] == arg_ref[[0, 2], :24]).float().mean().item()
    assert agree >= 0.97, agree


@pytest.mark.parametrize("batched", [False, True])
def test_slot_reuse_does_not_leak(batched):
    """A short utterance admitted into the slot a long one has just left gives bitwise the codes it gives on a fresh engine."""
    _, _, m = _setup(max_batch=4)
    long_u, short_u = _utts([(12, 60), (4, 20)])
    eng = m.engine()
    eng.batch_open()
    eng.batch_admit([1], [long_u[0][0]], [long_u[2][0, :, 0].contiguous()], top_k=5, seeds=[7], batched=batched)
    first = _run_all(eng)
    assert first[1][0].numel() == 16 * 12 + 1
    eng.batch_admit([1], [short_u[0][0]], [short_u[2][0, :, 0].contiguous()], top_k=5, seeds=[9], batched=batched)
    reused = _run_all(eng)[1]
    _, _, m2 = _setup(max_batch=4)
    e2 = m2.engine()
    e2.batch_open()
    e2.batch_admit([1], [short_u[0][0]], [short_u[2][0, :, 0].contiguous()], top_k=5, seeds=[9], batched=batched)
    fresh = _run_all(e2)[1]
    assert reused[0].numel() == 16 * 4 + 1
    assert torch.equal(reused[0], fresh[0]) and reused[1] == fresh[1]


def test_admitted_mid_flight_teacher_forced_against_fp32_oracle():
    """Utterances admitted while another slot decodes, teacher-forced with the fp32 oracle's greedy tokens: per-pass argmax
    agreement >= 0.97 with the oracle's (the criteria of test_batch_teacher_forced_against_fp32_oracle)."""
    from oracle import valle_oracle as vo

    cfg, sd, m = _setup(max_batch=4)
    eng = m.engine()
    utts = _utts([(5, 30), (6, 12), (3, 55), (4, 20)])
    om = vo.OracleModel(sd, cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers, 1, False, 8)
    refs = []
    with _few_threads():
        for x, xl, y in utts:
            tr = {}
            codes = vo.inference_cached(om, x, xl, y, None, 1, 1.0, None, trace=tr, skip_nar=True)
            refs.append((codes[0, :, 0].contiguous(), torch.stack(tr["ar_logits"])))
    t = lambda i: [utts[i][0][0]]
    p = lambda i: [utts[i][2][0, :, 0].contiguous()]
    eng.batch_open()
    eng.batch_admit([0], t(0), p(0), top_k=1, forced=[refs[0][0].cuda()])
    eng.batch_admit([3], t(3), p(3), top_k=1, forced=[refs[3][0][:5].cuda()])  # a pacer: stops after 5 tokens
    assert eng.batch_run(1, 2) == [3]
    eng.batch_result(3)
    eng.batch_admit([3, 1], t(1) + t(2), p(1) + p(2), top_k=1, forced=[refs[1][0].cuda(), refs[2][0].cuda()])  # slot 0 mid-decode
    res = _run_all(eng)
    arg = eng.read("batch_argmax", (BMAX, eng.max_audio + 2), dtype=torch.int32)
    for s, i in ((0, 0), (3, 1), (1, 2)):
        toks, ref_logits = refs[i]
        assert torch.equal(res[s][0], toks) and res[s][1] == 4, s
        n = toks.numel()
        agree = (arg[s, :n].long() == ref_logits.argmax(1)[:n]).float().mean().item()
        assert agree >= 0.97, (s, agree)


def test_stream_does_not_depend_on_uninitialised_memory():
    """VX_POISON=1 (every fresh device allocation filled with NaN / -1 bytes): a stream whose tail leaves slots vacant, on an
    engine that never filled some of them, gives the same codes as without poison."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = (
        "import sys, json, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from test_gpu_batch import _setup, _utts\n"
        "cfg, sd, m = _setup(max_batch=4)\n"
        "u = _utts([(6, 30), (9, 12), (4, 55), (5, 8), (7, 21), (3, 40)])\n"
        "out = []\n"
        "for ba in (False, True):\n"
        "    r = dict(m.inference_stream(u[:2], top_k=5, seeds=[1, 2], batched_admit=ba))\n"
        "    r2 = dict(m.inference_stream(u, top_k=5, seeds=[11, 22, 33, 44, 55, 66], batched_admit=ba, poll_steps=4))\n"
        "    out += [r[i].flatten().tolist() for i in range(2)] + [r2[i].flatten().tolist() for i in range(6)]\n"
        "print(json.dumps(out))\n" % (root, os.path.join(root, "tests")))
    outs = []
    for poison in ("0", "1"):
        env = dict(os.environ, VX_POISON=poison)
        r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]
    assert all(0 <= v < 1024 for seq in outs[1] for v in seq)


def test_session_error_paths():
    from valle_amd.engine import VxError, VxDecodeParams

    _, _, m = _setup(max_batch=4)
    eng = m.engine()
    lib = eng.lib
    stopped, n = (C.c_int32 * 4)(), C.c_int32()
    assert lib.vx_batch_run(eng.h, 1, 0, stopped, C.byref(n), None) == 3  # before vx_batch_open: VX_ERR_STATE
    u = _utts([(4, 20), (12, 560), (6, 30)])
    t = lambda i: [u[i][0][0]]
    p = lambda i: [u[i][2][0, :, 0].contiguous()]
    with pytest.raises(VxError) as ei:
        eng.batch_admit([0], t(0), p(0))
    assert ei.value.code == 3
    eng.batch_open()
    assert eng.batch_run() == []  # nothing live
    eng.batch_admit([0], t(0), p(0), top_k=5, seeds=[3])
    for slots, code in (([0], 3), ([4], 1), ([-1], 1), ([1, 1], 1), ([1, 0], 3)):
        with pytest.raises(VxError) as ei:
            eng.batch_admit(slots, t(0) * len(slots), p(0) * len(slots))
        assert ei.value.code == code, (slots, str(ei.value))
    with pytest.raises(VxError) as ei:
        eng.batch_result(0)  # still decoding
    assert ei.value.code == 3
    # a forced run that cannot fit the KV cache is refused at admission, before slot 1 is touched
    with pytest.raises(VxError) as ei:
        eng.batch_admit([1], t(1), p(1), top_k=1, forced=[torch.zeros(200, dtype=torch.int64).cuda()])
    assert ei.value.code == 4
    # slot 2: the length rule allows 16 * 12 + 1 tokens but only 700 - 560 = 140 rows are left: the KV cache fills first (the
    # synthetic model has no EOS), and the capacity error names slot 2; slot 0 stops by its length rule
    eng.batch_admit([2], t(1), p(1), top_k=5, seeds=[4])
    errs = []
    while True:
        try:
            st = eng.batch_run(1, 4)
        except VxError as e:
            errs.append(e)
            st = eng._last_stopped
        if not st:
            break
        for s in st:
            if s == 0:
                with pytest.raises(VxError) as ei:  # stopped, not read yet
                    eng.batch_admit([0], t(2), p(2))
                assert ei.value.code == 3
            eng.batch_result(s)
    eng.batch_admit([0], t(2), p(2), top_k=5, seeds=[5])  # read: vacant again
    assert sorted(_run_all(eng)) == [0]
    assert len(errs) == 1 and errs[0].code == 4 and "slot 2" in str(errs[0]), errs
