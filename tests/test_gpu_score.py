"""GPU: scoring (vx_op_nll_rows, vx_score, vx_score_batch, VALLE.score / score_batch) against the fp64 restatement score_ref.py.

Tolerances are those of test_gpu_engine.py (score_cases.py names them): an error of delta on every logit of a row moves that
row's nll by at most 2 delta (once through logsumexp, once through the target's own entry), and cannot change its rank unless
another entry lies within 2 delta of the target's value (score_ref.decided)."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import score_cases as sc
import score_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODELS = {}


def _model(cfg, sd, precision, **kw):
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.models import VALLE, VALLF

    key = (repr(cfg), precision, tuple(sorted(kw.items())))
    if key not in _MODELS:
        kw.setdefault("max_text", 32)
        kw.setdefault("max_audio", 192)
        cls = VALLF if cfg.is_vallf else VALLE
        m = cls(cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers, norm_first=cfg.norm_first, add_prenet=cfg.add_prenet,
                prefix_mode=cfg.prefix_mode, share_embedding=cfg.share_embedding, nar_scale_factor=cfg.scale_factor,
                prepend_bos=cfg.prepend_bos, num_quantizers=cfg.num_quantizers, precision=precision, print_eos=False, **kw)
        m.load_state_dict(sd)
        _MODELS[key] = m.to("cuda:0").eval()
    return _MODELS[key]


def _score(m, u):
    return m.score(u["x"].cuda(), u["x_lens"].cuda(), u["y"].cuda(), prompt_frames=u["P"])


# ---------------------------------------------------------------------------------------------- case 1: the kernel
def _master(V, seed=0):
    """259 rows of N(0, 4) logits with the special rows of the issue at 0..7, and their targets."""
    g = torch.Generator().manual_seed(seed + V)
    lg = torch.randn(259, V, generator=g) * 2.0
    tg = torch.randint(0, V, (259,), generator=g)
    ninf = float("-inf")
    lg[0] += 80.0                                        # fails without the max subtraction (exp overflows)
    lg[1] -= 80.0                                        # ... (every exp underflows to 0)
    keep = torch.randperm(V, generator=g)[: V - 900]
    row = torch.full((V,), ninf)
    row[keep] = lg[2, keep]
    lg[2], tg[2] = row, keep[3]                          # 900 entries at -inf, a finite target
    lg[3, tg[3]] = ninf                                  # the target's entry is -inf: +inf expected
    top = lg[4].argmax()
    lg[4, (top + 17) % V] = lg[4, top]                   # an exact tie at the maximum ...
    tg[4] = (top + 40) % V
    lg[4, (top + 90) % V] = lg[4, tg[4]]                 # ... and one at the target's value
    tg[5], tg[6], tg[7] = 0, V - 1, min(sr.EOS, V - 1)   # first / last column, the EOS id
    return lg, tg


def _run_kernel(lg, tg, ld):
    from valle_amd.engine import op_nll_rows

    rows, V = lg.shape
    buf = torch.full((rows, ld), float("nan"))           # the columns past V must never be read
    buf[:, :V] = lg
    nll, rank, am = op_nll_rows(buf.cuda(), tg.cuda(), V=V)
    torch.cuda.synchronize()
    return nll.cpu(), rank.cpu(), am.cpu()


@pytest.mark.parametrize("V", [1024, 1025])
@pytest.mark.parametrize("pad", [0, 7])
def test_nll_rows_kernel_against_fp64(V, pad):
    """rank / argmax exact; nll under the floor rule: worst error against fp64 at most 4 x that of torch's own fp32
    F.cross_entropy(reduction="none") on the host, same inputs, same fp64 (the ratio is printed).  rows = 259 is many
    workgroups with a ragged tail (4 rows per workgroup); 1, 4 and 5 are one row, a full workgroup and one row over, and must
    give bit for bit the 259-row call's values for the same rows (a row's result does not depend on the launch), which also
    carries the floor rule over to them."""
    import __graft_entry__ as ge

    ge.build()
    lg, tg = _master(V)
    ref_nll, ref_rank, ref_am = sr.nll_rank_argmax(lg, tg)
    nll, rank, am = _run_kernel(lg, tg, V + pad)
    assert torch.equal(rank.long(), ref_rank) and torch.equal(am.long(), ref_am)
    assert float(nll[3]) == float("inf") and int(rank[3]) == int((lg[3] > float("-inf")).sum())
    fin = torch.isfinite(ref_nll)
    assert int((~fin).sum()) == 1 and bool(torch.isfinite(nll[fin]).all())
    ce = F.cross_entropy(lg, tg, reduction="none")
    err_k = float((nll.double() - ref_nll)[fin].abs().max())
    err_t = float((ce.double() - ref_nll)[fin].abs().max())
    print(f"nll_rows V={V} ld={V + pad}: kernel worst |err| {err_k:.3e}, torch fp32 cross_entropy {err_t:.3e}, ratio {err_k / max(err_t, 1e-300):.3f}")
    assert err_k <= 4 * err_t
    for rows, offs in ((1, (0, 1, 2, 3, 4, 5, 6, 7, 200)), (4, (0, 4)), (5, (0, 3))):
        for o in offs:
            n1, r1, a1 = _run_kernel(lg[o : o + rows], tg[o : o + rows], V + pad)
            assert torch.equal(n1.view(torch.int32), nll[o : o + rows].view(torch.int32)), (rows, o)  # bit-identical (inf included)
            assert torch.equal(r1, rank[o : o + rows]) and torch.equal(a1, am[o : o + rows])


def test_nll_rows_kernel_bad_device_targets_are_flagged():
    lg, tg = _master(1025)
    lg, tg = lg[:6].clone(), tg[:6].clone()
    tg[1], tg[4] = -1, 1025
    nll, rank, am = _run_kernel(lg, tg, 1025)
    assert bool(torch.isnan(nll[[1, 4]]).all()) and rank[[1, 4]].tolist() == [-1, -1]
    ok = [0, 2, 3, 5]
    r_nll, r_rank, r_am = sr.nll_rank_argmax(lg[ok], tg[ok])
    assert torch.equal(rank[ok].long(), r_rank) and torch.equal(am.long(), sr.nll_rank_argmax(lg, tg.clamp(0, 1024))[2])


# ---------------------------------------------------------------------------------- cases 2 / 4: fp32 engine vs oracle
def _check_fp32(u, res):
    ref = u["ref"]
    d_ar, d_nar = sc.decided_fp32(ref)
    ar_nll, ar_rank = res.ar_nll.cpu().double(), res.ar_rank.cpu().long()
    err = float((ar_nll - ref["ar_nll"]).abs().max())
    msg = f"AR decided {float(d_ar.float().mean()):.3f} nll err {err:.2e}"
    assert float(d_ar.float().mean()) >= sc.DECIDED_MIN
    assert torch.equal(ar_rank[d_ar], ref["ar_rank"][d_ar])
    assert err <= 2 * sc.FP32_AR_TOL
    assert res.ar_loss == pytest.approx(float(ref["ar_nll"].sum()), abs=2 * sc.FP32_AR_TOL * ar_nll.numel())
    keep = ref["ar_targets"] != sr.EOS
    assert res.ar_topk_acc == pytest.approx(float((ar_rank[keep] < 10).float().mean()))
    if d_nar is not None:
        nar_nll, nar_rank = res.nar_nll.cpu().double(), res.nar_rank.cpu().long()
        tol = sc.FP32_NAR_REL * sc.absmax(ref["nar_logits"]).double() + 1e-6
        nerr = (nar_nll - ref["nar_nll"]).abs()
        msg += f"; NAR decided {float(d_nar.float().mean()):.3f} worst nll err / tol {float((nerr / tol).max()):.3f}"
        assert float(d_nar.float().mean()) >= sc.DECIDED_MIN
        assert torch.equal(nar_rank[d_nar], ref["nar_rank"][d_nar])
        assert bool((nerr <= 2 * tol).all())
        assert res.nar_loss == pytest.approx([float(v) for v in ref["nar_nll"].sum(1)], rel=1e-4)
    print(msg)


@pytest.mark.parametrize("bos,P", [(False, 5), (True, 5), (True, 0)])
def test_fp32_engine_score_matches_oracle(bos, P):
    """d 256 / 4 heads / 2 layers, Q = 8, S = 7, A = 70: with P = 5 the scored rows straddle the 64-row tile edge of the row
    kernels; P = 0 with BOS is the reference's validation form (valle.py:863-881 at batch size 1)."""
    u = sc.utterance(sc.config(prepend_bos=bos), P=P)
    _check_fp32(u, _score(_model(u["cfg"], u["sd"], "fp32"), u))


def test_fp32_engine_score_random_targets():
    """The same model on a plainly random utterance (no oracle-chosen tokens): AR ranks spread over the whole vocabulary.  The
    margin decides fewer rows there (flat synthetic AR logits), so no floor on the decided share; every decided row is exact."""
    u = sc.utterance(sc.config(prepend_bos=True), P=5, seed=2, likely=False)
    ref = u["ref"]
    res = _score(_model(u["cfg"], u["sd"], "fp32"), u)
    d_ar, d_nar = sc.decided_fp32(ref)
    ar_rank, nar_rank = res.ar_rank.cpu().long(), res.nar_rank.cpu().long()
    print(f"random targets: AR decided {float(d_ar.float().mean()):.3f}, median AR rank {int(ref['ar_rank'].median())}, NAR decided {float(d_nar.float().mean()):.3f}")
    assert int(d_ar.sum()) >= 20 and int(ref["ar_rank"][d_ar].max()) >= 100  # mid-range ranks are among the compared rows
    assert torch.equal(ar_rank[d_ar], ref["ar_rank"][d_ar]) and torch.equal(nar_rank[d_nar], ref["nar_rank"][d_nar])
    assert float((res.ar_nll.cpu().double() - ref["ar_nll"]).abs().max()) <= 2 * sc.FP32_AR_TOL


def test_score_follows_a_weight_reload_on_the_same_engine():
    """load A, score, load B on the SAME engine, score: the second score must be that of a fresh engine with B (the padded
    copy of the predict layer that MFMA engines score with is rebuilt with the weights)."""
    from valle_amd.engine import Engine
    from valle_amd.weights import synthetic_state_dict

    u = sc.utterance(sc.config())
    sd_b = synthetic_state_dict(u["cfg"], 5)
    for prec in ("bf16", "fp32"):
        e = Engine(u["cfg"], precision=prec, max_text=32, max_audio=192)
        e.load_state_dict(u["sd"])
        a = [t.cpu() for t in e.score(*_engine_args(u))]
        e.load_state_dict(sd_b)
        b = [t.cpu() for t in e.score(*_engine_args(u))]
        fresh = Engine(u["cfg"], precision=prec, max_text=32, max_audio=192)
        fresh.load_state_dict(sd_b)
        want = [t.cpu() for t in fresh.score(*_engine_args(u))]
        assert not torch.equal(a[0], b[0])
        for x, y in zip(b, want):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), prec
        assert torch.equal(e.read("score_ar_argmax", (b[0].numel(),), torch.int32), fresh.read("score_ar_argmax", (b[0].numel(),), torch.int32))
        e.close(); fresh.close()


@pytest.mark.parametrize("kw,seed", [(dict(model_name="VALL-F", num_quantizers=3, prepend_bos=True), 1), (dict(norm_first=False, num_quantizers=3), 1),
                                     (dict(add_prenet=True, num_quantizers=3), 1),
                                     (dict(model_name="VALL-F", add_prenet=True, num_quantizers=2), 4),  # seed 1: the oracle decides 19 of 22 AR rows
                                     (dict(num_quantizers=1, prepend_bos=True), 1)],
                         ids=["vallf", "postnorm", "prenet", "vallf-prenet", "q1"])
def test_fp32_engine_score_other_models(kw, seed):
    """VALL-F (text as cross-attention memory), a post-norm model, prenet models and a Q = 1 model through vx_score, each
    against its own oracle (OracleModelF / OracleModel) as above, one small shape each."""
    u = sc.utterance(sc.config(decoder_dim=128, nhead=2, **kw), S=5, A=24, P=3, seed=seed)
    res = _score(_model(u["cfg"], u["sd"], "fp32"), u)
    _check_fp32(u, res)
    if kw.get("num_quantizers") == 1:
        assert res.nar_nll is None and res.nar_loss is None


def test_engine_argument_checks():
    """Every check answers before any work is enqueued (vx_score, vx_score_batch), with its code and message."""
    import ctypes as C
    from valle_amd.engine import VxError, _check

    u = sc.utterance(sc.config())
    m = _model(u["cfg"], u["sd"], "fp32")
    e = m.engine()
    text, codes = u["text"], u["codes"].contiguous()
    out = torch.empty(256, dtype=torch.float32, device="cuda")

    def call(text=text, S=7, text_nar=text, S2=7, codes=codes, A=70, P=5, h=None):
        p = lambda t: None if t is None else t.data_ptr()
        return e.lib.vx_score(e.h if h is None else h, p(text), S, p(text_nar), S2, p(codes), A, P, out.data_ptr(), None, out.data_ptr(), None, None)

    for kw, code, match in [(dict(codes=None), 1, "null"), (dict(text=None), 1, "null"), (dict(text_nar=None), 1, "null"),
                            (dict(P=70), 1, "P=70"), (dict(P=-1), 1, "P=-1"), (dict(P=0), 1, "prepend_bos"), (dict(S=0), 1, "S"),
                            (dict(S=33), 4, "capacity"), (dict(A=192), 4, "capacity")]:
        assert call(**kw) == code and match.encode() in e.lib.vx_last_error(), (kw, e.lib.vx_last_error())
    bad = codes.clone()
    bad[40, 3] = 1024  # host codes are range-checked by the engine itself
    assert call(codes=bad) == 1 and b"frame 40, codebook 3" in e.lib.vx_last_error()
    with pytest.raises(VxError) as ei:  # fp32 engine: no concatenated pass
        e.score_batch([text], [text], [codes], [5])
    assert ei.value.code == 5 and "vx_score" in str(ei.value)
    from valle_amd.engine import Engine

    raw = Engine(u["cfg"], precision="fp32", max_text=32, max_audio=192)  # weights never finalised
    assert call(h=raw.h) == 3 and b"finalized" in e.lib.vx_last_error()
    raw.close()


# ------------------------------------------------------------------------------------------------- case 3: bf16
def _check_bf16(u, parts, label):
    """Per-row |nll - ref| within 2 x the bf16 logits tolerance (BF16_REL_TOL x the reference row's largest magnitude)."""
    ref = u["ref"]
    an, ak, nn_, nk = [t.cpu() for t in parts]
    tol = 2 * sc.BF16_REL_TOL * sc.absmax(ref["ar_logits"]).double()
    err = (an.double() - ref["ar_nll"]).abs()
    ntol = 2 * sc.BF16_REL_TOL * sc.absmax(ref["nar_logits"]).double()
    nerr = (nn_.double() - ref["nar_nll"]).abs()
    print(f"{label}: AR worst nll err / bound {float((err / tol).max()):.3f}, NAR {float((nerr / ntol).max()):.3f}; "
          f"loss AR {float(an.sum()):.2f} (ref {float(ref['ar_nll'].sum()):.2f}) NAR {float(nn_.sum()):.1f} (ref {float(ref['nar_nll'].sum()):.1f})")
    assert bool((err <= tol).all()) and bool((nerr <= ntol).all())
    return an, ak, nn_, nk


def _engine_args(u):
    return u["text"], u["text"], u["codes"].contiguous(), u["P"]


def test_bf16_engine_score_matches_oracle_and_step_path():
    u = sc.utterance(sc.config())
    ref, P = u["ref"], u["P"]
    m = _model(u["cfg"], u["sd"], "bf16")
    e = m.engine()
    an, ak, nn_, nk = _check_bf16(u, e.score(*_engine_args(u)), "bf16")
    T = u["codes"].shape[0] - P
    am = e.read("score_ar_argmax", (T + 1,), torch.int32).long()
    agree = float((am == ref["ar_argmax"]).float().mean())
    # the NAR stages' argmax through the same driver (vx_nar_ex with the same forced codes) and its consistency with the rank
    nar_codes = e.nar(u["text"], u["codes"][:P].contiguous(), u["codes"][P:, 0].contiguous(), forced_codes=u["codes"][P:].contiguous()).cpu()
    nar_am = nar_codes[:, 1:].t()
    nagree = (nar_am == ref["nar_argmax"]).float().mean(1)
    assert torch.equal(nk == 0, nar_am == ref["nar_targets"])
    # the row pass against the step path: a forced decode of the same tokens scores the same model
    e.ar_prefill(u["text"], u["codes"][:P, 0].contiguous())
    e.ar_decode(top_k=1, forced=u["codes"][P:, 0].contiguous())
    toks, _, n_pass = e.ar_result()
    assert n_pass == T + 1
    step_am = e.read("ar_argmax", (n_pass,), torch.int32).long()
    sagree = float((am == step_am).float().mean())
    print(f"bf16 argmax agreement: AR vs oracle {agree:.3f}, NAR per stage {[round(float(v), 3) for v in nagree]}, AR row pass vs step path {sagree:.3f}")
    assert agree >= sc.BF16_AGREE_MIN and float(nagree.min()) >= sc.BF16_AGREE_MIN and sagree >= sc.BF16_AGREE_MIN
    assert torch.equal(ak.long() == 0, am == ref["ar_targets"])


# ------------------------------------------------------------------------------------------------ case 5: batch
BATCH_SHAPES = [(6, 64, 3), (9, 65, 1), (4, 30, 29), (3, 129, 60)]  # segment lengths at, over and far under a 64-row boundary; T = 1


def test_bf16_score_batch_matches_oracle_and_single_calls():
    cfg = sc.config()
    us = [sc.utterance(cfg, S=S, A=A, P=P, seed=3 + i) for i, (S, A, P) in enumerate(BATCH_SHAPES)]
    m = _model(cfg, us[0]["sd"], "bf16")
    e = m.engine()
    parts = e.score_batch([u["text"] for u in us], [u["text"] for u in us], [u["codes"].contiguous() for u in us], [u["P"] for u in us])
    res = m.score_batch([(u["x"].cuda(), u["x_lens"].cuda(), u["y"].cuda()) for u in us], prompt_frames=[u["P"] for u in us])
    rows = [u["codes"].shape[0] - u["P"] + 1 for u in us]
    am_all = e.read("score_ar_argmax", (sum(rows),), torch.int32).long().split(rows)  # the batch call's AR rows, concatenated
    nar_all = e.nar_batch([u["text"] for u in us], [u["codes"][: u["P"]].contiguous() for u in us], [u["codes"][u["P"]:, 0].contiguous() for u in us],
                          forced_codes=[u["codes"][u["P"]:].contiguous() for u in us])
    ar_eq = torch.cat([am == u["ref"]["ar_argmax"] for am, u in zip(am_all, us)]).float()
    nar_eq = torch.cat([c.cpu()[:, 1:].t() == u["ref"]["nar_argmax"] for c, u in zip(nar_all, us)], 1).float()
    print(f"batch argmax agreement with the oracle: AR {float(ar_eq.mean()):.3f}, NAR per stage {[round(float(v), 3) for v in nar_eq.mean(1)]}")
    assert float(ar_eq.mean()) >= sc.BF16_AGREE_MIN and float(nar_eq.mean(1).min()) >= sc.BF16_AGREE_MIN
    for i, (u, p) in enumerate(zip(us, parts)):
        an, ak, nn_, nk = _check_bf16(u, p, f"batch utterance {i} {BATCH_SHAPES[i]}")
        assert torch.equal(ak.long() == 0, am_all[i] == u["ref"]["ar_targets"])
        assert torch.equal(nk == 0, nar_all[i].cpu()[:, 1:].t() == u["ref"]["nar_targets"])
        sa, sk, sn, snk = [t.cpu() for t in e.score(*_engine_args(u))]
        d_ar, d_nar = sc.decided_bf16(u["ref"])
        assert torch.equal(ak[d_ar], sk[d_ar]) and torch.equal(nk[d_nar], snk[d_nar])
        assert torch.equal(res[i].ar_nll.cpu(), an) and torch.equal(res[i].nar_rank.cpu(), nk)  # the model-level call is the same pass
        assert res[i].ar_loss == pytest.approx(float(an.double().sum()))


def test_vallf_score_batch_falls_back_to_single_calls():
    from valle_amd.engine import VxError

    cfg = sc.config(model_name="VALL-F", num_quantizers=3, prepend_bos=True)
    us = [sc.utterance(cfg, S=5, A=24, P=3), sc.utterance(cfg, S=4, A=20, P=0, seed=2)]
    m = _model(cfg, us[0]["sd"], "bf16")
    with pytest.raises(VxError) as ei:
        m.engine().score_batch([u["text"] for u in us], [u["text"] for u in us], [u["codes"].contiguous() for u in us], [3, 0])
    assert ei.value.code == 5 and "vx_score" in str(ei.value)
    res = m.score_batch([(u["x"].cuda(), u["x_lens"].cuda(), u["y"].cuda()) for u in us], prompt_frames=[3, 0])
    for u, r in zip(us, res):
        _check_bf16(u, (r.ar_nll, r.ar_rank, r.nar_nll, r.nar_rank), "VALL-F bf16 fallback")


# ------------------------------------------------------------------------------------- case 6: no side effects
def test_score_leaves_decode_state_alone():
    cfg = sc.config()
    us = [sc.utterance(cfg, S=S, A=A, P=P, seed=3 + i) for i, (S, A, P) in enumerate(BATCH_SHAPES[:3])]
    m = _model(cfg, us[0]["sd"], "bf16", max_batch=2)
    e = m.engine()
    third = _engine_args(us[2])

    def session(with_score):
        e.batch_open()
        for slot, new in ((0, 5), (1, 24)):  # slot 0 stops after 5 steps: batch_run(1) returns there, slot 1 mid-utterance
            e.batch_admit([slot], [us[slot]["text"]], [us[slot]["codes"][:8, 0].contiguous()], top_k=5, seeds=[11 + slot], max_new_tokens=new)
        assert e.batch_run(1) == [0]
        a, _ = e.batch_result(0)
        s = e.score(*third) if with_score else None
        assert e.batch_run(1) == [1]
        b, _ = e.batch_result(1)
        return a, b, s

    a0, b0, _ = session(False)
    a1, b1, s = session(True)
    assert a0.numel() == 5 and b0.numel() == 24 and torch.equal(a0, a1) and torch.equal(b0, b1)
    _check_bf16(us[2], s, "score inside a session")

    def batch1(with_score):
        e.ar_prefill(us[0]["text"], us[0]["codes"][:8, 0].contiguous())
        s = e.score(*third) if with_score else None
        e.ar_decode(top_k=5, seed=7, max_new_tokens=20)
        return e.ar_result()[0], s

    t0, _ = batch1(False)
    t1, s1 = batch1(True)
    assert t0.numel() == 20 and torch.equal(t0, t1)
    assert all(torch.equal(x, y) for x, y in zip(s, s1))  # and the score does not depend on what ran before it


def test_score_does_not_depend_on_uninitialised_memory():
    """VX_POISON=1 fills every fresh device allocation (the scoring scratch included) with NaN bytes: no score may change."""
    u = sc.utterance(sc.config())
    got = {}
    for prec in ("fp32", "bf16"):
        e = _model(u["cfg"], u["sd"], prec).engine()
        got[prec] = [t.cpu().flatten().tolist() for t in e.score(*_engine_args(u))]
    ub = [sc.utterance(u["cfg"], S=S, A=A, P=P, seed=3 + i) for i, (S, A, P) in enumerate(BATCH_SHAPES[:2])]
    e = _model(u["cfg"], u["sd"], "bf16").engine()
    got["batch"] = [[t.cpu().flatten().tolist() for t in p] for p in
                    e.score_batch([v["text"] for v in ub], [v["text"] for v in ub], [v["codes"].contiguous() for v in ub], [v["P"] for v in ub])]
    script = (
        "import sys, json, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import score_cases as sc\n"
        "from test_gpu_score import _model, _engine_args, BATCH_SHAPES\n"
        "u = sc.utterance(sc.config()); out = {}\n"
        "for prec in ('fp32', 'bf16'):\n"
        "    out[prec] = [t.cpu().flatten().tolist() for t in _model(u['cfg'], u['sd'], prec).engine().score(*_engine_args(u))]\n"
        "ub = [sc.utterance(u['cfg'], S=S, A=A, P=P, seed=3 + i) for i, (S, A, P) in enumerate(BATCH_SHAPES[:2])]\n"
        "e = _model(u['cfg'], u['sd'], 'bf16').engine()\n"
        "out['batch'] = [[t.cpu().flatten().tolist() for t in p] for p in e.score_batch([v['text'] for v in ub], [v['text'] for v in ub],"
        " [v['codes'].contiguous() for v in ub], [v['P'] for v in ub])]\n"
        "print(json.dumps(out))\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, VX_POISON="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == got


# ----------------------------------------------------------------------------------------------- case 7: fp8nar
def test_fp8nar_score(monkeypatch):
    """VX_MX_MIN_ROWS=1 sends one utterance's NAR rows through the MXFP8 kernels, as test_fp8_nar_stages_teacher_forced does.  A
    logits error within FP8_REL_TOL x the row scale moves a row's nll by at most twice that, so the mean moves by at most
    2 FP8_REL_TOL x the mean row scale - against the oracle, and (the bf16 engine being inside the same band) against bf16."""
    from test_gpu_engine import FP8_REL_TOL

    u = sc.utterance(sc.config())
    bf = [t.cpu() for t in _model(u["cfg"], u["sd"], "bf16").engine().score(*_engine_args(u))]
    monkeypatch.setenv("VX_MX_MIN_ROWS", "1")
    f8 = [t.cpu() for t in _model(u["cfg"], u["sd"], "fp8nar").engine().score(*_engine_args(u))]
    assert bool(torch.isfinite(f8[2]).all())
    bound = 2 * FP8_REL_TOL * float(sc.absmax(u["ref"]["nar_logits"]).mean())
    mean8, mean16, mean_ref = float(f8[2].mean()), float(bf[2].mean()), float(u["ref"]["nar_nll"].mean())
    print(f"fp8nar NAR mean nll {mean8:.3f}, bf16 {mean16:.3f}, oracle {mean_ref:.3f}, bound {bound:.3f}; rows whose rank differs from bf16: "
          f"{float((f8[3] != bf[3]).float().mean()):.3f}")
    assert abs(mean8 - mean16) <= bound and abs(mean8 - mean_ref) <= bound
    assert not torch.equal(f8[2], bf[2])  # the MXFP8 path did run
    assert torch.equal(f8[0].view(torch.int32), bf[0].view(torch.int32)) and torch.equal(f8[1], bf[1])  # fp8nar does not touch the AR stack
