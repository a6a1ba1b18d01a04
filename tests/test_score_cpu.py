"""CPU: the scoring entry points exist and refuse bad arguments before any HIP call, the fp64 restatement (score_ref.py) gives
hand-computed values, and the host-side aggregation (sums, EOS-ignoring top-k accuracy) is right.  The checks that need an engine
handle (P range, capacity, not finalised) run in test_gpu_score.py: vx_create needs a device."""
import ctypes as C
import math

import pytest
import torch

import score_ref as sr


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


def test_score_symbols_exist(lib):
    from valle_amd import engine

    for name in ("vx_score", "vx_score_batch", "vx_op_nll_rows"):
        assert hasattr(lib, name) and name in engine.declared_symbols()


@pytest.mark.parametrize("kw,match", [
    (dict(logits=None), "null"), (dict(targets=None), "null"), (dict(nll=None), "null"), (dict(rank=None), "null"),
    (dict(argmax=None), "null"), (dict(rows=0), "rows"), (dict(rows=-3), "rows"), (dict(V=0), "V=0"), (dict(V=1089), "V=1089"),
    (dict(V=1025, ld=1024), "ld=1024"),
])
def test_op_nll_rows_rejects_bad_arguments_without_gpu(lib, kw, match):
    a = dict(logits=8, targets=8, nll=8, rank=8, argmax=8, rows=4, V=1024, ld=1024)  # never dereferenced: refused first
    a.update(kw)
    rc = lib.vx_op_nll_rows(a["logits"], a["rows"], a["V"], a["ld"], a["targets"], a["nll"], a["rank"], a["argmax"], None)
    assert rc == 1 and match.encode() in lib.vx_last_error(), (kw, lib.vx_last_error())


def test_score_entry_points_refuse_a_null_engine_without_gpu(lib):
    assert lib.vx_score(None, None, 0, None, 0, None, 0, 0, None, None, None, None, None) == 1
    assert b"null" in lib.vx_last_error()
    assert lib.vx_score_batch(None, 1, None, None, None, None, None, None, None, None, None, None, None, None) == 1
    assert b"null" in lib.vx_last_error()


def test_score_ref_on_a_hand_made_matrix():
    """3 x 5 logits with a tie at the target's value (row 0), a -inf entry (row 1) and a -inf TARGET entry (row 2)."""
    ninf = float("-inf")
    lg = torch.tensor([[0.0, math.log(2.0), math.log(2.0), 0.0, math.log(3.0)],
                       [ninf, 0.0, math.log(4.0), math.log(4.0), 0.0],
                       [1.0, ninf, 1.0, 0.5, 0.25]], dtype=torch.float64)
    tg = torch.tensor([1, 4, 1])
    nll, rank, am = sr.nll_rank_argmax(lg, tg)
    # row 0: sum exp = 1 + 2 + 2 + 1 + 3 = 9, target value log 2 -> log(9 / 2); entries > log 2: only log 3 (the tie at index 2
    # counts for the target) -> rank 1; argmax 4
    assert abs(float(nll[0]) - math.log(4.5)) < 1e-12 and int(rank[0]) == 1 and int(am[0]) == 4
    # row 1: sum = 0 + 1 + 4 + 4 + 1 = 10, target value 0 -> log 10; entries > 0: the two log 4 -> rank 2 (the other 0 ties);
    # the maximum is tied at 2 and 3: the first index wins
    assert abs(float(nll[1]) - math.log(10.0)) < 1e-12 and int(rank[1]) == 2 and int(am[1]) == 2
    # row 2: the target's entry is -inf -> +inf, not NaN; all four finite entries are greater; first of the tied maxima
    assert float(nll[2]) == float("inf") and int(rank[2]) == 4 and int(am[2]) == 0
    # the same values in fp32 give the same rank / argmax (comparisons on the values as given)
    _, r32, a32 = sr.nll_rank_argmax(lg.float(), tg)
    assert torch.equal(r32, rank) and torch.equal(a32, am)


def test_decided_rule_on_a_hand_made_matrix():
    lg = torch.tensor([[0.0, 1.0, 1.0005, 3.0], [0.0, 1.0, 1.0005, 3.0]])
    tg = torch.tensor([1, 3])
    assert sr.decided(lg, tg, 2e-4).tolist() == [True, True]     # nearest other entry 5e-4 > 2 x 2e-4
    assert sr.decided(lg, tg, 3e-4).tolist() == [False, True]    # 5e-4 < 6e-4: row 0's rank may move
    assert sr.decided(lg, tg, torch.tensor([3e-4, 1.1])).tolist() == [False, False]


def test_aggregation_sums_and_ignores_eos_in_the_accuracy():
    from valle_amd.models import aggregate_score

    ar_nll = torch.tensor([1.0, 2.0, 4.0, 8.0])
    ar_rank = torch.tensor([0, 9, 10, 0], dtype=torch.int32)
    ar_tg = torch.tensor([3, 5, 7, 1024])  # the closing EOS row: in the loss, not in the accuracy
    nar_nll = torch.tensor([[1.0, 1.0, 1.0], [2.0, 3.0, 4.0]])
    nar_rank = torch.tensor([[0, 1, 2], [2, 3, 40]], dtype=torch.int32)
    nar_tg = torch.tensor([[1, 2, 3], [4, 5, 6]])
    r = aggregate_score(ar_nll, ar_rank, ar_tg, nar_nll, nar_rank, nar_tg, top_k=10)
    assert r.ar_loss == 15.0 and r.nar_loss == [3.0, 9.0]
    assert r.ar_topk_acc == pytest.approx(2 / 3)  # ranks 0 and 9 of the three non-EOS rows; rank 10 is outside the top 10
    assert r.nar_topk_acc == [1.0, pytest.approx(2 / 3)]
    r3 = aggregate_score(ar_nll, ar_rank, ar_tg, nar_nll, nar_rank, nar_tg, top_k=3)
    assert r3.ar_topk_acc == pytest.approx(1 / 3) and r3.nar_topk_acc == [1.0, pytest.approx(1 / 3)]
    r1 = aggregate_score(ar_nll, ar_rank, ar_tg, None, None, None)  # Q = 1 models have no NAR part
    assert r1.nar_nll is None and r1.nar_loss is None and r1.nar_topk_acc is None and r1.ar_loss == 15.0


def test_score_checks_its_inputs_like_inference():
    from valle_amd.models import VALLE

    m = VALLE(64, 1, 1, prepend_bos=False, num_quantizers=2, print_eos=False)
    x, xl = torch.zeros((1, 4), dtype=torch.int64), torch.tensor([4])
    y = torch.zeros((1, 6, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match="prompt_frames"):
        m.score(x, xl, y, prompt_frames=6)
    with pytest.raises(ValueError, match="prepend_bos"):
        m.score(x, xl, y, prompt_frames=0)
    with pytest.raises(IndexError):
        m.score(x, xl, y + 1024, prompt_frames=2)
    with pytest.raises(RuntimeError, match="unpadded"):
        m.score(torch.zeros((1, 5), dtype=torch.int64), xl, y, prompt_frames=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the checks passed: only the engine is missing
        m.score(x, xl, y, prompt_frames=2)


def test_oracle_fp32_decides_the_test_utterance():
    """The utterance of test_gpu_score.py's engine cases: the fp32 oracle against the fp64 one decides at least 90 % of the
    AR rows and of the NAR rows under the margin rule, and agrees with it there (so the GPU test's rule is not vacuous)."""
    import score_cases as sc

    for bos in (False, True):
        u = sc.utterance(sc.config(prepend_bos=bos))
        r64 = u["ref"]
        r32 = sr.score(sr.oracle(u["cfg"], u["sd"], torch.float32), u["text"], u["codes"], u["P"])
        d_ar, d_nar = sc.decided_fp32(r64)
        assert float(d_ar.float().mean()) >= 0.9 and float(d_nar.float().mean()) >= 0.9
        assert torch.equal(r32["ar_rank"][d_ar], r64["ar_rank"][d_ar])
        assert torch.equal(r32["nar_rank"][d_nar], r64["nar_rank"][d_nar])
        assert float((r32["ar_nll"] - r64["ar_nll"]).abs().max()) <= 2 * sc.FP32_AR_TOL
