"""CPU: the nucleus (top-p) filter.  The restatement the GPU tests use (tests/topp_ref.py) reproduces the reference's own
kept masks (tests/golden/topp, written by tools/gen_topp_golden.py from the unmodified top_k_top_p_filtering) on every
decided (row, case); the C struct keeps its size with the new field; the Python entry points refuse top_p outside (0, 1]."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import topp_ref
from conftest import GOLDEN

TOPP = os.path.join(GOLDEN, "topp")
MARGIN = 1e-6


def _cases(tag):
    rows = np.load(os.path.join(TOPP, "rows.npz"))
    z = np.load(os.path.join(TOPP, f"cases_{tag}.npz"))
    V = rows["logits"].shape[1]
    masks = np.unpackbits(z["masks"], axis=-1)[..., :V].astype(bool)
    return torch.from_numpy(rows["logits"]), z, masks


@pytest.mark.parametrize("tag", ["t100", "t070"])
def test_restatement_reproduces_reference_masks(tag):
    logits, z, masks = _cases(tag)
    temp = float(z["temperature"])
    decided = z["margin"] > MARGIN
    assert decided.mean() >= 0.95, decided.mean()
    for c, (tp, tk) in enumerate(zip(z["top_p"], z["top_k"])):
        got = topp_ref.kept_mask(logits, int(tk), temp, float(tp)).numpy()
        for r in np.nonzero(decided[:, c])[0]:
            assert np.array_equal(got[r], masks[r, c]), (tag, r, float(tp), int(tk))
        # undecided rows: the tie rule keeps a superset of the reference's mask (never fewer tokens, never a top-k reject)
        for r in np.nonzero(~decided[:, c])[0]:
            k_only = topp_ref.kept_mask(logits[r], int(tk), temp, 1.0).numpy()
            assert not (masks[r, c] & ~k_only).any()
            assert (got[r] <= k_only).all()


def test_restated_sampling_matches_oracle_with_top_p_off():
    from oracle import valle_oracle as vo

    g = torch.Generator().manual_seed(3)
    for top_k, temp in [(-100, 1.0), (10, 1.0), (1, 0.7), (64, 0.7)]:
        x = torch.randn(1, 1025, generator=g) * 3
        q = torch.empty(1, 1025).exponential_(1, generator=g)
        assert torch.equal(topp_ref.topk_sampling(x.clone(), top_k, temp, q), vo.topk_sampling(x.clone(), top_k, temp, q))


def test_top_p_keeps_position_zero_and_top_k_rejects():
    x = torch.tensor([5.0, 4.0, 4.0, 1.0, 0.0, -3.0])
    assert topp_ref.kept_mask(x, -100, 1.0, 1e-4).tolist() == [True, False, False, False, False, False]
    # the boundary falls on a run of equal logits: the whole run is kept
    assert topp_ref.kept_mask(x, -100, 1.0, 0.75).tolist() == [True, True, True, False, False, False]
    # top-k removed entries never come back, whatever top_p
    assert topp_ref.kept_mask(x, 1, 1.0, 0.999).tolist() == [True, False, False, False, False, False]


def test_decode_params_layout():
    from valle_amd.engine import VxDecodeParams, _struct_top_p

    assert C.sizeof(VxDecodeParams) == 56
    assert VxDecodeParams.top_p.offset == 52
    assert VxDecodeParams.n_forced.offset == 48
    assert _struct_top_p(1.0) == 0.0 and _struct_top_p(0.9) == pytest.approx(0.9)
    assert VxDecodeParams().top_p == 0.0  # zero-filled: off


def test_decode_params_arrays_carry_top_p_per_slot():
    from valle_amd.engine import Engine

    arr, _ = Engine._decode_params(3, [10, -100, 5], 1.0, None, None, None, -1, [1.0, 0.9, 0.5])
    assert [arr[i].top_k for i in range(3)] == [10, -100, 5]
    assert arr[0].top_p == 0.0 and arr[1].top_p == pytest.approx(0.9) and arr[2].top_p == pytest.approx(0.5)
    arr, _ = Engine._decode_params(2, -100, 1.0, None, None, None, -1)
    assert arr[0].top_p == 0.0 and arr[1].top_p == 0.0


@pytest.mark.parametrize("bad", [0.0, -0.1, 1.5, float("nan"), "x"])
def test_python_entry_points_refuse_top_p_outside_unit_interval(bad):
    from valle_amd.models import VALLE, VALLF

    x = torch.randint(3, 50, (1, 6))
    xl = torch.tensor([6])
    y = torch.randint(0, 1024, (1, 10, 8))
    m = VALLE(128, 2, 2).eval()  # on the CPU: the check comes before any engine exists
    with pytest.raises(ValueError, match="top_p"):
        m.inference(x, xl, y, None, top_p=bad)
    with pytest.raises(ValueError, match="top_p"):
        m.inference_batch([(x, xl, y)], top_p=bad)
    with pytest.raises(ValueError, match="top_p"):
        m.inference_stream([(x, xl, y)], top_p=bad)
    f = VALLF(128, 2, 2, max_batch=4, precision="bf16").eval()
    with pytest.raises(ValueError, match="top_p"):
        f.inference_batch([(x, xl, y)], top_p=bad)
    with pytest.raises(ValueError, match="top_p"):
        f.inference_stream([(x, xl, y)], top_p=bad)


def test_engine_refuses_nan_and_negative_top_p_before_any_hip_call():
    """vx_op_sample_topp reads the value first: NaN / negative are VX_ERR_ARG even with null pointers and no GPU."""
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    lib = engine.load_library()
    out = (C.c_int32 * 2)()
    for bad in (float("nan"), -0.5):
        assert lib.vx_op_sample_topp(C.c_void_p(16), 1025, 10, 1.0, bad, None, out, None) == 1
        assert b"top_p" in lib.vx_last_error()
