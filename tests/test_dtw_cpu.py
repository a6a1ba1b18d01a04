"""No GPU: the restatement of dynamic time warping (tests/dtw_ref.py), the host side of the C ABI (vx_dtw_*) and the Python
surface of valle_amd.dtw.

* known answers on the reference: B = A, B = A with every row twice, a constant matrix, the tie rule on a hand-made matrix, the
  anti-diagonal formulation against the cell-by-cell one, the DCT table's orthonormality;
* vx_dtw_create / vx_dtw_compare / vx_op_dtw_* refuse what the header says they refuse, in its order, without any HIP call;
* DTW, DTWResult, mel_cepstral_distortion, mel_distance(warp=): shapes, the ValueError cases, no CPU fallback, and
  mel_distance(a, b) unchanged without warp."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import dtw_ref as DR
from conftest import ROOT
from valle_amd.dtw import DTW, DTWResult, MCD_DB, mel_cepstral_distortion
from valle_amd.engine import VxDtwConfig, VxError
from valle_amd.fbank import mel_distance


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


def _cells(path):
    return [tuple(c) for c in path.tolist()]


# ---- 1. the reference ----------------------------------------------------------------------------------------------------------
def test_identical_sequences_cost_nothing_and_take_the_diagonal():
    A = DR.make_feats(37, 100, 1)
    for n_ceps in (13, 0):
        for dtype in (np.float64, np.float32):
            cost, total, path = DR.chain(A, A, n_ceps, dtype)
            assert total == 0.0 and np.array_equal(path, np.stack([np.arange(37)] * 2, 1))
            assert float(np.diag(cost).max()) == 0.0 and float(cost[0, 1]) > 0


def test_doubled_rows_cost_nothing():
    A = DR.make_feats(21, 100, 2)
    B = np.repeat(A, 2, axis=0)
    for n_ceps in (13, 0):
        _, total, path = DR.chain(A, B, n_ceps)
        k = np.arange(42)
        assert total == 0.0 and np.array_equal(path, np.stack([k // 2, k], 1))
        _, total, path = DR.chain(B, A, n_ceps)
        assert total == 0.0 and DR.path_is_valid(path, 42, 21) and len(path) == 42


def test_constant_matrix():
    total, path = DR.warp(np.ones((5, 9), dtype=np.float32))
    assert total == 9.0
    assert _cells(path) == [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 5), (2, 6), (3, 7), (4, 8)]
    total, path = DR.warp(np.ones((9, 5)))
    assert total == 9.0 and _cells(path) == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 1), (6, 2), (7, 3), (8, 4)]
    assert DR.warp(np.full((1, 1), 2.5))[0] == 2.5 and _cells(DR.warp(np.full((1, 1), 2.5))[1]) == [(0, 0)]
    assert DR.warp(np.ones((1, 7)))[0] == 7.0 and _cells(DR.warp(np.ones((7, 1)))[1]) == [(i, 0) for i in range(7)]


def test_tie_rule():
    # all three predecessors of (1, 1) equal -> diagonal; (i-1, j) and (i, j-1) equal and smaller -> (i-1, j)
    c = np.array([[1.0, 0.0], [0.0, 1.0]])
    assert _cells(DR.warp(c)[1]) == [(0, 0), (1, 1)]           # G: 1 1 / 1 2: all equal
    c = np.array([[2.0, -1.0], [-1.0, 1.0]])
    assert _cells(DR.warp(c)[1]) == [(0, 0), (0, 1), (1, 1)]   # G(0,1) = G(1,0) = 1 < 2: from (i-1, j) = (0, 1)
    c = np.array([[2.0, 0.0], [-1.0, 1.0]])
    assert _cells(DR.warp(c)[1]) == [(0, 0), (1, 0), (1, 1)]   # (i, j-1) strictly smaller


def test_antidiagonals_equal_the_cell_by_cell_recurrence():
    g = np.random.default_rng(5)
    for Ta, Tb in ((1, 1), (1, 6), (6, 1), (2, 2), (7, 19), (19, 7), (23, 23)):
        for cost in (g.random((Ta, Tb), dtype=np.float32), g.integers(0, 3, (Ta, Tb)).astype(np.float32), np.ones((Ta, Tb), np.float32)):
            t0, p0 = DR.warp(cost)
            t1, p1 = DR.warp_loops(cost)
            assert t0 == t1 and np.array_equal(p0, p1) and DR.path_is_valid(p0, Ta, Tb)
            assert DR.path_sum(cost, p0) == t0


def test_dct_table_is_orthonormal_without_its_first_row():
    for D, k in ((100, 13), (5, 4), (128, 127)):
        t = DR.dct_table(D, k)
        assert t.shape == (D, k) and t.dtype == np.float32
        assert float(np.abs(t.astype(np.float64).T @ t.astype(np.float64) - np.eye(k)).max()) < 1e-6
        assert float(np.abs(t.astype(np.float64).sum(0)).max()) < 1e-5  # every kept row is orthogonal to the constant one
    x = DR.make_feats(3, 100, 0)
    assert np.allclose(DR.cepstra(x + 7.5, 13), DR.cepstra(x, 13), atol=1e-4)  # a level change is the 0th coefficient only


def test_fp32_chain_floor_is_small():
    A, B = DR.make_feats(63, 100, 3), DR.make_feats(70, 100, 4)
    c64, t64, _ = DR.chain(A, B, 13)
    c32, t32, _ = DR.chain(A, B, 13, np.float32)
    floor = float(np.abs(c32.astype(np.float64) - c64).max())
    assert c64.dtype == np.float64 and c32.dtype == np.float32 and 0 < floor < 1e-4
    assert abs(t32 - t64) <= (63 + 70 - 1) * floor


# ---- 2. host side of the C ABI -------------------------------------------------------------------------------------------------
def _config(**kw):
    c = VxDtwConfig()
    c.struct_size = C.sizeof(VxDtwConfig)
    c.dim, c.n_ceps, c.max_frames, c.max_batch = 100, 13, 4096, 4
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_symbols(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = set(re.findall(r"\b(vx_[a-z0-9_]+)\s*\(", hdr))
    names = {"vx_dtw_create", "vx_dtw_destroy", "vx_dtw_compare", "vx_op_dtw_cost", "vx_op_dtw_path"}
    assert names <= declared and names <= set(engine.declared_symbols())
    assert all(hasattr(lib, n) for n in names)
    assert C.sizeof(VxDtwConfig) == 20


def test_create_refusals(lib):
    h = C.c_void_p()
    assert lib.vx_dtw_create(C.byref(_config()), None) == 1
    assert lib.vx_dtw_create(None, C.byref(h)) == 1
    for kw, code in (({"struct_size": 0}, 1), ({"struct_size": 24}, 1), ({"max_batch": 0}, 1), ({"max_batch": -2}, 1),
                     ({"max_batch": 0, "dim": 0}, 1),  # the argument errors come first
                     ({"dim": 0}, 5), ({"dim": 129}, 5), ({"n_ceps": -1}, 5), ({"n_ceps": 100}, 5), ({"dim": 1, "n_ceps": 1}, 5),
                     ({"max_frames": 0}, 5), ({"max_frames": 4097}, 5), ({"max_batch": 65}, 5)):
        assert lib.vx_dtw_create(C.byref(_config(**kw)), C.byref(h)) == code, kw
        assert lib.vx_last_error()
    for kw in ({}, {"n_ceps": 0}, {"n_ceps": 99}, {"dim": 1, "n_ceps": 0}, {"dim": 128, "n_ceps": 127}, {"max_frames": 1}, {"max_batch": 64}):
        assert lib.vx_dtw_create(C.byref(_config(**kw)), C.byref(h)) == 0, kw
        lib.vx_dtw_destroy(h)
    lib.vx_dtw_destroy(None)


def test_compare_refusals_before_any_hip_call(lib):
    dtw = DTW(max_frames=300, max_batch=2)  # never moved to a device: no HIP call may be reached
    out = np.zeros(8)

    def code_of(a, Ta, b, Tb, total=out.ctypes.data, length=out.ctypes.data):
        with pytest.raises(VxError) as e:
            dtw._compare_raw(a, Ta, b, Tb, total, length)
        return e.value.code, str(e.value)

    assert code_of([8], [10], [8], [10], total=None)[0] == 1          # null result pointers
    assert code_of([8], [10], [8], [10], length=None)[0] == 1
    assert code_of([8] * 3, [10] * 3, [8] * 3, [10] * 3)[0] == 4      # n > max_batch
    assert code_of([8] * 3, [0] * 3, [0] * 3, [10] * 3)[0] == 4       # ... before any pair is looked at
    assert code_of([0], [10], [8], [10])[0] == 1                      # null input
    assert code_of([8], [10], [0], [10])[0] == 1
    assert code_of([8], [0], [8], [10])[0] == 1                       # no frames
    assert code_of([8], [10], [8], [-4])[0] == 1
    code, msg = code_of([8, 8], [10, 10], [8, 8], [10, 301])          # beyond max_frames: the pair is named
    assert code == 4 and "pair 1" in msg
    assert code_of([8, 8], [301, 10], [8, 8], [10, 0])[0] == 4        # the pairs in order: pair 0's capacity before pair 1's length
    assert code_of([8, 0], [10, 301], [8, 8], [10, 10])[0] == 1       # within a pair: the null pointer before the capacity
    assert dtw._h is not None and dtw._bound is None
    assert lib.vx_dtw_compare(dtw._h, 0, None, None, None, None, None, None, None, None) == 1
    assert lib.vx_dtw_compare(None, 1, None, None, None, None, None, None, None, None) == 1
    dtw.close()
    assert dtw._h is None
    # the test entries
    i64 = (C.c_int64 * 4)
    assert lib.vx_op_dtw_cost(100, 13, None, 1, None, 1, None, None) == 1
    assert lib.vx_op_dtw_cost(100, 100, 8, 1, 8, 1, 8, None) == 1 and lib.vx_op_dtw_cost(129, 0, 8, 1, 8, 1, 8, None) == 1
    assert lib.vx_op_dtw_cost(100, 13, 8, 0, 8, 1, 8, None) == 1 and lib.vx_op_dtw_cost(100, 13, 8, 1, 8, 4097, 8, None) == 1
    assert lib.vx_op_dtw_path(None, 1, i64(1, 1, 0, 0), 8, 8, None, None) == 1
    assert lib.vx_op_dtw_path(8, 0, i64(1, 1, 0, 0), 8, 8, None, None) == 1
    assert lib.vx_op_dtw_path(8, 1, i64(0, 1, 0, 0), 8, 8, None, None) == 1
    assert lib.vx_op_dtw_path(8, 1, i64(1, 1, -1, 0), 8, 8, None, None) == 1
    assert lib.vx_op_dtw_path(8, 1, i64(4097, 1, 0, 0), 8, 8, None, None) == 4


# ---- 3. the Python surface -----------------------------------------------------------------------------------------------------
def test_object_and_result():
    d = DTW()
    assert (d.dim, d.n_ceps, d.max_frames, d.max_batch) == (100, 13, 4096, 64) and d.device.type == "cpu"
    with pytest.raises(VxError) as e:
        DTW(dim=200)
    assert e.value.code == 5
    with pytest.raises(VxError):
        DTW(dim=13, n_ceps=13)
    with pytest.raises(VxError):
        DTW(max_frames=5000)
    r = DTWResult(3.0, 2, 1.5, MCD_DB * 1.5, None)
    assert r.total == 3.0 and r.length == 2 and r.path is None
    assert 6.1418 < MCD_DB < 6.1419 and DR.MCD_DB == MCD_DB
    h = d._h
    assert d.to("cuda:0")._h is h and d.to("cuda:1")._h is h     # never used: nothing is bound yet
    d._bound = torch.device("cuda", 0)
    assert d.to("cuda:1")._h is None and d._handle() is not None
    d.close()
    d.close()


def test_no_cpu_fallback_and_empty_inputs():
    d = DTW()
    a = torch.zeros(4, 100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.compare(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.compare_batch([(a, a)], return_path=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mel_cepstral_distortion(torch.zeros(1000), torch.zeros(1000))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mel_distance(a, a, warp=True)
    with pytest.raises(ValueError):
        mel_cepstral_distortion([], [])
    with pytest.raises(ValueError):
        mel_cepstral_distortion([torch.zeros(1000)], [])
    with pytest.raises(ValueError):
        mel_distance(a, a[:0], warp=True)
    d.device = torch.device("cuda", 0)  # as after .to("cuda:0"): the argument checks come before any device work
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.compare(a, a)                 # host tensors are not moved
    with pytest.raises(AssertionError):
        d.compare(torch.zeros(4, 80, device="meta"), torch.zeros(4, 80, device="meta"))
    d.close()


def test_mel_distance_without_warp_is_unchanged():
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(40, 100, generator=g), torch.randn(33, 100, generator=g)
    want = (a[:33] - b).abs().mean()
    assert torch.equal(mel_distance(a, b), want) and torch.equal(mel_distance(a, b, warp=False), want)
    assert torch.equal(mel_distance(a, b, False), want)
    with pytest.raises(ValueError):
        mel_distance(a, b[:0])
    with pytest.raises(AssertionError):
        mel_distance(a, torch.zeros(4, 2))


def test_public_names():
    import valle_amd

    for n in ("DTW", "DTWResult", "mel_cepstral_distortion", "mel_distance"):
        assert n in valle_amd.__all__ and callable(getattr(valle_amd, n))
    assert math.isclose(MCD_DB, 10 * math.sqrt(2) / math.log(10))
