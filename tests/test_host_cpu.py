"""No GPU: the host support the translation units share (csrc/host.hpp).

Every unit reports through the one thread-local message behind vx_last_error(), and a failing HIP call names the unit that made
it, also where DevBuf or CallStage made it on the unit's behalf.  Without a device the first HIP call of each entry fails: the
three small handles (vx_fbank, vx_resampler, vx_dtw) must come out of that failed first use as they went in - the same answer
a second time, a clean destroy - and the op-level entries must give their scratch back.  Where a GPU is present the same calls
succeed (the buffers are then real device memory), so either return code is accepted and the message is checked only on failure."""
import ctypes as C

import pytest
import torch

from valle_amd.engine import VxDtwConfig
from valle_amd.fbank import BigVGANFbank

DEV = "cuda" if torch.cuda.is_available() else "cpu"  # without a GPU the pointers are never dereferenced


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


def _buf(*shape, dtype=torch.float32):
    return torch.ones(*shape, dtype=dtype, device=DEV)


def _twice(lib, call, hip_call, unit):
    """The call, and the identical call again: VX_OK both times with a GPU, VX_ERR_HIP both times without, naming call and unit."""
    seen = []
    for _ in range(2):
        rc = call()
        assert rc in (0, 2), (rc, lib.vx_last_error())
        if rc == 2:
            msg = lib.vx_last_error().decode()
            assert hip_call in msg and " failed: " in msg and unit + ":" in msg, msg
            seen.append(msg)
        else:
            seen.append(None)
    assert seen[0] == seen[1]
    if DEV == "cuda":
        torch.cuda.synchronize()


def test_fbank_first_use_without_a_device_leaves_a_usable_handle(lib):
    fb = BigVGANFbank(max_batch=2)
    wav, out = _buf(300), _buf(1, 100)
    wp, L, op = (C.c_void_p * 1)(wav.data_ptr()), (C.c_int32 * 1)(300), (C.c_void_p * 1)(out.data_ptr())
    _twice(lib, lambda: lib.vx_fbank_extract(fb._h, 1, wp, L, op, None), "hipGetDevice", "fbank.hip")
    assert lib.vx_fbank_extract(fb._h, 3, wp, L, op, None) == 4  # the host-side checks still answer
    fb.close()


def test_resampler_first_use_without_a_device_leaves_a_usable_handle(lib):
    h = C.c_void_p()
    assert lib.vx_resampler_create(16000, 24000, 2, C.byref(h)) == 0
    wav, out = _buf(64), _buf(96)
    ip, ch, L, op = (C.c_void_p * 1)(wav.data_ptr()), (C.c_int32 * 1)(1), (C.c_int32 * 1)(64), (C.c_void_p * 1)(out.data_ptr())
    _twice(lib, lambda: lib.vx_resample(h, 1, ip, ch, L, op, None), "hipGetDevice", "codec.hip")
    assert lib.vx_resample(h, 3, ip, ch, L, op, None) == 4
    lib.vx_resampler_destroy(h)


def test_dtw_first_use_without_a_device_leaves_a_usable_handle(lib):
    c = VxDtwConfig()
    c.struct_size = C.sizeof(VxDtwConfig)
    c.dim, c.n_ceps, c.max_frames, c.max_batch = 8, 3, 16, 2
    h = C.c_void_p()
    assert lib.vx_dtw_create(C.byref(c), C.byref(h)) == 0
    a, b, total, length = _buf(5, 8), _buf(4, 8), _buf(1, dtype=torch.float64), _buf(1, dtype=torch.int32)
    ap, ta, bp, tb = (C.c_void_p * 1)(a.data_ptr()), (C.c_int32 * 1)(5), (C.c_void_p * 1)(b.data_ptr()), (C.c_int32 * 1)(4)
    _twice(lib, lambda: lib.vx_dtw_compare(h, 1, ap, ta, bp, tb, total.data_ptr(), length.data_ptr(), None, None), "hipGetDevice",
           "dtw.hip")
    assert lib.vx_dtw_compare(h, 3, ap, ta, bp, tb, total.data_ptr(), length.data_ptr(), None, None) == 4
    lib.vx_dtw_destroy(h)


def test_op_entries_name_the_failing_call_and_their_unit(lib):
    V = 8
    logits, noise = _buf(V), _buf(V)
    out, lp = (C.c_int32 * 2)(), C.c_float()
    _twice(lib, lambda: lib.vx_op_sample(logits.data_ptr(), V, 2, 1.0, noise.data_ptr(), out, None), "hipMalloc", "engine.hip")
    _twice(lib, lambda: lib.vx_op_sample_topp(logits.data_ptr(), V, 2, 1.0, 0.5, noise.data_ptr(), out, None), "hipMalloc", "engine.hip")
    _twice(lib, lambda: lib.vx_op_sample_logprob(logits.data_ptr(), V, 2, 1.0, 0.5, noise.data_ptr(), out, C.byref(lp), None),
           "hipMalloc", "engine.hip")
    a, b, cost = _buf(5, 8), _buf(4, 8), _buf(5, 4)
    _twice(lib, lambda: lib.vx_op_dtw_cost(8, 3, a.data_ptr(), 5, b.data_ptr(), 4, cost.data_ptr(), None), "hipMalloc", "dtw.hip")
    total, length = _buf(1, dtype=torch.float64), _buf(1, dtype=torch.int32)
    desc = (C.c_int64 * 4)(5, 4, 0, 0)
    _twice(lib, lambda: lib.vx_op_dtw_path(cost.data_ptr(), 1, desc, total.data_ptr(), length.data_ptr(), None, None), "hipMalloc",
           "dtw.hip")
    assert lib.vx_op_sample(logits.data_ptr(), 1, 2, 1.0, noise.data_ptr(), out, None) == 5  # an argument error replaces the message
    assert b"sample: V=1" in lib.vx_last_error()
