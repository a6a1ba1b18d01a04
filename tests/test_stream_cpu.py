"""CPU: the continuous-batching entry points (vx_batch_open / _admit / _run) refuse bad arguments before any HIP call, and the
Python surface refuses the models the batched path does not serve."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


def test_session_calls_refuse_a_null_engine(lib):
    from valle_amd.engine import VxDecodeParams

    stopped, n = (C.c_int32 * 4)(), C.c_int32()
    assert lib.vx_batch_open(None, None) == 1
    assert lib.vx_batch_run(None, 1, 0, stopped, C.byref(n), None) == 1
    slots = (C.c_int32 * 1)(0)
    ptrs = (C.c_void_p * 1)(None)
    ints = (C.c_int32 * 1)(4)
    params = (VxDecodeParams * 1)()
    assert lib.vx_batch_admit(None, 1, slots, ptrs, ints, ptrs, ints, params, 0, None) == 1
    assert b"null" in lib.vx_last_error()


def test_admission_modes_exported():
    from valle_amd import engine

    assert (engine.VX_ADMIT_BATCHED, engine.VX_ADMIT_PER_SLOT) == (0, 1)
    for name in ("vx_batch_open", "vx_batch_admit", "vx_batch_run"):
        assert name in engine.declared_symbols()


def test_vallf_has_no_stream():
    from valle_amd.models import VALLF

    m = VALLF(128, 2, 2)
    with pytest.raises(NotImplementedError, match="batch-1"):
        m.inference_stream([])


def test_stream_needs_a_batched_model_on_the_gpu():
    from valle_amd.models import VALLE

    m = VALLE(128, 2, 2).eval()  # on the CPU: no engine, no fallback
    with pytest.raises(RuntimeError, match="MI355X"):
        m.inference_stream([])
