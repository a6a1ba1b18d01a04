"""CPU: the opt-in VALL-F batched row passes (VX_FLAG_VALLF_ROWS, ``VALLF(..., batched_rows=True)``) are accepted by the host mirror
and by vx_create within the VALL-F slot limits and refused outside them before any HIP call, with a message that names the flag;
vx_op_cross_attention_segs refuses a bad segment / memory layout without a device."""
import ctypes as C

import pytest

from valle_amd.models import VALLE, VALLF, get_model


def _cfg(flags, d=256, nhead=4, prec=1, max_batch=4):
    from valle_amd.engine import VxConfig

    c = VxConfig()
    c.struct_size = C.sizeof(VxConfig)
    c.d_model, c.nhead, c.num_layers = d, nhead, 2
    c.nar_d_model, c.nar_nhead, c.nar_num_layers = d, nhead, 2
    c.num_quantizers, c.prefix_mode, c.precision, c.max_text, c.max_audio = 8, 1, prec, 16, 64
    c.flags, c.max_batch = flags, max_batch
    return c


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


def test_flag_value_and_header_agree():
    import os
    import re

    from valle_amd.engine import VX_FLAG_VALLF_ROWS

    assert VX_FLAG_VALLF_ROWS == 128
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "vallex.h")).read()
    assert re.search(r"VX_FLAG_VALLF_ROWS\s*=\s*128\b", hdr)


def test_vx_create_accepts_the_flag_within_the_vallf_slot_limits(lib):
    from valle_amd.engine import VX_FLAG_VALLF, VX_FLAG_VALLF_ROWS

    h = C.c_void_p()
    rc = lib.vx_create(C.byref(_cfg(VX_FLAG_VALLF | VX_FLAG_VALLF_ROWS)), C.byref(h))
    if rc == 0:  # a GPU is present: the engine exists
        lib.vx_destroy(h)
    else:  # passes the configuration checks; without a GPU it then fails in its first HIP call (VX_ERR_HIP = 2)
        assert rc == 2, lib.vx_last_error()


def test_vx_create_refuses_the_flag_outside_them_naming_it(lib):
    from valle_amd.engine import VX_FLAG_KV_FP8, VX_FLAG_POST_NORM, VX_FLAG_PRENET, VX_FLAG_SIMPLE_ROWS, VX_FLAG_VALLF, VX_FLAG_VALLF_ROWS

    F = VX_FLAG_VALLF | VX_FLAG_VALLF_ROWS
    cases = {
        "without VX_FLAG_VALLF": _cfg(VX_FLAG_VALLF_ROWS),
        "max_batch 1": _cfg(F, max_batch=1),
        "max_batch 0": _cfg(F, max_batch=0),
        "post-norm": _cfg(F | VX_FLAG_POST_NORM),
        "prenet": _cfg(F | VX_FLAG_PRENET),
        "fp32": _cfg(F, prec=0),
        "fp8nar": _cfg(F, prec=2),
        "fp8 slot caches": _cfg(F | VX_FLAG_KV_FP8),
        "simple rows": _cfg(F | VX_FLAG_SIMPLE_ROWS),
        "head_dim 32": _cfg(F, d=256, nhead=8),
    }
    for name, c in cases.items():
        h = C.c_void_p()
        assert lib.vx_create(C.byref(c), C.byref(h)) == 5, (name, lib.vx_last_error())  # VX_ERR_UNSUPPORTED
        assert b"VX_FLAG_VALLF_ROWS" in lib.vx_last_error(), (name, lib.vx_last_error())
        assert not h.value
    # a width the slots do not run at is refused as before (by the rule every max_batch >= 2 engine meets)
    h = C.c_void_p()
    assert lib.vx_create(C.byref(_cfg(F, d=192, nhead=3)), C.byref(h)) == 5, lib.vx_last_error()


def test_host_mirror_option():
    m = VALLF(256, 4, 2, max_batch=4, batched_rows=True)
    assert m.engine_opts["batched_rows"] is True
    assert VALLF(256, 4, 2, max_batch=4).engine_opts["batched_rows"] is False
    p = dict(model_name="VALL-F", decoder_dim=256, nhead=4, num_decoder_layers=2, scale_factor=1.0, norm_first=True, add_prenet=False,
             prefix_mode=1, share_embedding=True, prepend_bos=False, num_quantizers=8, max_batch=4)
    assert get_model(dict(p, batched_rows=True)).engine_opts["batched_rows"] is True
    assert get_model(p).engine_opts["batched_rows"] is False


def test_valle_refuses_batched_rows():
    with pytest.raises(ValueError, match="batched_rows"):
        VALLE(256, 4, 2, max_batch=4, batched_rows=True)
    with pytest.raises(ValueError, match="batched_rows"):
        get_model(dict(model_name="VALL-E", decoder_dim=256, nhead=4, num_decoder_layers=2, max_batch=4, batched_rows=True))
    assert VALLE(256, 4, 2, max_batch=4, batched_rows=False).engine_opts["batched_rows"] is False


@pytest.mark.parametrize("kw", [dict(max_batch=0), dict(max_batch=1), dict(max_batch=4, norm_first=False), dict(max_batch=4, add_prenet=True),
                                dict(max_batch=4, precision="fp32"), dict(max_batch=4, simple_rows=True)])
def test_vallf_refuses_batched_rows_outside_the_slot_limits(kw):
    with pytest.raises(NotImplementedError):
        VALLF(256, 4, 2, batched_rows=True, **kw)


def test_engine_refuses_batched_rows_on_a_valle_config():
    from valle_amd.config import ModelConfig
    from valle_amd.engine import Engine

    with pytest.raises(ValueError, match="batched_rows"):
        Engine(ModelConfig(decoder_dim=256, nhead=4, num_decoder_layers=2), max_batch=4, batched_rows=True)


def _i32(v):
    return (C.c_int32 * len(v))(*v)


def _i64(v):
    return (C.c_int64 * len(v))(*v)


def _call(lib, starts, lens, klens, offs=None, ldq=256, nhead=4, head_stride=128 * 64, v_offset=4 * 128 * 64, rows=512):
    n = len(starts)
    offs = [z * 2 * 4 * 128 * 64 for z in range(n)] if offs is None else offs
    return lib.vx_op_cross_attention_segs(None, ldq, None, _i64(offs), head_stride, v_offset, _i32(klens), None, rows, nhead, n,
                                          _i32(starts), _i32(lens), None)


BAD_LAYOUTS = {
    "start not a multiple of 64": (dict(starts=[0, 100], lens=[64, 10], klens=[5, 5]), "multiple of 64"),
    "overlapping segments": (dict(starts=[0, 64], lens=[65, 10], klens=[5, 5]), "overlaps"),
    "segments out of order": (dict(starts=[128, 0], lens=[10, 10], klens=[5, 5]), "overlaps or precedes"),
    "segment past the rows": (dict(starts=[0, 448], lens=[10, 65], klens=[5, 5]), "outside"),
    "empty segment": (dict(starts=[0], lens=[0], klens=[5]), "empty"),
    "klen 0": (dict(starts=[0, 64], lens=[10, 10], klens=[5, 0]), "klen[1]"),
    "klen > max_text": (dict(starts=[0, 64], lens=[10, 10], klens=[129, 5]), "klen[0]"),
    "nhead * 64 > ldq": (dict(starts=[0], lens=[10], klens=[5], ldq=192), "ldq"),
    "misaligned memory": (dict(starts=[0], lens=[10], klens=[5], offs=[4]), "mem_off[0]"),
    "misaligned V": (dict(starts=[0], lens=[10], klens=[5], v_offset=4 * 128 * 64 + 4), "v_offset"),
}


@pytest.mark.parametrize("name", sorted(BAD_LAYOUTS))
def test_cross_attention_segs_rejects_bad_layout_without_gpu(lib, name):
    """The layout is validated on the host before any HIP call (the null device pointers are never used)."""
    kw, match = BAD_LAYOUTS[name]
    rc = _call(lib, **kw)
    assert rc == 1 and match.encode() in lib.vx_last_error(), (name, rc, lib.vx_last_error())  # VX_ERR_ARG


def test_cross_attention_segs_rejects_bad_counts_without_gpu(lib):
    assert _call(lib, [], [], []) == 1 and b"nseg" in lib.vx_last_error()
    assert _call(lib, [64 * z for z in range(65)], [1] * 65, [1] * 65, rows=65 * 64) == 1 and b"nseg" in lib.vx_last_error()
    assert _call(lib, [0], [10], [5], nhead=0) == 1
