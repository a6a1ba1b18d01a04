"""CPU: VALL-F models with max_batch >= 2 (the batched and continuous decode of the cross-attention variant) are accepted by the
host mirror and by vx_create within their limits - pre-norm, no prenets, head_dim 64, d_model % 128 == 0, bf16 - and refused
loudly outside them, before any HIP call."""
import ctypes as C

import pytest

from valle_amd.models import VALLF, get_model


def _params(**kw):
    p = dict(model_name="VALL-F", decoder_dim=1024, nhead=16, num_decoder_layers=12, scale_factor=1.0, norm_first=True,
             add_prenet=False, prefix_mode=1, share_embedding=True, prepend_bos=False, num_quantizers=8, max_batch=4)
    p.update(kw)
    return p


def test_vallf_with_slots_constructs():
    m = VALLF(256, 4, 2, max_batch=4)
    assert m.engine_opts["max_batch"] == 4 and m.cfg.is_vallf
    g = get_model(_params())
    assert type(g) is VALLF and g.engine_opts["max_batch"] == 4
    with pytest.raises(AttributeError):  # VALLF.continual stays absent
        g.continual(None, None, None)


@pytest.mark.parametrize("args,kw", [
    ((256, 4, 2), dict(norm_first=False)),
    ((256, 4, 2), dict(add_prenet=True)),
    ((256, 4, 2), dict(kv_cache="fp8")),
    ((256, 4, 2), dict(precision="fp32")),
    ((256, 8, 2), dict()),   # head_dim 32
    ((192, 3, 2), dict()),   # head_dim 64, d_model % 128 != 0
    ((64, 1, 2), dict()),    # head_dim 64, d_model 64
])
def test_vallf_with_slots_refuses_outside_its_limits(args, kw):
    with pytest.raises(NotImplementedError):
        VALLF(*args, max_batch=4, **kw)


def test_vallf_without_slots_keeps_refusing_the_batched_entry_points():
    m = VALLF(256, 4, 2)
    with pytest.raises(NotImplementedError):
        m.inference_batch([])
    with pytest.raises(NotImplementedError):
        m.inference_stream([])


def _cfg(flags, d=256, nhead=4, prec=1, max_batch=4):
    from valle_amd.engine import VxConfig

    c = VxConfig()
    c.struct_size = C.sizeof(VxConfig)
    c.d_model, c.nhead, c.num_layers = d, nhead, 2
    c.nar_d_model, c.nar_nhead, c.nar_num_layers = d, nhead, 2
    c.num_quantizers, c.prefix_mode, c.precision, c.max_text, c.max_audio = 8, 1, prec, 16, 64
    c.flags, c.max_batch = flags, max_batch
    return c


def test_vx_create_accepts_vallf_slots_and_refuses_the_rest():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine
    from valle_amd.engine import VX_FLAG_KV_FP8, VX_FLAG_POST_NORM, VX_FLAG_PRENET, VX_FLAG_VALLF

    lib = engine.load_library()
    # passes the configuration checks; without a GPU it then fails in its first HIP call (VX_ERR_HIP = 2), not VX_ERR_UNSUPPORTED
    h = C.c_void_p()
    rc = lib.vx_create(C.byref(_cfg(VX_FLAG_VALLF)), C.byref(h))
    if rc == 0:  # a GPU is present: the engine exists
        lib.vx_destroy(h)
    else:
        assert rc == 2, lib.vx_last_error()
    for c in (_cfg(VX_FLAG_VALLF | VX_FLAG_POST_NORM), _cfg(VX_FLAG_VALLF | VX_FLAG_PRENET), _cfg(VX_FLAG_VALLF | VX_FLAG_KV_FP8),
              _cfg(VX_FLAG_VALLF, prec=2), _cfg(VX_FLAG_VALLF, prec=0), _cfg(VX_FLAG_VALLF, d=192, nhead=3)):
        h = C.c_void_p()
        assert lib.vx_create(C.byref(c), C.byref(h)) == 5, lib.vx_last_error()  # VX_ERR_UNSUPPORTED
