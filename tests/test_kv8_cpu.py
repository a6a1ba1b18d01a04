"""CPU: the fp8 slot-cache format (tests/kv8_ref.py, VX_FLAG_KV_FP8) - scale rule edge cases, code range, round-trip error, a
live regeneration of a committed kv8 fixture - and the refusal of unsupported configurations by VALLE and by vx_create (before
any HIP call)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from kv8_ref import KV8_EMU_ERR_MAX, KV8_TOL, kv8_dequant, kv8_quant, kv8_scale_bytes

FIXTURES = ["cfg0_greedy", "cfg0_topk10", "cfg1_topk10", "cfg4_s94_topk10"]


def _block(vals):
    x = torch.zeros(16)
    x[: len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return x.to(torch.bfloat16).float()


def test_scale_rule_edge_cases():
    # amax = 0: byte 0, every code 0
    q, s = kv8_quant(torch.zeros(2, 64))
    assert int(s.max()) == 0 and int(q.max()) == 0
    # amax exactly 448 * 2^k: that k's byte (no clipping, no spare binade); just above it: one more
    for k in (-20, -3, 0, 5, 30):
        exact = 448.0 * 2.0**k
        q, s = kv8_quant(_block([exact, -1.0 * 2.0**k]))
        assert int(s[0]) == 127 + k
        assert float(kv8_dequant(q, s)[0]) == exact
        above = 452.0 * 2.0**k  # the next bf16 value up
        q, s = kv8_quant(_block([above]))
        assert int(s[0]) == 128 + k
        assert float(kv8_dequant(q, s)[0]) == pytest.approx(above, rel=2**-4)
    # the MX rule's byte (max(E, 8) - 8) where amax <= 1.75 * 2^(E - 127); one more above that
    for amax, byte in ((1.0, 119), (1.75, 119), (1.7578125, 120), (3.5, 120), (3.9921875, 121)):
        assert int(kv8_scale_bytes(torch.tensor([amax]))[0]) == byte, amax
    # subnormal bf16 values: byte 0 (2^-127), codes still exact where e4m3 can hold them
    tiny = torch.tensor([2.0**-130, -(2.0**-128), 2.0**-133], dtype=torch.float32)
    q, s = kv8_quant(_block(tiny.tolist()))
    assert int(s[0]) == 0
    assert torch.equal(kv8_dequant(q, s)[:3], tiny)
    # mixed signs: the sign survives, the magnitude sets the scale
    x = _block([-3.0, 2.0, -0.5, 0.25, 1.0])
    q, s = kv8_quant(x)
    assert torch.equal(kv8_dequant(q, s), x)


def test_codes_in_range_and_round_trip_error():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 8, 64, generator=g) * torch.exp(torch.randn(64, 8, 1, generator=g) * 6)  # blocks over many binades
    x[3, 2, 16:32] = 0.0
    x = x.to(torch.bfloat16).float()
    q, s = kv8_quant(x)
    v = q.view(torch.float8_e4m3fn).float()
    assert torch.isfinite(v).all() and float(v.abs().max()) <= 448.0
    assert int(s.max()) <= 254
    err = (kv8_dequant(q, s) - x).abs().reshape(64, 8, 4, 16).amax(-1)
    amax = x.abs().reshape(64, 8, 4, 16).amax(-1)
    assert bool((err <= amax * 2.0**-4).all())


def test_fixture_regenerates_and_error_stays_below_tolerance():
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "tools"))
    from gen_kv8_golden import kv8_case

    steps, got, plain, rel = kv8_case("cfg0_greedy")
    z = np.load(os.path.join(GOLDEN, "kv8", "cfg0_greedy.npz"))
    assert np.array_equal(steps, z["probe_steps"])
    np.testing.assert_allclose(got, z["kv8_logits"], rtol=0, atol=1e-5 * float(np.abs(plain).max()))
    assert float(rel.max()) <= KV8_EMU_ERR_MAX
    for name in FIXTURES:
        z = np.load(os.path.join(GOLDEN, "kv8", name + ".npz"))
        assert float(z["rel_err"].max()) <= KV8_EMU_ERR_MAX, name
        assert float(z["rel_err"][0]) <= 1e-6, name  # pass 0: the prefill attends over its own unquantised rows
    assert KV8_TOL >= 0.03 + 4 * KV8_EMU_ERR_MAX


def test_valle_refuses_unsupported_kv_fp8():
    from valle_amd.models import VALLE

    VALLE(256, 4, 2, max_batch=4, kv_cache="fp8")
    VALLE(256, 4, 2, max_batch=4, kv_cache="fp8", precision="fp8nar")
    VALLE(256, 4, 2, kv_cache="bf16")
    with pytest.raises(ValueError):
        VALLE(256, 4, 2, max_batch=4, kv_cache="int8")
    for kw in (dict(max_batch=1), dict(max_batch=0), dict(max_batch=4, precision="fp32"), dict(max_batch=4, norm_first=False),
               dict(max_batch=4, add_prenet=True)):
        with pytest.raises(NotImplementedError):
            VALLE(256, 4, 2, kv_cache="fp8", **kw)
    with pytest.raises(NotImplementedError):
        VALLE(256, 8, 2, max_batch=4, kv_cache="fp8")  # head_dim 32


def test_get_model_and_cli_forward_kv_cache():
    import argparse

    from valle_amd.config import add_model_arguments
    from valle_amd.models import get_model

    p = argparse.ArgumentParser()
    add_model_arguments(p)
    args = p.parse_args(["--decoder-dim", "256", "--nhead", "4", "--num-decoder-layers", "2", "--kv-cache", "fp8"])
    assert args.kv_cache == "fp8"
    args.max_batch = 4
    m = get_model(args)
    assert m.engine_opts["kv_cache"] == "fp8" and m.engine_opts["max_batch"] == 4
    args.max_batch = 0
    with pytest.raises(NotImplementedError):
        get_model(args)
    assert p.parse_args([]).kv_cache is None  # not given: get_model keeps the bf16 default


def test_vx_create_refuses_kv_fp8_before_any_hip_call():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine
    from valle_amd.engine import VX_FLAG_KV_FP8, VX_FLAG_POST_NORM, VX_FLAG_PRENET, VX_FLAG_VALLF, VxConfig

    lib = engine.load_library()

    def cfg(d=256, nhead=4, prec=1, flags=VX_FLAG_KV_FP8, max_batch=4):
        c = VxConfig()
        c.struct_size = C.sizeof(VxConfig)
        c.d_model, c.nhead, c.num_layers = d, nhead, 2
        c.nar_d_model, c.nar_nhead, c.nar_num_layers = d, nhead, 2
        c.num_quantizers, c.prefix_mode, c.precision, c.max_text, c.max_audio = 8, 1, prec, 16, 64
        c.flags, c.max_batch = flags, max_batch
        return c

    # without a GPU a config that passed the checks would fail in its first HIP call (VX_ERR_HIP) instead
    for c in (cfg(max_batch=1), cfg(max_batch=0)):  # batch-1 engines: only the new check refuses them
        h = C.c_void_p()
        assert lib.vx_create(C.byref(c), C.byref(h)) == 5  # VX_ERR_UNSUPPORTED
        assert b"VX_FLAG_KV_FP8" in lib.vx_last_error()
    for c in (cfg(prec=0), cfg(d=256, nhead=8), cfg(flags=VX_FLAG_KV_FP8 | VX_FLAG_POST_NORM),
              cfg(flags=VX_FLAG_KV_FP8 | VX_FLAG_PRENET), cfg(flags=VX_FLAG_KV_FP8 | VX_FLAG_VALLF)):
        h = C.c_void_p()
        assert lib.vx_create(C.byref(c), C.byref(h)) == 5, lib.vx_last_error()
