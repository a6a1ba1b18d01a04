"""CPU: the log-probability switch (VX_FLAG_LOGPROBS, ``logprobs=True``) and best-of-N synthesis as far as they can be checked
without a GPU: the flag value, the exported symbols, the struct sizes, the refusals that are answered before any HIP call, the
host mirror's argument checks, GenLogProbs arithmetic and the ranking rule."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import ROOT

NEW_SYMBOLS = ("vx_ar_logprobs", "vx_batch_logprobs", "vx_nar_logprobs", "vx_op_sample_logprob")
VX_ERR_ARG, VX_ERR_UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


def test_flag_value_and_header():
    from valle_amd import engine

    assert engine.VX_FLAG_LOGPROBS == 256
    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    assert re.search(r"\bVX_FLAG_LOGPROBS\s*=\s*256\b", hdr)
    flags = [int(v) for v in re.findall(r"\bVX_FLAG_[A-Z0-9_]+\s*=\s*(\d+)", hdr)]
    assert len(flags) == len(set(flags)) and all(v & (v - 1) == 0 for v in flags)  # distinct single bits


def test_symbols_declared_and_exported(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in engine.declared_symbols(), name
        assert hasattr(lib, name), name
    for meth in ("ar_logprobs", "batch_logprobs", "nar_logprobs", "op_sample_logprob"):
        assert callable(getattr(engine.Engine, meth))


def test_struct_sizes_unchanged():
    from valle_amd.engine import VxConfig, VxDecodeParams

    assert C.sizeof(VxDecodeParams) == 56
    assert C.sizeof(VxConfig) == 16 * 4


def test_entry_points_refuse_before_any_hip_call(lib):
    n = C.c_int32()
    buf = (C.c_float * 4)()
    assert lib.vx_ar_logprobs(None, buf, 4, C.byref(n)) == VX_ERR_ARG
    assert lib.vx_batch_logprobs(None, 0, buf, 4, C.byref(n)) == VX_ERR_ARG
    assert lib.vx_nar_logprobs(None, 0, buf, 4) == VX_ERR_ARG
    out = (C.c_int32 * 2)()
    lp = C.c_float()
    row = (C.c_float * 2048)()
    addr = C.addressof(row)  # never dereferenced: every call below is refused first
    assert lib.vx_op_sample_logprob(None, 1025, 0, 1.0, 0.0, None, out, C.byref(lp), None) == VX_ERR_ARG
    assert lib.vx_op_sample_logprob(addr, 1025, 0, 1.0, 0.0, None, None, C.byref(lp), None) == VX_ERR_ARG
    assert lib.vx_op_sample_logprob(addr, 1025, 0, 1.0, 0.0, None, out, None, None) == VX_ERR_ARG
    assert lib.vx_op_sample_logprob(addr, 1089, 0, 1.0, 0.0, None, out, C.byref(lp), None) == VX_ERR_UNSUPPORTED
    assert b"1088" in lib.vx_last_error()
    assert lib.vx_op_sample_logprob(addr, 1, 0, 1.0, 0.0, None, out, C.byref(lp), None) == VX_ERR_UNSUPPORTED
    assert lib.vx_op_sample_logprob(addr, 1025, 0, 1.0, float("nan"), None, out, C.byref(lp), None) == VX_ERR_ARG
    assert lib.vx_op_sample_logprob(addr, 1025, 0, 1.0, -0.5, None, out, C.byref(lp), None) == VX_ERR_ARG


def test_model_keyword_is_an_engine_option():
    from valle_amd.models import VALLE, VALLF, get_model

    assert VALLE(128, 2, 2).engine_opts["logprobs"] is False
    assert VALLE(128, 2, 2, logprobs=True).engine_opts["logprobs"] is True
    assert VALLF(128, 2, 2, logprobs=True, max_batch=2).engine_opts["logprobs"] is True
    # every configuration the host mirror accepts takes the switch: post-norm + prenets, fp32, fp8 slot caches, batched rows
    VALLE(64, 16, 4, norm_first=False, add_prenet=True, precision="fp32", logprobs=True)
    VALLE(256, 4, 2, max_batch=4, kv_cache="fp8", logprobs=True)
    VALLF(256, 4, 2, max_batch=4, batched_rows=True, logprobs=True)
    params = dict(model_name="VALL-E", decoder_dim=128, nhead=2, num_decoder_layers=2, logprobs=True)
    assert get_model(params).engine_opts["logprobs"] is True


def _utt():
    from valle_amd.weights import synthetic_inputs

    return synthetic_inputs(5, 4, 8, seed=3)


def test_return_logprobs_needs_the_switch():
    """Refused before any engine call: the models below sit on the CPU, where creating an engine would raise RuntimeError."""
    from valle_amd.models import VALLE, VALLF

    x, xl, y = _utt()
    for m in (VALLE(128, 2, 2, max_batch=2), VALLF(128, 2, 2, max_batch=2)):
        with pytest.raises(ValueError, match="logprobs=True"):
            m.inference(x, xl, y, None, return_logprobs=True)
        with pytest.raises(ValueError, match="logprobs=True"):
            m.inference_batch([(x, xl, y)], return_logprobs=True)
        with pytest.raises(ValueError, match="logprobs=True"):
            m.inference_stream([(x, xl, y)], return_logprobs=True)


def test_best_of_refusals():
    from valle_amd.models import VALLE, VALLF

    x, xl, y = _utt()
    with pytest.raises(ValueError, match="logprobs=True"):
        VALLE(128, 2, 2, max_batch=4).inference_best_of(x, xl, y, None, 4)
    with pytest.raises(NotImplementedError, match="max_batch >= 2"):
        VALLE(128, 2, 2, logprobs=True).inference_best_of(x, xl, y, None, 4)
    with pytest.raises(NotImplementedError, match="max_batch >= 2"):
        VALLF(128, 2, 2, logprobs=True).inference_best_of(x, xl, y, None, 4)
    m = VALLE(128, 2, 2, max_batch=4, logprobs=True)
    with pytest.raises(ValueError, match="n must be >= 1"):
        m.inference_best_of(x, xl, y, None, 0)
    with pytest.raises(ValueError, match="seeds"):
        m.inference_best_of(x, xl, y, None, 3, seeds=[1, 2])
    with pytest.raises(ValueError, match="top_p"):
        m.inference_best_of(x, xl, y, None, 3, top_p=0.0)


def test_gen_logprobs_ar_mean():
    from valle_amd.models import GenLogProbs

    ar = torch.tensor([-1.0, -2.0, -6.0, -100.0])
    # stopped on EOS after 2 tokens: 3 passes count, the EOS term included
    assert GenLogProbs(ar[:3], None, 2, 1).ar_mean == pytest.approx(-3.0)
    assert GenLogProbs(ar[:3], None, 2, 2).ar_mean == pytest.approx(-3.0)
    # length / max_new stop: the tokens only, whatever later passes hold
    assert GenLogProbs(ar, None, 2, 3).ar_mean == pytest.approx(-1.5)
    assert GenLogProbs(ar, None, 3, 4).ar_mean == pytest.approx(-3.0)
    assert GenLogProbs(ar[:1], None, 0, 1).ar_mean == pytest.approx(-1.0)  # EOS at the first pass: the EOS term alone
    assert math.isnan(GenLogProbs(ar, None, 0, 4).ar_mean)                 # nothing emitted
    g = GenLogProbs(ar, torch.zeros(7, 3), 3, 4)
    assert g.nar.shape == (7, 3) and g.n_tokens == 3 and g.stop_reason == 4


def test_best_of_ranking_and_ties():
    from valle_amd.models import BestOf, best_of_index

    assert best_of_index([-3.0, -1.0, -2.0]) == 1
    assert best_of_index([-1.0, -3.0, -1.0, -1.0]) == 0          # ties go to the lower index
    assert best_of_index([-5.0, -2.0, -2.0]) == 1
    assert best_of_index([float("nan"), -9.0, float("nan")]) == 1  # a candidate that emitted nothing ranks last
    assert best_of_index([float("nan"), float("nan")]) == 0
    assert best_of_index([-0.5]) == 0
    with pytest.raises(ValueError):
        best_of_index([])
    b = BestOf(1, [7, 8], [-2.0, -1.0], [torch.zeros(3), torch.zeros(4)])
    assert (b.index, b.seeds, b.ar_mean) == (1, [7, 8], [-2.0, -1.0]) and len(b.tokens) == 2
