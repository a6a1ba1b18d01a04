"""CPU: the C-ABI library builds, loads and exports every symbol include/vallex.h declares
(no compute call is made without a GPU), and the host-side mirror validates arguments like the
reference does."""
import os
import re

import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


def test_header_symbols_exported(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = sorted(set(re.findall(r"\b(vx_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 18
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in vallex.h but not exported"
    assert declared == engine.declared_symbols()  # the ctypes table covers the whole header


def test_struct_sizes_match_header(lib):
    from valle_amd.engine import VxConfig, VxDecodeParams
    import ctypes as C

    assert C.sizeof(VxConfig) == 16 * 4
    assert C.sizeof(VxDecodeParams) == 56


def test_error_reporting_without_gpu(lib):
    import ctypes as C
    from valle_amd.engine import VxConfig

    c = VxConfig()
    c.struct_size = 0  # wrong on purpose: rejected before any HIP call
    h = C.c_void_p()
    assert lib.vx_create(C.byref(c), C.byref(h)) == 1
    assert b"struct_size" in lib.vx_last_error()


def test_geometry_checks_without_gpu(lib):
    """Geometry is validated before any HIP call: head_dim 4..64 (powers of two) is accepted by the Python mirror, anything
    else and batched decode at head_dim != 64 are refused loudly on both sides of the C ABI."""
    import ctypes as C
    from valle_amd.engine import VxConfig
    from valle_amd.models import VALLE

    VALLE(64, 16, 4, norm_first=False, add_prenet=True)  # the reference's own test geometry (valle_test.py:93-95)
    with pytest.raises(NotImplementedError, match="head_dim"):
        VALLE(96, 8, 2)  # head_dim 12
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        VALLE(64, 16, 4, max_batch=4)
    c = VxConfig()
    c.struct_size = C.sizeof(VxConfig)
    c.d_model, c.nhead, c.num_layers = 96, 8, 2
    c.nar_d_model, c.nar_nhead, c.nar_num_layers = 96, 8, 2
    c.num_quantizers, c.prefix_mode, c.precision, c.max_text, c.max_audio = 8, 1, 0, 16, 64
    h = C.c_void_p()
    assert lib.vx_create(C.byref(c), C.byref(h)) != 0
    assert b"head_dim" in lib.vx_last_error()


def test_wrapper_argument_checks_match_reference():
    from valle_amd.models import VALLE

    m = VALLE(128, 2, 2).eval()
    x = torch.randint(3, 50, (1, 6))
    y = torch.randint(0, 1024, (1, 10, 8))
    with pytest.raises(AssertionError):  # valle.py:986
        m.inference(x[0], torch.tensor([6]), y, None)
    with pytest.raises(AssertionError):  # valle.py:989 batch-1 only
        m.inference(x, torch.tensor([6]), y.repeat(2, 1, 1), None)
    with pytest.raises(AssertionError):  # valle.py:991
        m.inference(x, torch.tensor([0]), y, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # product path never falls back to CPU
        m.inference(x, torch.tensor([6], dtype=torch.int32), y, None)


def test_state_dict_strict_loading():
    from valle_amd.config import ModelConfig
    from valle_amd.models import VALLE
    from valle_amd.weights import expected_keys, synthetic_state_dict

    cfg = ModelConfig(decoder_dim=128, nhead=2, num_decoder_layers=2)
    sd = synthetic_state_dict(cfg, 3)
    m = VALLE(128, 2, 2)
    r = m.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    assert list(m.state_dict()) == list(expected_keys(cfg))
    bad = dict(sd)
    bad.pop("ar_predict_layer.weight")
    with pytest.raises(RuntimeError):
        m.load_state_dict(bad, strict=True)
    bad = dict(sd)
    bad["bogus"] = torch.zeros(1)
    with pytest.raises(RuntimeError):
        m.load_state_dict(bad, strict=True)


def test_key_table_is_372_entries_at_baseline_config():
    from valle_amd.config import ModelConfig
    from valle_amd.weights import expected_keys

    keys = expected_keys(ModelConfig())
    assert len(keys) == 372
    n = 0
    seen = set()
    for k, s in keys.items():
        if k.startswith("nar_predict_layers.") and int(k.split(".")[1]) < 6:
            continue  # tied to nar_audio_embeddings.{j+2}
        p = 1
        for v in s:
            p *= v
        n += p
    assert n == 367386628


def _layouts():
    import json

    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "state_dict_layout.json")))


@pytest.mark.parametrize("case", sorted(_layouts()))
def test_state_dict_layout_matches_reference(case):
    """tests/golden/state_dict_layout.json is the reference's own `get_model(params).state_dict()` (names, order, shapes,
    dtypes, tied storage) for each constructor option the build supports (oracle/gen_keys.py): the loader contract of
    bin/infer.py:139-143 (`load_state_dict(checkpoint["model"], strict=True)`)."""
    from valle_amd.config import ModelConfig
    from valle_amd.weights import expected_keys, synthetic_state_dict, tied_keys

    ref = _layouts()[case]
    cfg = ModelConfig(**ref["cfg"])
    want = expected_keys(cfg)
    assert [k for k, _, _ in ref["keys"]] == list(want)  # same names, same order
    for k, shape, dtype in ref["keys"]:
        assert tuple(shape) == tuple(want[k]), k
    sd = synthetic_state_dict(cfg, 0)
    for k, shape, dtype in ref["keys"]:
        assert str(sd[k].dtype).replace("torch.", "") == dtype, k
    assert sorted((a, b) for a, b in ref["shared"]) == sorted(tied_keys(cfg).items())  # valle.py:261-271


def _i32(vals):
    import ctypes as C

    return (C.c_int32 * len(vals))(*vals)


@pytest.mark.parametrize("starts,lens,texts,match", [
    ([0, 96], [64, 10], None, "multiple of 64"),          # unaligned start
    ([0, 64], [100, 10], None, "overlaps"),               # segment 0 runs into segment 1
    ([128, 0], [10, 10], None, "overlaps or precedes"),   # starts out of order
    ([0, 64], [64, 0], None, "empty"),                    # empty segment
    ([0, 64], [64, 200], None, "outside"),                # runs past the buffer (rows = 256)
    ([0, 64], [64, 10], [0, 11], "seg_text"),             # text longer than the segment
    ([0, 64], [64, 10], [-1, 3], "seg_text"),
])
def test_attention_segs_rejects_bad_layout_without_gpu(lib, starts, lens, texts, match):
    """vx_op_attention_segs validates the segment layout on the host before any HIP call (null device pointers are never used)."""
    rc = lib.vx_op_attention_segs(None, None, 256, 4, 64, len(starts), _i32(starts), _i32(lens), None if texts is None else _i32(texts),
                                  None)
    assert rc == 1 and match.encode() in lib.vx_last_error()


def test_attention_segs_rejects_bad_shape_without_gpu(lib):
    one = _i32([0])
    assert lib.vx_op_attention_segs(None, None, 256, 8, 32, 1, one, _i32([64]), None, None) == 5  # head_dim 32: unsupported
    assert b"head_dim" in lib.vx_last_error()
    for nseg in (0, 65):
        z = _i32([64 * i for i in range(max(nseg, 1))])
        assert lib.vx_op_attention_segs(None, None, 65 * 64, 4, 64, nseg, z, _i32([1] * max(nseg, 1)), None, None) == 1
        assert b"nseg" in lib.vx_last_error()


@pytest.mark.parametrize("B,ctx,done,stride,voff,match", [
    (2, [0, 5], None, 4096, 2048, "ctx[0]"),              # empty context on a live slot
    (2, [5, 33], None, 4096, 2048, "ctx[1]"),             # ctx > ctx_max
    (65, [1] * 65, None, 4096, 2048, "B 65"),             # more slots than BMAX
    (0, [1], None, 4096, 2048, "B 0"),
    (2, [5, 5], None, 4096, 2040, "multiples of 16"),     # V offset off the fp8 scale grid
    (2, [5, 5], None, 4100, 2048, "multiples of 16"),
])
def test_attn_slots_rejects_bad_arguments_without_gpu(lib, B, ctx, done, stride, voff, match):
    for fp8 in (0, 1):
        rc = lib.vx_op_attn_slots(fp8, None, None, None if not fp8 else 8, stride, voff, 32, B, 1, _i32(ctx),
                                  None if done is None else _i32(done), None, None)
        assert rc == 1 and match.encode() in lib.vx_last_error(), (fp8, lib.vx_last_error())


def test_attn_slots_done_slots_skip_the_ctx_check_without_gpu(lib):
    """ctx is only checked on live slots (a done slot's ctx is never read); the fp8 form needs its scale bytes."""
    rc = lib.vx_op_attn_slots(0, None, None, None, 4096, 2048, 32, 2, 1, _i32([0, 40]), _i32([1, 0]), None, None)
    assert rc == 1 and b"ctx[1]" in lib.vx_last_error()
    rc = lib.vx_op_attn_slots(1, None, None, None, 4096, 2048, 32, 1, 1, _i32([5]), None, None, None)
    assert rc == 1 and b"kv_scale" in lib.vx_last_error()


# ---- vx_op_bgemm / vx_op_ln_batch: every argument check fires on the host, before any HIP call -----------------------------------
# Every case below is invalid in exactly one way; pointers are passed only where a check further down needs them (never used).
_P = 4096  # a non-null stand-in for a device pointer


def _bgemm(lib, epi=2, kv8=0, A=_P, W=_P, bias=_P, N=256, K=256, B=4, kgroups=1, done=None, row=None, pass_=None, q=_P, kv=_P,
           kv8s=_P, stride=4096, voff=2048, d=0, ctx_max=32, f=_P, part=_P, logits=_P, logits_stride=1088, trace=None, trace_rows=0,
           slot_map=None):
    opt = lambda v: None if v is None else _i32(v)  # noqa: E731
    return lib.vx_op_bgemm(epi, kv8, A, W, bias, N, K, B, kgroups, opt(done), opt(row), opt(pass_), q, kv, kv8s, stride, voff, d,
                           ctx_max, f, part, logits, logits_stride, trace, trace_rows, opt(slot_map), None)


@pytest.mark.parametrize("kw,match", [
    (dict(epi=6), "unknown epilogue"),
    (dict(epi=-1), "unknown epilogue"),
    (dict(epi=2, kv8=1), "kv8"),                                   # fp8 caches outside the QKV epilogue
    (dict(epi=3, kv8=1), "kv8"),
    (dict(B=0), "B 0"),
    (dict(B=65), "B 65"),
    (dict(N=65536), "N 65536"),                                    # (N << 16) | K travels as one kernel argument
    (dict(K=65536 * 2), "K 131072"),
    (dict(N=0), "N 0"),
    (dict(K=384), "K 384"),                                        # ns = 3
    (dict(K=768), "K 768"),                                        # ns = 6
    (dict(K=2048, kgroups=1), "K 2048"),                           # ns = 16
    (dict(K=1024, kgroups=4, epi=3), "kgroups 4"),                 # split K outside BE_PARTIAL: the groups would race
    (dict(K=1024, kgroups=0), "kgroups 0"),
    (dict(K=64), "K 64"),                                          # less than one 128-wide slice
    (dict(A=None), "null A"),
    (dict(W=None), "null A or W"),
    (dict(epi=0, N=768, d=128), "N == 3 d"),                       # QKV N != 3 d
    (dict(epi=0, N=288, K=128, d=96), "d % 64"),                   # QKV d % 64 != 0
    (dict(epi=0, N=768, d=256, q=None), "QKV needs q"),
    (dict(epi=0, N=768, d=256, kv=None), "QKV needs q"),
    (dict(epi=0, kv8=1, N=768, d=256, kv8s=None), "fp8"),
    (dict(epi=0, N=768, d=256, bias=None), "needs bias"),
    (dict(epi=1, bias=None), "needs bias"),
    (dict(epi=5, bias=None), "needs bias"),
    (dict(epi=0, N=768, d=256, ctx_max=0), "ctx_max 0"),
    (dict(epi=0, kv8=1, N=768, d=256, voff=2040), "V offset 2040"),  # off the fp8 scale grid
    (dict(epi=0, N=768, d=256, row=[0, 1, 32, 2]), "row[2]"),       # the KV row past the cache
    (dict(epi=0, N=768, d=256, row=[0, 1, -1, 2]), "row[2]"),
    (dict(epi=1, f=None), "needs f"),
    (dict(epi=5, q=None), "needs q"),
    (dict(epi=2, part=None), "needs part"),
    (dict(epi=3, logits=None), "logits"),
    (dict(epi=3, N=1025, logits_stride=1024), "stride"),
    (dict(epi=3, trace=_P, trace_rows=0), "trace_rows 0"),
    (dict(epi=3, pass_=[0, 0, -3, 0]), "pass[2]"),
    (dict(epi=4, slot_map=None), "needs slot_map"),
    (dict(epi=4, slot_map=[0, 1, 64, 2]), "slot_map[2] = 64"),
    (dict(epi=4, slot_map=[0, -1, 3, 2]), "slot_map[1] = -1"),
])
def test_bgemm_rejects_bad_arguments_without_gpu(lib, kw, match):
    rc = _bgemm(lib, **kw)
    assert rc == 1 and match.encode() in lib.vx_last_error(), (kw, lib.vx_last_error())


def test_bgemm_done_slots_skip_the_row_check_without_gpu(lib):
    """a done slot's KV row is never written, so only live slots' rows are checked"""
    rc = _bgemm(lib, epi=0, N=768, d=256, row=[0, 99, 5, 40], done=[0, 1, 0, 0])
    assert rc == 1 and b"row[3]" in lib.vx_last_error()


def _ln(lib, x=_P, part=_P, kgroups=4, pbias=_P, gamma=_P, beta=_P, h=_P, B=4, d=256, slot_map=None):
    return lib.vx_op_ln_batch(x, part, kgroups, pbias, gamma, beta, h, B, d, None if slot_map is None else _i32(slot_map), None)


@pytest.mark.parametrize("kw,match", [
    (dict(d=258), "d 258"),                  # float4 columns
    (dict(d=1028), "d 1028"),                # 256 threads x 4 columns
    (dict(d=0), "d 0"),
    (dict(B=0), "B 0"),
    (dict(B=65), "B 65"),
    (dict(kgroups=2), "kgroups 2"),
    (dict(kgroups=8), "kgroups 8"),
    (dict(x=None), "null x"),
    (dict(gamma=None), "null x"),
    (dict(beta=None), "null x"),
    (dict(h=None), "null x"),
    (dict(part=None), "needs part"),
    (dict(kgroups=1, pbias=None), "needs part"),
    (dict(kgroups=1, slot_map=[0, 1, 2, 3]), "no partials"),
    (dict(kgroups=0, slot_map=[0, 1, 64, 3]), "slot_map[2] = 64"),
    (dict(kgroups=0, slot_map=[0, 1, 2, -5]), "slot_map[3] = -5"),
])
def test_ln_batch_rejects_bad_arguments_without_gpu(lib, kw, match):
    rc = _ln(lib, **kw)
    assert rc == 1 and match.encode() in lib.vx_last_error(), (kw, lib.vx_last_error())


# ---- vx_op_gemm_partial / vx_op_ln_fold / vx_op_rows_plan: the row path's split-K pieces ------------------------------------------
def _partial(lib, A=_P, W=_P, slabs=_P, M=300, N=256, K=1024, splits=4):
    return lib.vx_op_gemm_partial(A, W, slabs, M, N, K, splits, None)


@pytest.mark.parametrize("kw,rc,match", [
    (dict(A=None), 1, "null operand"),
    (dict(W=None), 1, "null operand"),
    (dict(slabs=None), 1, "null operand"),
    (dict(M=0), 1, "M 0"),
    (dict(N=192), 5, "N 192"),                                     # not whole 128-wide tiles
    (dict(N=0), 5, "N 0"),
    (dict(splits=3), 5, "splits 3"),
    (dict(splits=0), 5, "splits 0"),
    (dict(splits=8), 5, "splits 8"),
    (dict(K=128, splits=4), 5, "K 128"),                           # a slice of 32 k
    (dict(K=192, splits=2), 5, "K 192"),                           # slices of 96 k
    (dict(K=96, splits=1), 5, "K 96"),
    (dict(K=0, splits=1), 5, "K 0"),
])
def test_gemm_partial_rejects_bad_arguments_without_gpu(lib, kw, rc, match):
    assert _partial(lib, **kw) == rc and match.encode() in lib.vx_last_error(), (kw, lib.vx_last_error())


def _fold(lib, prec=1, x=_P, part=_P, nsplit=4, stride=4 * 256, pbias=_P, gamma=_P, beta=_P, ada_w=None, ada_b=None, out=_P, xout=None,
          rows=4, d=256):
    return lib.vx_op_ln_fold(prec, x, part, nsplit, stride, pbias, gamma, beta, ada_w, ada_b, out, xout, rows, d, None)


@pytest.mark.parametrize("kw,rc,match", [
    (dict(d=258), 5, "d 258"),                                     # float4 columns
    (dict(d=1028), 5, "d 1028"),                                   # 4 float4 per lane
    (dict(d=0), 5, "d 0"),
    (dict(prec=2), 1, "prec 2"),
    (dict(x=None), 1, "null x"),
    (dict(rows=0), 1, "rows 0"),
    (dict(nsplit=0), 1, "nsplit 0"),
    (dict(nsplit=5), 1, "nsplit 5"),
    (dict(pbias=None), 1, "needs pbias"),
    (dict(stride=4 * 256 - 1), 1, "part_stride 1023"),             # slabs that overlap
    (dict(out=None, part=None), 1, "needs part"),                  # fold only without anything to fold
    (dict(out=None, xout=_P), 1, "xout needs out"),
    (dict(gamma=None), 1, "gamma and beta"),
    (dict(beta=None), 1, "gamma and beta"),
    (dict(ada_w=_P), 1, "come together"),
    (dict(ada_b=_P), 1, "come together"),
])
def test_ln_fold_rejects_bad_arguments_without_gpu(lib, kw, rc, match):
    assert _fold(lib, **kw) == rc and match.encode() in lib.vx_last_error(), (kw, lib.vx_last_error())


@pytest.mark.parametrize("M,d,want", [
    (1000, 1024, (1, 4, 4)),   # 64 tiles x 4 slices = 256 workgroups: one round
    (1025, 1024, (1, 2, 2)),   # 72 tiles: 4 slices would be two rounds
    (2100, 1024, (1, 1, 1)),   # 136 tiles: no slabs, the GEMM epilogue adds the residual
    (300, 128, (1, 2, 4)),     # K = 128 has two 64-wide slices at most
    (129, 256, (1, 4, 4)),
    (70, 1024, (1, 4, 4)),
    (257, 512, (1, 4, 4)),
    (4095, 128, (1, 2, 4)),
])
def test_rows_plan_table_without_gpu(lib, M, d, want):
    """vx_op_rows_plan with an explicit CU count is the stack's own host function and makes no HIP call."""
    from valle_amd.engine import op_rows_plan

    assert op_rows_plan(M, d, 256) == want
    if M == 2100:
        assert op_rows_plan(M, d, 304) == (1, 2, 2)  # the plan follows the CU count


def test_rows_plan_no_slabs_from_4096_rows_and_bad_arguments_without_gpu(lib):
    import ctypes as C
    from valle_amd.engine import op_rows_plan

    for d in (128, 256, 512, 1024):
        assert op_rows_plan(4096, d, 256)[0] == 0 and op_rows_plan(4095, d, 256)[0] == 1
    assert op_rows_plan(300, 192, 256)[0] == 0  # d % 128 != 0: no split-K form
    out = (C.c_int32 * 3)()
    for args in ((0, 128, 256, out), (300, 0, 256, out), (300, 128, 256, None)):
        assert lib.vx_op_rows_plan(*args) == 1 and b"rows_plan" in lib.vx_last_error()


# ---- batched decode widths: d_model in {128, 256, 512, 1024} ----------------------------------------------------------------------
def _batch_cfg(d, max_batch=4, flags=0):
    import ctypes as C
    from valle_amd.engine import VxConfig

    c = VxConfig()
    c.struct_size = C.sizeof(VxConfig)
    c.d_model, c.nhead, c.num_layers = d, d // 64, 2
    c.nar_d_model, c.nar_nhead, c.nar_num_layers = d, d // 64, 2
    c.num_quantizers, c.prefix_mode, c.precision, c.max_text, c.max_audio = 8, 1, 1, 16, 64
    c.flags, c.max_batch = flags, max_batch
    return c


@pytest.mark.parametrize("d", [384, 640, 768, 896])
def test_vx_create_refuses_batched_widths_without_a_bgemm_form(lib, d):
    """head_dim 64 and d % 128 == 0, but K = d (or 4 d) needs 3, 5, 6 or 7 steps per wave: refused up front (it used to construct and
    fail at the first batched step with 'bgemm: 6 steps per wave').  Batch-1 engines of these widths stay accepted."""
    import ctypes as C
    from valle_amd.engine import VX_FLAG_VALLF

    for flags in (0, VX_FLAG_VALLF):
        h = C.c_void_p()
        assert lib.vx_create(C.byref(_batch_cfg(d, flags=flags)), C.byref(h)) == 5, lib.vx_last_error()
        assert b"d_model in {128, 256, 512, 1024}" in lib.vx_last_error()
    h = C.c_void_p()
    rc = lib.vx_create(C.byref(_batch_cfg(d, max_batch=1)), C.byref(h))
    if rc == 0:  # a GPU is present: the engine exists
        lib.vx_destroy(h)
    else:
        assert rc == 2, lib.vx_last_error()  # passes the configuration checks; fails in its first HIP call without a GPU


@pytest.mark.parametrize("d", [128, 256, 512, 1024])
def test_vx_create_accepts_the_batched_widths(lib, d):
    import ctypes as C

    h = C.c_void_p()
    rc = lib.vx_create(C.byref(_batch_cfg(d)), C.byref(h))
    if rc == 0:
        lib.vx_destroy(h)
    else:
        assert rc == 2, lib.vx_last_error()


@pytest.mark.parametrize("d", [384, 640, 768, 896])
def test_host_mirror_refuses_batched_widths_without_a_bgemm_form(d):
    from valle_amd.models import VALLE, VALLF

    for cls in (VALLE, VALLF):
        with pytest.raises(NotImplementedError, match="d_model in"):
            cls(d, d // 64, 2, max_batch=4)
        cls(d, d // 64, 2)  # batch-1: accepted
    with pytest.raises(NotImplementedError, match="d_model in"):
        VALLE(d, d // 64, 2, max_batch=4, kv_cache="fp8")
    for d_ok in (128, 256, 512, 1024):
        VALLE(d_ok, d_ok // 64, 2, max_batch=4)
        VALLF(d_ok, d_ok // 64, 2, max_batch=4)


# ---- the batch-1 KV cache tap ("ar_kv") --------------------------------------------------------------------------------------------
def test_ar_kv_tap_size_without_gpu(lib):
    """vx_read_buffer's "ar_kv" ([layer][K|V][head][max_text + max_audio][head_dim], fp32 on fp32 engines, else bf16) spans exactly
    the cache: vx_buffer_bytes gives the size its range check uses, and Engine.read_ar_kv asks for exactly that many bytes.  Names
    without a configuration-sized tap, and a bad struct, are refused before any HIP call."""
    import ctypes as C
    from valle_amd.config import ModelConfig
    from valle_amd.engine import VX_PREC_BF16, VX_PREC_F32, VX_PREC_FP8_NAR, Engine, VxConfig

    c = VxConfig()
    c.struct_size = C.sizeof(VxConfig)
    c.d_model, c.nhead, c.num_layers, c.max_text, c.max_audio = 512, 8, 3, 40, 1000
    n = C.c_int64()
    for prec, esz in ((VX_PREC_F32, 4), (VX_PREC_BF16, 2), (VX_PREC_FP8_NAR, 2)):
        c.precision = prec
        assert lib.vx_buffer_bytes(C.byref(c), b"ar_kv", C.byref(n)) == 0, lib.vx_last_error()
        assert n.value == 3 * 2 * 8 * 1040 * 64 * esz
    for bad in (b"ar_kv_", b"batch_kv", b"ar_logits"):
        assert lib.vx_buffer_bytes(C.byref(c), bad, C.byref(n)) == 1
        assert bad in lib.vx_last_error()
    c.struct_size = 0
    assert lib.vx_buffer_bytes(C.byref(c), b"ar_kv", C.byref(n)) == 1
    assert b"struct_size" in lib.vx_last_error()

    class Tap:  # records what the reader asks vx_read_buffer for
        def vx_read_buffer(self, h, name, dst, off, nbytes):
            self.call = (name, off, nbytes)
            return 0

    for precision, dtype, prec in (("fp32", torch.float32, VX_PREC_F32), ("bf16", torch.bfloat16, VX_PREC_BF16)):
        e = Engine.__new__(Engine)
        e.lib, e.h, e.precision, e.max_text, e.max_audio = Tap(), None, precision, 40, 1000
        e.cfg = ModelConfig(decoder_dim=512, nhead=8, num_decoder_layers=3)
        kv = e.read_ar_kv()
        assert kv.shape == (3, 2, 8, 1040, 64) and kv.dtype == dtype
        c.struct_size, c.precision = C.sizeof(VxConfig), prec
        assert lib.vx_buffer_bytes(C.byref(c), b"ar_kv", C.byref(n)) == 0
        assert e.lib.call == (b"ar_kv", 0, n.value)


def test_ar_mem_tap_size_without_gpu(lib):
    """vx_read_buffer's "ar_mem" ([layer][K|V][head][max_text][head_dim], the cache's element type) is the VALL-F text memory:
    vx_buffer_bytes gives the size its range check uses on a configuration with VX_FLAG_VALLF and refuses the name on any other,
    and Engine.read_ar_mem asks for exactly that many bytes."""
    import ctypes as C
    from valle_amd.config import ModelConfig
    from valle_amd.engine import VX_FLAG_VALLF, VX_PREC_BF16, VX_PREC_F32, Engine, VxConfig

    c = VxConfig()
    c.struct_size = C.sizeof(VxConfig)
    c.d_model, c.nhead, c.num_layers, c.max_text, c.max_audio = 512, 8, 3, 40, 1000
    n = C.c_int64()
    for prec, esz in ((VX_PREC_F32, 4), (VX_PREC_BF16, 2)):
        c.precision, c.flags = prec, VX_FLAG_VALLF
        assert lib.vx_buffer_bytes(C.byref(c), b"ar_mem", C.byref(n)) == 0, lib.vx_last_error()
        assert n.value == 3 * 2 * 8 * 40 * 64 * esz
        assert lib.vx_buffer_bytes(C.byref(c), b"ar_kv", C.byref(n)) == 0  # the cache tap is unchanged by the flag
        assert n.value == 3 * 2 * 8 * 1040 * 64 * esz
        c.flags = 0  # a VALL-E configuration has no text memory
        assert lib.vx_buffer_bytes(C.byref(c), b"ar_mem", C.byref(n)) == 1
        assert b"ar_mem" in lib.vx_last_error()
    c.flags = VX_FLAG_VALLF
    for bad in (b"ar_mem_", b"ar_me", b"nar_mem"):
        assert lib.vx_buffer_bytes(C.byref(c), bad, C.byref(n)) == 1
        assert bad in lib.vx_last_error()

    class Tap:  # records what the reader asks vx_read_buffer for
        def vx_read_buffer(self, h, name, dst, off, nbytes):
            self.call = (name, off, nbytes)
            return 0

    for precision, dtype, prec in (("fp32", torch.float32, VX_PREC_F32), ("bf16", torch.bfloat16, VX_PREC_BF16)):
        e = Engine.__new__(Engine)
        e.lib, e.h, e.precision, e.max_text, e.max_audio = Tap(), None, precision, 40, 1000
        e.cfg = ModelConfig(model_name="VALL-F", decoder_dim=512, nhead=8, num_decoder_layers=3)
        mem = e.read_ar_mem()
        assert mem.shape == (3, 2, 8, 40, 64) and mem.dtype == dtype
        c.precision = prec
        assert lib.vx_buffer_bytes(C.byref(c), b"ar_mem", C.byref(n)) == 0
        assert e.lib.call == (b"ar_mem", 0, n.value)
