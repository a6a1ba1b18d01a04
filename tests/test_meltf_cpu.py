"""CPU: the mel-spectrogram Transformer (valle/models/transformer.py) - fixtures, key layout, factory, refusals and the C ABI's
argument checks.  No GPU and no compute call.
  * tests/meltf_ref.py (the functional restatement the GPU tests compare against) reproduces the fixtures that
    tools/gen_meltf_golden.py recorded from it after checking it against the unmodified reference class;
  * weights.mel_expected_keys is the reference's state_dict layout (state_dict_layout.json, dumped from the reference);
  * get_model / add_model_arguments accept --model-name Transformer; scaling_xformers=True is refused on both sides of the ABI;
  * header <-> exports <-> ctypes table agree on the vx_mel_* entries;
  * bad arguments are refused before any HIP call."""
import argparse
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from meltf_ref import MelRef

MEL = os.path.join(GOLDEN, "meltf")
FIXTURES = ("a_prenorm", "b_postnorm", "c_hd4_prenet", "d_hd64_stop", "e_d192", "f_stop_first")


def load_fixture(name):
    from valle_amd.config import MelConfig
    from valle_amd.weights import mel_synthetic_state_dict

    z = np.load(os.path.join(MEL, name + ".npz"))
    d, H, L, nf, pn, S = (int(v) for v in z["cfg"])
    cfg = MelConfig(d, H, L, bool(nf), bool(pn))
    sd = mel_synthetic_state_dict(cfg, int(z["weight_seed"]), stop_bias=float(z["stop_bias"]))
    return dict(cfg=cfg, sd=sd, S=S, x=torch.from_numpy(z["x"]), run_frames=torch.from_numpy(z["run_frames"]),
                run_stops=torch.from_numpy(z["run_stops"]), n_frames=int(z["n_frames"]), reason=str(z["reason"]))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_fixture(name):
    """One causal row pass over the recorded frames gives them back, with their stop logits (fp64: 1e-9; the recorded run
    recomputed every row on every pass, so only the order of a few fp64 sums can differ)."""
    f = load_fixture(name)
    c = f["cfg"]
    ref = MelRef(f["sd"], c.d_model, c.nhead, c.num_layers, c.norm_first, c.add_prenet, dtype=torch.float64)
    assert f["run_frames"].shape == (10 * f["S"], 100) and f["run_stops"].shape == (10 * f["S"] + 1,)
    predict, stops = ref.teacher_forced(f["x"], f["run_frames"])
    assert float((predict - f["run_frames"]).abs().max()) < 1e-9
    assert float((stops - f["run_stops"][:-1]).abs().max()) < 1e-9
    assert f["reason"] == ("length" if f["n_frames"] == 10 * f["S"] else "logit")


@pytest.mark.parametrize("name", ("d_hd64_stop", "f_stop_first"))
def test_restatement_stops_where_the_fixture_says(name):
    f = load_fixture(name)
    c = f["cfg"]
    frames, stops, reason = MelRef(f["sd"], c.d_model, c.nhead, c.num_layers, c.norm_first, c.add_prenet, dtype=torch.float32).inference(f["x"])
    assert reason == "logit" and frames.shape == (f["n_frames"], 100) and stops.shape == (f["n_frames"] + 1,)
    assert float((stops.double() - f["run_stops"][: f["n_frames"] + 1]).abs().max()) < 1e-4
    # the fixture's condition: every earlier pass is below -2 tol, the stopping pass above +2 tol (tol: the GPU tests' bf16 bound)
    tol = 0.03 * float(f["run_stops"][: f["n_frames"] + 1].abs().max())
    assert bool((f["run_stops"][: f["n_frames"]] < -2 * tol).all()) and float(f["run_stops"][f["n_frames"]]) > 2 * tol


def test_key_layout_is_the_references():
    from valle_amd.config import MelConfig
    from valle_amd.weights import mel_expected_keys, mel_synthetic_state_dict

    layout = json.load(open(os.path.join(MEL, "state_dict_layout.json")))
    assert len(layout) == 4
    for nf in (True, False):
        for pn in (False, True):
            want = layout[f"d64_h4_l2_norm_first{int(nf)}_add_prenet{int(pn)}"]
            got = mel_expected_keys(MelConfig(64, 4, 2, nf, pn))
            assert list(got) == list(want)
            assert all(tuple(got[k]) == tuple(want[k]) for k in got)
    cfg = MelConfig(64, 4, 2, True, True)
    sd = mel_synthetic_state_dict(cfg, 3, stop_bias=-2.5)
    assert list(sd) == list(mel_expected_keys(cfg)) and float(sd["stop_layer.bias"]) == -2.5
    assert float(sd["encoder_position.alpha"]) != 1.0 and float(sd["decoder_position.alpha"]) != 1.0
    assert float(sd["encoder_position.alpha"]) != float(sd["decoder_position.alpha"])
    assert float(sd["encoder_prenet.2.running_var"].min()) > 0 and float(sd["encoder_prenet.6.running_mean"].abs().max()) > 0
    assert sd["encoder_prenet.2.num_batches_tracked"].dtype == torch.int64


def test_get_model_and_arguments_accept_the_model():
    from valle_amd.models import Transformer, add_model_arguments, get_model

    p = argparse.ArgumentParser()
    add_model_arguments(p)
    a = p.parse_args("--model-name Transformer --decoder-dim 64 --nhead 4 --num-decoder-layers 2 --norm-first false --add-prenet true "
                     "--scaling-xformers false".split())
    m = get_model(a)
    assert type(m) is Transformer and m.cfg.d_model == 64 and not m.cfg.norm_first and m.cfg.add_prenet
    from valle_amd.weights import mel_expected_keys

    assert list(m.state_dict()) == list(mel_expected_keys(m.cfg))
    sd = m.state_dict()
    r = Transformer(64, 4, 2, norm_first=False, add_prenet=True).load_state_dict(sd)
    assert not r.missing_keys and not r.unexpected_keys
    bad = dict(sd)
    del bad["stop_layer.bias"]
    with pytest.raises(RuntimeError, match="stop_layer.bias"):
        m.load_state_dict(bad)
    bad = dict(sd, bogus=torch.zeros(1))
    with pytest.raises(RuntimeError, match="bogus"):
        m.load_state_dict(bad)
    with pytest.raises(NotImplementedError):
        get_model(dict(model_name="Conformer", decoder_dim=64, nhead=4, num_decoder_layers=2))
    # the reference reads params.scaling_xformers unconditionally (models/__init__.py:133): without the field there is no default
    with pytest.raises(NotImplementedError, match="scaling_xformers"):
        get_model(dict(model_name="Transformer", decoder_dim=64, nhead=4, num_decoder_layers=2))
    assert type(get_model(dict(model_name="Transformer", decoder_dim=64, nhead=4, num_decoder_layers=2, scaling_xformers=False))) is Transformer


def test_scaling_xformers_is_refused_loudly(lib):
    from valle_amd.engine import VxMelConfig
    from valle_amd.models import Transformer, get_model

    with pytest.raises(NotImplementedError, match="scaling_xformers"):
        Transformer(64, 4, 2, scaling_xformers=True)
    with pytest.raises(NotImplementedError, match="scaling_xformers"):
        get_model(dict(model_name="Transformer", decoder_dim=64, nhead=4, num_decoder_layers=2, scaling_xformers=True))
    c = _mel_config(VxMelConfig)
    c.scaling_xformers = 1
    h = C.c_void_p()
    assert lib.vx_mel_create(C.byref(c), C.byref(h)) == 5  # VX_ERR_UNSUPPORTED, before any HIP call
    assert b"scaling_xformers" in lib.vx_last_error()


def _mel_config(VxMelConfig):
    c = VxMelConfig()
    c.struct_size = C.sizeof(VxMelConfig)
    c.d_model, c.nhead, c.num_layers, c.norm_first, c.precision, c.max_text, c.max_frames = 64, 4, 2, 1, 0, 16, 64
    return c


def test_abi_tables_are_consistent(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = sorted(n for n in set(re.findall(r"\b(vx_[a-z0-9_]+)\s*\(", hdr)) if n.startswith("vx_mel_"))
    assert declared == ["vx_mel_create", "vx_mel_decode", "vx_mel_decode_forced", "vx_mel_destroy", "vx_mel_encode", "vx_mel_finalize",
                        "vx_mel_get_timings", "vx_mel_read", "vx_mel_result", "vx_mel_set_sine_table", "vx_mel_set_weight",
                        "vx_mel_teacher_forced"]
    for n in declared:
        assert hasattr(lib, n) and n in engine.declared_symbols()
    assert C.sizeof(engine.VxMelConfig) == 12 * 4
    stops = dict(re.findall(r"VX_MEL_STOP_([A-Z_]+) = (\d)", hdr))
    assert {k.lower(): int(v) for k, v in stops.items()} == {v: k for k, v in engine.MEL_STOP_REASONS.items()}


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    from valle_amd.engine import VxMelConfig
    from valle_amd.models import Transformer

    h = C.c_void_p()
    c = _mel_config(VxMelConfig)
    c.struct_size = 0
    assert lib.vx_mel_create(C.byref(c), C.byref(h)) == 1 and b"struct_size" in lib.vx_last_error()
    for field, value, code in (("d_model", 96, 5), ("nhead", 5, 1), ("max_frames", 0, 1), ("precision", 2, 1), ("d_model", 2048, 5)):
        c = _mel_config(VxMelConfig)
        setattr(c, field, value)
        if field == "d_model":
            c.nhead = 8  # head_dim 12 / 256
        assert lib.vx_mel_create(C.byref(c), C.byref(h)) == code, (field, lib.vx_last_error())
    assert lib.vx_mel_encode(None, None, 3, None) == 1
    assert lib.vx_mel_decode(None, -1, None) == 1
    assert lib.vx_mel_teacher_forced(None, None, 3, None, 1, None, None, None) == 1

    m = Transformer(64, 4, 2, max_text=8, max_frames=32).eval()
    x = torch.randint(3, 50, (1, 6))
    with pytest.raises(AssertionError):  # transformer.py:337
        m.inference(x[0], torch.tensor([6]))
    with pytest.raises(AssertionError):  # transformer.py:340
        m.inference(x, torch.tensor([0]))
    with pytest.raises(ValueError, match="max_text"):
        m.inference(torch.randint(3, 50, (1, 9)), torch.tensor([9]))
    with pytest.raises(ValueError, match="100 bins"):
        m.teacher_forced(x, torch.tensor([6]), torch.zeros(5, 80))
    with pytest.raises(ValueError, match="max_frames"):
        m.teacher_forced(x, torch.tensor([6]), torch.zeros(33, 100))
    with pytest.raises(ValueError, match="max_frames"):
        m.inference(x, torch.tensor([6]), max_frames=33)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # valid arguments, no GPU: never a CPU path
        m.inference(x, torch.tensor([6]))
