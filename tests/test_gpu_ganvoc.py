"""GPU: the HiFi-GAN / BigVGAN generator (ganvoc_kernels.hpp behind vx_gan_synthesize, valle_amd.ganvoc.GanVocoder) against the fp64
restatement of tests/ganvoc_ref.py.

Yardstick: the restatement in fp64.  Floor: the same formula in torch fp32 on the host.  Bound: engine max-abs error <= 4 x floor
(ganvoc_ref.TOL_FACTOR, the project's rule); both figures are printed before they are asserted.  Every output holds NaN before
the call.  That the inputs tell a wrong pad, tap, crop, dilation, padding, 1/R or parameter apart (each moves the output by more
than 100 x the bound at T = 33, none left out) is checked without a GPU in test_ganvoc_cpu.py::test_every_mutation_moves_the_output.

1. the three narrow geometries of ganvoc_ref.GEOMETRIES at T in {1, 2, 3, 5, 33, 70}: T = 1..3 put every pad wider than the signal
   (conv_pre's 3, the dilation pad 25 of g2, the replicate pads 5 / 6 on L = T u), T = 33 and 70 cross the row tiles of the GEMM
   (64 and 128 rows) and of the activation (32 rows);
2. a ragged batch at odd pointer offsets: bitwise its solo results, repeatable, nothing written outside the outputs;
3. bigvgan_base's channel widths (C0 = 512, T = 8): float4 gather, both MFMA tile shapes;
4. a call cut into several groups of whole utterances is bitwise its solo results;
5. Transformer.inference_waveform(..., vocoder=GanVocoder(narrow)) on a fixture."""
import json
import os

import pytest
import torch

import ganvoc_ref as GR
from test_meltf_cpu import load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_VOC, _REF, _PARITY = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    yield
    for v in _VOC.values():
        v.close()
    _VOC.clear()
    out = os.environ.get("VX_GANVOC_PARITY_OUT")  # profiles/ganvoc_parity.json is written from here
    if out and _PARITY:
        with open(out, "w") as f:
            json.dump(_PARITY, f, indent=1, sort_keys=True)


def _cfg(name):
    return GR.BASE if name == "base" else GR.GEOMETRIES[name]


def _weights(name):
    cfg = _cfg(name)
    return GR.make_weights(cfg, 1, calib_T=8) if name == "base" else GR.make_weights(cfg, 1)  # base is checked at T = 8 only


def _voc(name):
    from valle_amd.ganvoc import GanVocoder

    if name not in _VOC:
        cfg = _cfg(name)
        _VOC[name] = GanVocoder(cfg, state_dict=_weights(name), max_batch=8, max_total_frames=4096).to(DEV)
    return _VOC[name]


def _reference(name, T, dtype):
    """The restatement's waveform for logmel(T), computed once and left unchanged."""
    key = (name, T, dtype)
    if key not in _REF:
        cfg = _cfg(name)
        _REF[key] = GR.forward(_weights(name), cfg, GR.logmel(T), dtype)
    return _REF[key]


def _run(v, mels, offset=0, fill=float("nan")):
    """One raw call: every input `offset` floats into a buffer of `fill`, every output likewise in a buffer of NaN with a cell after
    it.  -> (wavs, the whole output buffers)."""
    hopv = v.hop

    def place(t):
        buf = torch.full((t.numel() + offset + 1,), fill, dtype=torch.float32, device=DEV)
        buf[offset: offset + t.numel()] = t.reshape(-1).to(DEV)
        return buf

    Ts = [m.shape[0] for m in mels]
    ins = [place(m) for m in mels]
    outs = [torch.full((hopv * T + offset + 1,), float("nan"), dtype=torch.float32, device=DEV) for T in Ts]
    v._synthesize_raw([b.data_ptr() + 4 * offset if T else 0 for b, T in zip(ins, Ts)], Ts,
                      [b.data_ptr() + 4 * offset if T else 0 for b, T in zip(outs, Ts)])
    torch.cuda.synchronize()
    return [b[offset: offset + hopv * T].clone() for b, T in zip(outs, Ts)], outs


def _guards_hold(bufs, sizes, offset):
    for b, n in zip(bufs, sizes):
        assert bool(torch.isnan(b[:offset]).all()) and bool(torch.isnan(b[offset + n:]).all()), "a write outside an output"
        assert not bool(torch.isnan(b[offset: offset + n]).any()), "an output cell was not written"


def _check(name, T, wav):
    y64 = _reference(name, T, torch.float64)
    floor = float((_reference(name, T, torch.float32).double() - y64).abs().max())
    err = float((wav.cpu().double() - y64).abs().max())
    print(f"{name} T={T}: engine {err:.3e}, floor {floor:.3e}, ratio {err / floor if floor else float('inf'):.2f}")
    _PARITY[f"{name}_T{T}"] = {"engine": err, "floor": floor}
    assert wav.shape == y64.shape and bool(torch.isfinite(wav).all())
    assert err <= GR.tolerance(floor), f"{name} T={T}: engine {err:.3e} > {GR.TOL_FACTOR} x floor {floor:.3e}"


# ---- 1. the narrow geometries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (1, 2, 3, 5, 33, 70))
@pytest.mark.parametrize("name", sorted(GR.GEOMETRIES))
def test_against_fp64(name, T):
    v = _voc(name)
    wavs, bufs = _run(v, [GR.logmel(T)])
    _guards_hold(bufs, [v.hop * T], 0)
    _check(name, T, wavs[0])


# ---- 2. ragged batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GR.GEOMETRIES))
def test_ragged_batch_is_bitwise_its_solo_results(name):
    v = _voc(name)
    Ts = (1, 7, 2, 33)
    mels = [GR.logmel(T) for T in Ts]
    sizes = [v.hop * T for T in Ts]
    w0, bufs = _run(v, mels, offset=1)
    _guards_hold(bufs, sizes, 1)
    w1, _ = _run(v, mels, offset=3, fill=0.0)  # what surrounds the inputs does not matter; a repeat is bitwise equal
    for i, T in enumerate(Ts):
        assert torch.equal(w0[i], w1[i]), T
        ws, _ = _run(v, [mels[i]])
        assert torch.equal(w0[i], ws[0]), f"T={T}: the batch differs from the utterance alone"
    _check(name, 33, w0[3])
    # another order, with an empty utterance in it
    w2, _ = _run(v, mels[::-1] + [torch.zeros(0, 100)], offset=1)
    for i in range(len(Ts)):
        assert torch.equal(w0[i], w2[len(Ts) - 1 - i])


# ---- 3. full width ------------------------------------------------------------------------------------------------------------
def test_base_channel_widths():
    v = _voc("base")
    assert v.hop == 256
    wavs, bufs = _run(v, [GR.logmel(8)])
    _guards_hold(bufs, [256 * 8], 0)
    _check("base", 8, wavs[0])


# ---- 4. groups and the Python surface -----------------------------------------------------------------------------------------
def test_groups_of_whole_utterances_are_bitwise_solo():
    """C0 = 64 at rates 8 x 2: the widest row buffer holds max(100, 64, 8 x 32, 16 x 16) = 256 floats per frame, so 2^24 / 256 =
    65536 frames fill a group and one vx_gan_synthesize of 30000 + 30000 + 20000 + 25000 frames is served as two groups of two
    utterances: the second group reads its segment table, its pointers and the reused buffers at offsets.  Every utterance is
    bitwise its solo result.  Short lengths again through synthesize_batch's own chunking into several calls."""
    from valle_amd.ganvoc import GanVocoder

    cfg = GR.GEOMETRIES["g2_snake"]
    Ts = (30000, 30000, 20000, 25000)
    assert Ts[0] + Ts[1] <= (1 << 24) // 256 < Ts[0] + Ts[1] + Ts[2] and Ts[2] + Ts[3] <= (1 << 24) // 256
    big = GanVocoder(cfg, state_dict=GR.make_weights(cfg, 1), max_batch=4, max_total_frames=sum(Ts)).to(DEV)
    g = torch.Generator().manual_seed(4)
    mels = [(torch.randn((T, 100), generator=g) * 2.0 - 4.0).to(DEV) for T in Ts]
    wavs = big.synthesize_batch(mels)  # 4 <= max_batch and sum(Ts) <= max_total_frames: one call
    for i, T in enumerate(Ts):
        w = big(mels[i])
        assert w.shape == (16 * T,) and bool(torch.isfinite(w).all()) and torch.equal(w, wavs[i]), i
    big.close()
    small = GanVocoder(cfg, state_dict=GR.make_weights(cfg, 1), max_batch=2, max_total_frames=40).to(DEV)
    short = [GR.logmel(T).to(DEV) if T else torch.zeros(0, 100, device=DEV) for T in (7, 0, 3, 33, 1)]
    got = small.synthesize_batch(short)
    for m, w in zip(short, got):
        assert w.shape == (16 * m.shape[0],)
        if m.shape[0]:
            assert torch.equal(w, _voc("g2_snake")(m))
    assert torch.equal(small(short[0][None]), got[0])  # (1, T, n_mels) is accepted
    small.close()


# ---- 5. text -> mel -> waveform -----------------------------------------------------------------------------------------------
def test_inference_waveform_through_the_generator():
    from valle_amd.models import Transformer

    f = load_fixture("a_prenorm")
    c = f["cfg"]
    m = Transformer(c.d_model, c.nhead, c.num_layers, norm_first=c.norm_first, add_prenet=c.add_prenet, precision="fp32", max_text=16,
                    max_frames=96, print_eos=False)
    m.load_state_dict(f["sd"])
    m = m.to(DEV).eval()
    v = _voc("g1_snakebeta")
    x, x_lens = f["x"][None].to(DEV), torch.tensor([f["S"]])
    mel, wav = m.inference_waveform(x, x_lens, vocoder=v)
    T = mel.shape[1]
    assert mel.shape[0] == 1 and T >= 1 and wav.shape == (T * v.hop,) and wav.device == mel.device
    assert bool(torch.isfinite(wav).all()) and torch.equal(wav, v(mel[0]))
