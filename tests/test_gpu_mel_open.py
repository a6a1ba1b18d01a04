"""GPU: mel_open_kernel (csrc/meltf.hip), the launch that opens every decode step of the mel-spectrogram Transformer, alone on caller
buffers (vx_op_mel_open) against the fp64 references of tests/mel_step_ref.py, at the widths of mel_step_cases.OPEN_WIDTHS: d = 8
leaves eight of the 16 workgroups without a prenet row, 200 / 1000 / 1016 end in a ragged slice, none of them but 1024 fills the
norm's 256 x 4 channels or the head's four 256-channel groups.

  * the stored frame and stop logit: within C_LOGIT units of 2^-24 (sum |w| |h| + |b|) of the fp64 LayerNorm + head of xh;
  * the next input row: within C_LOGIT units of 2^-24 (sum |w| |h| + |b| + |alpha pe|) of the fp64 prenet + position row of the
    frame the kernel itself stored (the all-zero frame at row -1); with a prenet that is exact in fp32, bitwise
    fadd(prenet, fmul(alpha, pe));
  * the stop rule on stop logits set exactly, every state word after every case (mel_step_cases.OPEN_RULE);
  * x, frames and stops lie inside blocks filled with a marked NaN: exactly x[0:d], frames[n_gen] (when appended) and
    stops[pass] change, x not on a stopping pass, nothing on a finished decode; the arrival counter is 0 after every launch;
  * three launches on one device state equal three single launches bitwise;
  * every wrong answer of mel_step_ref.open_wrong lies at least SEP bounds from the kernel's output.

C_LOGIT (3.5) and SEP are test_gpu_ar_step.py's.  Measured on the MI355X (profiles/mel_step_parity.json): the head at most 2.51
units (d = 8, where eight channels carry the whole variance; 1.13 from d = 64 up), the next input row at most 2.16 (d = 1016, MLP
prenet: three layers deep), the nearest wrong answer 4.18e+03 bounds away (the last prenet row taken from the one before, d = 1024).
The bitwise check found the position product contracted into a fused multiply-add; the kernel now rounds it on its own."""
import math

import pytest
import torch

import mel_step_cases as MC
import mel_step_ref as R
from test_gpu_ar_step import C_LOGIT, SEP

pytestmark = pytest.mark.gpu

FILL = 0x7FC12345  # a NaN no arithmetic produces: a cell that still holds it was not written
STOPS_CAP = 16
WORDS = ("row", "pass", "n_gen", "done", "stop_reason")


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    engine.load_library()
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return engine


def _block(n):
    return torch.full((n,), FILL, dtype=torch.int32, device="cuda").view(torch.float32)


def _launch(eng, inp, st, max_frames=50, n_forced=0, launches=1):
    """One call on fresh guarded blocks -> dict(state, arrive, x (d,), frames (OPEN_CAP, 100), stops (STOPS_CAP,), and the
    written cells of each block as index lists relative to the buffer the kernel was given; the guards count as negative or
    past-the-end indices)."""
    d = inp["xh"].numel()
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else None) for k, v in inp.items()}
    xb, fb, sb = _block(d + 32), _block((MC.OPEN_CAP + 2) * R.MEL_BINS), _block(STOPS_CAP + 16)
    x, frames, stops = xb[16: 16 + d], fb[R.MEL_BINS: (MC.OPEN_CAP + 1) * R.MEL_BINS].view(MC.OPEN_CAP, R.MEL_BINS), sb[8: 8 + STOPS_CAP]
    forced = dev["forced"][:n_forced].contiguous() if n_forced else None
    state, arrive = eng.op_mel_open(dev["xh"], dev["gamma"], dev["beta"], dev["Wh"], dev["bh"], dev["W0"], dev["b0"], dev["alpha"],
                                    dev["pe"], x, frames, stops, st, dev["W1"], dev["b1"], dev["W2"], dev["b2"], max_frames=max_frames,
                                    n_forced=n_forced, forced=forced, launches=launches)
    wr = lambda b, off: [int(i) - off for i in (b.view(torch.int32) != FILL).nonzero().flatten().cpu()]
    return dict(state=state, arrive=arrive, x=x.cpu(), frames=frames.cpu(), stops=stops.cpu(), x_written=wr(xb, 16),
                frames_written=wr(fb, R.MEL_BINS), stops_written=wr(sb, 8))


def _check_written(r, d, st, append, go, counted=True):
    """Exactly x[0:d] (when the decode goes on), frames[n_gen] (when appended) and stops[pass] (when a head was computed)."""
    assert r["x_written"] == (list(range(d)) if go else []), "x"
    n = st["n_gen"]
    assert r["frames_written"] == (list(range(n * R.MEL_BINS, (n + 1) * R.MEL_BINS)) if append else []), "frames"
    assert r["stops_written"] == ([st["pass"]] if counted and st["row"] >= 0 else []), "stops"
    assert r["arrive"] == 0, "arrival counter"


def _state(row, n_gen, S=2, done=0):
    return dict(row=row, **{"pass": max(row, 0)}, n_gen=n_gen, S=S, done=done, stop_reason=0)


@pytest.mark.parametrize("mlp", MC.OPEN_PRENETS, ids=["linear", "mlp"])
@pytest.mark.parametrize("d", list(MC.OPEN_WIDTHS))
def test_open_outputs_match_fp64(eng, d, mlp):
    inp = MC.open_inputs(d, mlp)
    head, hs = R.open_head(inp)
    fails, worst_h, worst_x, nearest = [], 0.0, 0.0, (float("inf"), "")
    for row in MC.OPEN_ROWS:
        st = _state(row, min(max(row, 0), 5), S=5)
        r = _launch(eng, inp, st)
        want, append, go = R.open_rule(st, float(head[R.MEL_BINS]), 50, 0)
        assert go and append == (row >= 0)
        assert {k: r["state"][k] for k in WORDS} == {k: want[k] for k in WORDS}, (row, r["state"])
        _check_written(r, d, st, append, go)
        frame = torch.zeros(R.MEL_BINS, dtype=torch.float64)
        if row >= 0:
            frame = r["frames"][st["n_gen"]].double()
            got_h = torch.cat([frame, r["stops"][st["pass"]: st["pass"] + 1].double()])
            u = R.units((got_h - head).abs(), R.U32 * hs)
            worst_h = max(worst_h, u)
            if not u <= C_LOGIT:
                fails.append(f"row {row} head: {u:.4g} units")
        x, xs = R.open_x(inp, frame, row + 1)
        got_x = r["x"].double()
        u = R.units((got_x - x).abs(), R.U32 * xs)
        worst_x = max(worst_x, u)
        if not u <= C_LOGIT:
            fails.append(f"row {row} x: {u:.4g} units")
        for name, (kind, w) in R.open_wrong(inp, row, frame).items():
            got, scale = (got_h, hs) if kind == "head" else (got_x, xs)
            sep = R.units((w - got).abs(), C_LOGIT * R.U32 * scale)
            nearest = min(nearest, (sep, f"{name}@{row}"))
            if not sep >= SEP:
                fails.append(f"row {row} wrong answer {name}: {sep:.3g} bounds")
    print(f"\nmel_open d={d} mlp={mlp}: head {worst_h:.3g} units, x {worst_x:.3g} units (bound {C_LOGIT}); nearest wrong answer "
          f"{nearest[1]} {nearest[0]:.3g} bounds")
    MC.parity_note(f"mel_open/d{d}/{'mlp' if mlp else 'linear'}", dict(head_units=worst_h, x_units=worst_x, nearest_wrong=nearest[0],
                                                                   nearest_wrong_name=nearest[1]))
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("mlp", MC.OPEN_PRENETS, ids=["linear", "mlp"])
@pytest.mark.parametrize("d", list(MC.OPEN_WIDTHS))
def test_open_position_product_is_bitwise(eng, d, mlp):
    """An exact prenet leaves two roundings, the product's and the sum's: x is bitwise fadd(prenet, fmul(alpha, pe[row + 1]))."""
    inp = MC.open_exact_inputs(d, mlp)
    for row in (-1, 0, 3, MC.OPEN_CAP - 2):
        st = _state(row, max(row, 0))
        r = _launch(eng, inp, st, n_forced=MC.OPEN_CAP)
        frame = inp["forced"][row] if row >= 0 else torch.zeros(R.MEL_BINS)
        want = R.open_x_exact32(inp, frame, row + 1)
        assert r["state"]["row"] == row + 1 and r["state"]["done"] == 0
        assert torch.equal(r["x"].view(torch.int32), want.view(torch.int32)), (row, float((r["x"] - want).abs().max()))
        _check_written(r, d, st, row >= 0, True)


@pytest.mark.parametrize("d", MC.OPEN_RULE_WIDTHS)
@pytest.mark.parametrize("name", list(MC.OPEN_RULE))
def test_open_stop_rule(eng, name, d):
    value, st, max_frames, n_forced = MC.OPEN_RULE[name]
    inp = MC.with_stop(MC.open_inputs(d, d == 8), value)
    r = _launch(eng, inp, st, max_frames=max_frames, n_forced=n_forced)
    assert tuple(r["state"][k] for k in WORDS) == MC.OPEN_RULE_WANT[name], r["state"]
    assert r["state"]["S"] == st["S"]
    want, append, go = R.open_rule(st, value, max_frames, n_forced)
    _check_written(r, d, st, append, go, counted=not st["done"])
    if st["done"]:
        return
    stop = float(r["stops"][st["pass"]])
    assert (math.isnan(stop) and math.isnan(value)) or stop == value, stop  # row zeroed, value in the bias: exact
    if go:  # the fed-back frame: the forced one, or the one just stored
        frame = (inp["forced"][st["n_gen"]] if n_forced else r["frames"][st["n_gen"]]).double()
        x, xs = R.open_x(inp, frame, st["row"] + 1)
        assert R.units((r["x"].double() - x).abs(), R.U32 * xs) <= C_LOGIT
    if append:  # what is stored is the prediction, forced or not
        head, hs = R.open_head(inp)
        assert R.units((r["frames"][st["n_gen"]].double() - head[: R.MEL_BINS]).abs(), R.U32 * hs[: R.MEL_BINS]) <= C_LOGIT


@pytest.mark.parametrize("mlp", MC.OPEN_PRENETS, ids=["linear", "mlp"])
@pytest.mark.parametrize("d", MC.OPEN_RULE_WIDTHS + (1024,))
def test_open_three_launches_equal_three_single_ones(eng, d, mlp):
    inp = MC.open_inputs(d, mlp)
    bits = lambda t: t.view(torch.int32)
    for row0 in (-1, 0):
        st0 = _state(row0, 0)
        r3 = _launch(eng, inp, st0, launches=3)
        k = 3 if row0 >= 0 else 2  # the launch at row -1 only forms input row 0
        assert (r3["state"]["row"], r3["state"]["pass"], r3["state"]["n_gen"], r3["state"]["done"]) == (row0 + 3, k, k, 0)
        assert r3["arrive"] == 0 and r3["x_written"] == list(range(d))
        assert r3["frames_written"] == list(range(k * R.MEL_BINS)) and r3["stops_written"] == list(range(k))
        st = st0
        for i in range(3):
            r1 = _launch(eng, inp, st)
            assert r1["state"]["row"] == st["row"] + 1 and r1["arrive"] == 0
            if st["row"] >= 0:
                assert r1["state"]["pass"] == st["pass"] + 1 and r1["state"]["n_gen"] == st["n_gen"] + 1
                assert torch.equal(bits(r1["frames"][st["n_gen"]]), bits(r3["frames"][st["n_gen"]])), i
                assert torch.equal(bits(r1["stops"][st["pass"]]), bits(r3["stops"][st["pass"]])), i
            st = r1["state"]
        assert torch.equal(bits(r1["x"]), bits(r3["x"]))
        assert st == r3["state"]


def test_open_argument_checks(eng):
    """As vx_mel_create: d % 8 == 0 and d <= 1024; and the launches must stay inside pe, frames and stops."""
    from valle_amd.engine import VxError

    inp = MC.open_inputs(8, False)
    with pytest.raises(VxError, match="leave pe"):
        _launch(eng, inp, _state(MC.OPEN_PE_ROWS - 2, 0), launches=2)
    with pytest.raises(VxError, match="leave pe"):
        _launch(eng, inp, _state(0, MC.OPEN_CAP - 1), launches=2)
    bad = dict(inp)
    for d in (12, 1032):
        bad.update(xh=torch.zeros(d))
        with pytest.raises(VxError, match="multiple of 8"):
            _launch(eng, bad, _state(0, 0))
