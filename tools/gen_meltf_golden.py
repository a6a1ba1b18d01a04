"""Writes the mel-Transformer fixtures under tests/golden/meltf/ - build container only (needs the reference tree).

    python tools/gen_meltf_golden.py

For every fixture: the UNMODIFIED reference class (valle/models/transformer.py, imported through oracle.ref_harness) runs
``Transformer.inference`` on name-seeded weights; the functional restatement tests/meltf_ref.py must give, in fp32, the same
number of frames and the same frames (within FP32_EQ: the two differ in the order of fp32 operations only - torch's fused
attention against explicit matmuls); only then are the restatement's fp64 results recorded.  Recorded per fixture:
  cfg [d, heads, L, norm_first, add_prenet, S], weight_seed, stop_bias, x (S,) ids,
  run_frames (10 S, 100) / run_stops (10 S + 1,) fp64: the run to the length rule (the frames do not depend on stop_layer.bias;
      the stop logits are given under the fixture's bias),
  n_frames, reason: what ``inference`` returns under the fixture's bias - run_frames[:n_frames].
Stop-logit fixtures: the stop pass t* is the argmax of the raw stop logits over the first 40 passes, the bias puts 0 midway
between that logit and the largest earlier one, and the half-margin must exceed twice the bf16 tolerance of the GPU tests
(0.03 x the largest |stop logit| up to t*), so that exactly one pass lies above -2 tol, and it lies above +2 tol; weight seeds
are scanned until that holds.  Also writes state_dict_layout.json: the reference's keys and shapes for four constructor variants."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from meltf_ref import MelRef  # noqa: E402
from oracle.ref_harness import load_reference  # noqa: E402
from valle_amd.config import MelConfig  # noqa: E402
from valle_amd.weights import mel_synthetic_state_dict, synthetic_inputs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "meltf")
FP32_EQ = 2e-5  # fp32 restatement against the reference class, frames of magnitude 1-3
BF16_REL = 0.03  # the bf16 tolerance of tests/test_gpu_meltf.py
LONG_BIAS = -8.0  # a stop bias under which no pass stops: the run to the length rule

# name: (d, heads, L, S, norm_first, add_prenet, stop)   stop: None = length rule, "mid" = on the stop logit, "first" = pass 0
FIXTURES = {
    "a_prenorm": (64, 4, 2, 6, True, False, None),
    "b_postnorm": (64, 4, 2, 6, False, False, None),
    "c_hd4_prenet": (64, 16, 2, 5, True, True, None),
    "d_hd64_stop": (256, 4, 3, 8, True, False, "mid"),
    "e_d192": (192, 12, 2, 5, True, False, None),
    "f_stop_first": (64, 4, 2, 6, True, False, "first"),
}


def reference_run(models, cfg, sd, x):
    ref = models.Transformer(cfg.d_model, cfg.nhead, cfg.num_layers, norm_first=cfg.norm_first, add_prenet=cfg.add_prenet).eval()
    missing, unexpected = ref.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    with torch.no_grad():
        return ref.inference(x, torch.tensor([x.shape[1]]))[0]


def build(models, name, spec):
    d, H, L, S, nf, pn, stop = spec
    cfg = MelConfig(d, H, L, nf, pn)
    x = synthetic_inputs(S, 1, seed=7)[0]
    for seed in range(1, 200):
        sd = mel_synthetic_state_dict(cfg, seed, stop_bias=LONG_BIAS)
        frames, stops, reason = MelRef(sd, d, H, L, nf, pn, dtype=torch.float64).inference(x[0])
        assert reason == "length" and frames.shape[0] == 10 * S, (reason, frames.shape)
        raw = stops - LONG_BIAS
        bias, n_frames, why = LONG_BIAS, 10 * S, "length"
        if stop == "mid":
            t = int(torch.argmax(raw[:40]))
            if t < 5:
                continue
            prev = float(raw[:t].max())
            half = (float(raw[t]) - prev) / 2
            bias = -(float(raw[t]) + prev) / 2
            tol = BF16_REL * float((raw[: t + 1] + bias).abs().max())
            if not half > 2 * tol:
                continue
            n_frames, why = t, "logit"
        elif stop == "first":
            bias = 0.5 - float(raw[0])  # pass 0 sits at +0.5: 0.5 > 2 x 0.03 x 0.5
            n_frames, why = 0, "logit"
        sd = mel_synthetic_state_dict(cfg, seed, stop_bias=bias)
        bias = float(sd["stop_layer.bias"][0])  # as the fp32 tensor holds it
        run_stops = raw + bias
        if stop is not None:  # exactly one pass above -2 tol, and it is above +2 tol
            tol = BF16_REL * float(run_stops[: n_frames + 1].abs().max())
            assert bool((run_stops[:n_frames] < -2 * tol).all()) and float(run_stops[n_frames]) > 2 * tol, (name, seed)
        # the restatement under the fixture's bias, fp64 and fp32, and the unmodified reference class
        f64, s64, r64 = MelRef(sd, d, H, L, nf, pn, dtype=torch.float64).inference(x[0])
        assert r64 == why and f64.shape[0] == n_frames and torch.equal(f64, frames[:n_frames])
        f32, s32, r32 = MelRef(sd, d, H, L, nf, pn, dtype=torch.float32).inference(x[0])
        ref = reference_run(models, cfg, sd, x)
        assert ref.shape == f32.shape == (n_frames, 100), (name, ref.shape, f32.shape)
        err = float((ref - f32).abs().max()) if n_frames else 0.0
        drift = float((f32.double() - f64).abs().max()) if n_frames else 0.0
        assert err < FP32_EQ, (name, err)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), cfg=np.array([d, H, L, int(nf), int(pn), S], dtype=np.int64),
                            weight_seed=np.int64(seed), stop_bias=np.float64(bias), x=x[0].numpy(), run_frames=frames.numpy(),
                            run_stops=run_stops.numpy(), n_frames=np.int64(n_frames), reason=np.array(why))
        print(f"{name}: seed {seed}, bias {bias:+.6f}, {n_frames} frames ({why}), restatement fp32 vs reference {err:.2e}, "
              f"fp32 vs fp64 {drift:.2e}, |frames| <= {float(frames.abs().max()):.2f}, raw stop logits {float(raw.min()):+.3f} .. {float(raw.max()):+.3f}")
        return
    raise SystemExit(f"{name}: no weight seed gives the required stop margin")


def main():
    models = load_reference()
    os.makedirs(OUT, exist_ok=True)
    layout = {}
    for nf in (True, False):
        for pn in (False, True):
            m = models.Transformer(64, 4, 2, norm_first=nf, add_prenet=pn)
            layout[f"d64_h4_l2_norm_first{int(nf)}_add_prenet{int(pn)}"] = {k: list(v.shape) for k, v in m.state_dict().items()}
    with open(os.path.join(OUT, "state_dict_layout.json"), "w") as f:
        json.dump(layout, f, indent=0, sort_keys=False)
    for name, spec in FIXTURES.items():
        build(models, name, spec)


if __name__ == "__main__":
    main()
