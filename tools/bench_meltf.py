"""Times the mel-spectrogram Transformer's decode on the GPU and writes profiles/meltf_times.json.

    python tools/bench_meltf.py [--out profiles/meltf_times.json] [--frames 470] [--repeats 3]

At d 1024 / 16 heads / 12 layers, a text of 47 ids run to the length rule (470 frames; stop_layer.bias = -8), per precision:
  * ms per step of the cached decode (device time of the replayed steps over their number), best and all of `repeats` runs;
  * the opening kernel alone, by difference: the step at 1 and at 2 layers (step(1) - (step(2) - step(1)));
  * baselines measured in the same process: the VALL-F batch-1 AR step at the same geometry (teacher-forced tokens, so that it runs
    the same number of passes), and the reference's no-cache loop restated on stock torch GPU ops (tests/meltf_ref.py, fp32) at 60
    frames.
The two-launch form of the head (a one-workgroup head, then the GEMV with the position epilogue) is not built; it is reported as
not measured.  No GPU: the script fails, it does not fall back."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def mel_steps(cfg, sd, prec, S, frames, repeats):
    from valle_amd.engine import MelEngine
    from valle_amd.weights import synthetic_inputs

    x = synthetic_inputs(S, 1, seed=7)[0][0]
    e = MelEngine(cfg, precision=prec, max_text=64, max_frames=frames + 2)
    e.load_state_dict(sd)
    runs = []
    for r in range(repeats + 1):  # run 0 warms up (graph capture, code objects)
        e.encode(x)
        e.decode(frames)
        t = e.timings()
        n = e.result()[0].shape[0]
        assert n == frames, (n, frames)
        if r:
            runs.append(t["decode_ms"] / t["step_launches"])
    kernels = t["kernels_per_step"]
    e.close()
    return dict(best=min(runs), runs=runs), kernels


def vallf_step(prec, S, frames, repeats):
    from valle_amd.config import ModelConfig
    from valle_amd.engine import Engine
    from valle_amd.weights import synthetic_inputs, synthetic_state_dict

    cfg = ModelConfig(model_name="VALL-F", num_quantizers=1)
    e = Engine(cfg, precision=prec, max_text=64, max_audio=frames + 8)
    e.load_state_dict(synthetic_state_dict(cfg, 0))
    x, _, y = synthetic_inputs(S, 1, num_quantizers=1, seed=7)
    forced = torch.randint(0, 1024, (frames,), generator=torch.Generator().manual_seed(1)).cuda()
    runs = []
    for r in range(repeats + 1):
        e.ar_prefill(x[0], y[0, :, 0].contiguous())
        e.ar_decode(top_k=1, forced=forced)
        t = e.timings()
        if r:
            runs.append(t["decode_ms"] / t["launches"])
    e.close()
    return dict(best=min(runs), runs=runs)


def torch_no_cache(cfg, sd, S, frames):
    from meltf_ref import MelRef
    from valle_amd.weights import synthetic_inputs

    x = synthetic_inputs(S, 1, seed=7)[0][0]
    ref = MelRef(sd, cfg.d_model, cfg.nhead, cfg.num_layers, dtype=torch.float32, device="cuda")
    ref.inference(x, max_frames=4)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ref.inference(x, max_frames=frames)[0]
    torch.cuda.synchronize()
    return dict(frames=int(out.shape[0]), ms_per_frame=(time.perf_counter() - t0) * 1e3 / max(1, out.shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meltf_times.json"))
    ap.add_argument("--frames", type=int, default=470)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meltf needs the GPU: no measurement without one")
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.config import MelConfig
    from valle_amd.weights import mel_synthetic_state_dict

    S = a.frames // 10
    res = dict(geometry=dict(d_model=1024, nhead=16, num_layers=12, S=S, frames=a.frames), device=torch.cuda.get_device_name(0),
               two_launch_head="not built, not measured")
    cfg = MelConfig(1024, 16, 12)
    sd = mel_synthetic_state_dict(cfg, 0, stop_bias=-8.0)
    for prec in ("bf16", "fp32"):
        steps, kernels = mel_steps(cfg, sd, prec, S, a.frames, a.repeats)
        res[prec] = dict(mel_ms_per_step=steps, kernels_per_step=kernels, vallf_ar_ms_per_step=vallf_step(prec, S, a.frames, a.repeats))
        small = {}
        for L in (1, 2):
            c = MelConfig(1024, 16, L)
            small[L] = mel_steps(c, mel_synthetic_state_dict(c, 0, stop_bias=-8.0), prec, S, a.frames, a.repeats)[0]["best"]
        res[prec]["step_ms_1_layer"], res[prec]["step_ms_2_layers"] = small[1], small[2]
        res[prec]["opening_kernel_ms_by_difference"] = small[1] - (small[2] - small[1])
    res["torch_no_cache_fp32"] = torch_no_cache(cfg, sd, S, 60)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
