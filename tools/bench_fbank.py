"""Log-mel filterbank time at (B, seconds) = (1, 3), (1, 10), (32, 10), (64, 20): `BigVGANFbank.extract_batch` (one HIP launch,
device waveforms in, device features out) against the same formula on stock torch GPU ops (pad, `torch.stft` on the device,
sqrt, matmul with the mel basis, clamp, log) per utterance and on the stacked batch; plus the error ratios of the parity test's
inputs (engine error and fp32 host floor against the fp64 definition of tests/fbank_ref.py).  One JSON line on stdout, the same
object written to --out.

    python tools/bench_fbank.py [--reps 9] [--points 1x3,1x10,32x10,64x20] [--out profiles/fbank_times.json]
    python tools/bench_fbank.py --only-hip --points 64x20 --reps 20      # the run to put under a kernel tracer

Each point is warmed twice per implementation, then the implementations alternate rep by rep.  A rep runs the call `inner`
times back to back (chosen per implementation so that a rep lasts about 20 ms or more) and ends in a device synchronise; the
figure is the median over the reps of the rep's wall time / inner."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--points", default="1x3,1x10,32x10,64x20", help="BxSECONDS,...")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fbank_times.json"))
    ap.add_argument("--only-hip", action="store_true", help="time the HIP call alone (for a kernel trace); writes no file")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F

    import __graft_entry__ as ge

    ge.build()
    import fbank_ref as FR
    from valle_amd.fbank import TILE_FRAMES, BigVGANFbank

    if not torch.cuda.is_available():
        raise SystemExit("bench_fbank.py measures on the GPU; none found")
    dev = "cuda:0"
    points = [tuple(int(v) for v in p.split("x")) for p in args.points.split(",")]
    fb = BigVGANFbank(max_batch=max(b for b, _ in points)).to(dev)
    basis = fb.mel_basis.to(dev)
    window = torch.hann_window(1024, device=dev)
    sync = torch.cuda.synchronize

    @torch.no_grad()
    def torch_fbank(y):
        """y (B, L) on the device -> (B, frames, 100): the reference's formula on stock ops."""
        nf = FR.n_frames(y.shape[-1])
        y = F.pad(y, (0, (nf - 1) * 256 + 1024 - y.shape[-1]))
        spec = torch.stft(y, 1024, hop_length=256, win_length=1024, window=window, center=False, pad_mode="reflect",
                          normalized=False, onesided=True, return_complex=True)
        mag = torch.sqrt(torch.view_as_real(spec).pow(2).sum(-1) + 1e-9)
        return torch.log(torch.clamp(torch.matmul(basis, mag), min=1e-5)).transpose(2, 1)

    def timed(fn, inner):
        sync()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        return (time.perf_counter() - t0) / inner

    out = {"bench": "fbank", "reps": args.reps, "tile_frames": TILE_FRAMES, "points": []}
    if not args.only_hip:
        try:  # torch.stft on the device needs the FFT library of the torch build
            torch_fbank(torch.zeros(1, 4801, device=dev))
            sync()
        except RuntimeError as e:
            out["torch_gpu"] = "not measured: " + str(e).splitlines()[0][:200]
            args.only_hip, args.no_torch = True, True
    for B, sec in points:
        L = 24000 * sec
        wavs = [FR.make_noise(L, 300 + b, 0.3).to(dev) for b in range(B)]
        stacked = torch.stack(wavs)
        impls = {"hip": lambda: fb.extract_batch(wavs)}
        row = {"B": B, "seconds": sec, "samples": L, "frames": FR.n_frames(L)}
        if not args.only_hip:
            impls["torch_gpu"] = lambda: [torch_fbank(w[None]) for w in wavs]
            impls["torch_gpu_batched"] = lambda: torch_fbank(stacked)
            ours = torch.stack(fb.extract_batch(wavs))
            row["hip_vs_torch_gpu_max_abs_diff"] = float((ours - torch_fbank(stacked)).abs().max())
        inner = {}
        for k, fn in impls.items():
            timed(fn, 1)
            inner[k] = max(1, min(200, int(0.02 / max(timed(fn, 1), 1e-6))))
        times = {k: [] for k in impls}
        for _ in range(args.reps):
            for k, fn in impls.items():
                times[k].append(timed(fn, inner[k]))
        for k, v in times.items():
            row[k + "_ms"] = round(1e3 * statistics.median(v), 4)
            row[k + "_min_ms"] = round(1e3 * min(v), 4)
            row[k + "_inner"] = inner[k]
        out["points"].append(row)
    if not args.only_hip or getattr(args, "no_torch", False):
        ratios = []
        for amp in (0.1, 1.0):
            for L in (128, 1024, 1025, 4801, 24000, (TILE_FRAMES + 1) * 256):
                x = FR.make_noise(L, 7 * L + int(10 * amp), amp)
                ref64 = FR.fbank_definition(x, fb.mel_basis)
                floor = float((FR.fbank_definition(x, fb.mel_basis, torch.float32).double() - ref64).abs().max())
                err = float((fb.extract_batch([x])[0].double().cpu() - ref64).abs().max())
                ratios.append({"amp": amp, "L": L, "floor": floor, "engine": err, "ratio": round(err / floor, 3)})
        out["parity"] = ratios
        out["parity_ratio_max"] = max(r["ratio"] for r in ratios)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
