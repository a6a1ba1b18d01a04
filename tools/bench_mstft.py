"""Multi-resolution STFT distance time at (pairs, seconds) = (1, 3), (1, 10), (32, 10), (64, 20): `MultiResolutionSTFT.compare_sums`
(one launch of stft_tile_kernel per resolution and one of stft_finish_kernel per 64 pairs; device waveforms in, 12 doubles per pair
out) against the same definition on stock torch GPU ops in fp32: `torch.stft(center=True, pad_mode="reflect")` with the Hann window
of `win` samples, sqrt(clamp(re^2 + im^2, 1e-8)), the Frobenius norms and the mean absolute log difference per pair, once on the
stacked batch (`torch_gpu_stacked`, all pairs in one stft per signal and resolution) and once pair by pair (`torch_gpu_per_pair`).
Plus the error ratios of the magnitudes on the parity test's inputs.  One JSON line on stdout, the same object written to --out.

    python tools/bench_mstft.py [--reps 5] [--points 1x3,1x10,32x10,64x20] [--out profiles/mstft_times.json]
    python tools/bench_mstft.py --only-hip --points 64x20 --reps 20      # the run to put under a kernel tracer

Each point is warmed once per implementation, then the implementations alternate rep by rep.  A rep runs the call `inner` times
back to back (chosen per implementation so that a rep lasts about 20 ms or more) and ends in a device synchronise; the figure is
the median over the reps of the rep's wall time / inner.  The waveforms are Gaussian noise, not speech: the time does not depend
on the samples."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", default="1x3,1x10,32x10,64x20", help="PAIRSxSECONDS,...")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mstft_times.json"))
    ap.add_argument("--only-hip", action="store_true", help="time the HIP call alone (for a kernel trace); writes no file")
    args = ap.parse_args()
    import numpy as np
    import torch

    import __graft_entry__ as ge

    ge.build()
    import stft_ref as SR
    from valle_amd.stft import TILE_FRAMES, MultiResolutionSTFT, STFTConfig

    if not torch.cuda.is_available():
        raise SystemExit("bench_mstft.py measures on the GPU; none found")
    dev = "cuda:0"
    points = [tuple(int(v) for v in p.split("x")) for p in args.points.split(",")]
    sync = torch.cuda.synchronize
    obj = MultiResolutionSTFT().to(dev)
    windows = [torch.hann_window(w, device=dev) for _, _, w in SR.RESOLUTIONS]

    @torch.no_grad()
    def torch_sums(X, Y):
        """X, Y (P, L) fp32 -> (P, R, 3) fp32: sc, lm and their sum per pair and resolution."""
        rows = []
        for (n_fft, hop, win), window in zip(SR.RESOLUTIONS, windows):
            mags = []
            for s in (X, Y):
                spec = torch.stft(s, n_fft, hop_length=hop, win_length=win, window=window, center=True, pad_mode="reflect",
                                  normalized=False, onesided=True, return_complex=True)
                mags.append(torch.sqrt(torch.clamp(spec.real ** 2 + spec.imag ** 2, min=SR.EPS)))
            mx, my = mags
            sc = torch.linalg.norm((my - mx).flatten(1), dim=1) / torch.linalg.norm(my.flatten(1), dim=1)
            lm = (torch.log(my) - torch.log(mx)).abs().flatten(1).mean(1)
            rows.append(torch.stack([sc, lm, sc + lm], 1))
        return torch.stack(rows, 1)

    def timed(fn, inner):
        sync()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        return (time.perf_counter() - t0) / inner

    out = {"bench": "mstft", "reps": args.reps, "resolutions": [list(r) for r in SR.RESOLUTIONS], "tile_frames": TILE_FRAMES, "points": []}
    for P, sec in points:
        L = 24000 * sec
        X = torch.stack([SR.make_noise(L, 10 * P + p, 0.3) for p in range(P)]).to(dev)
        Y = torch.stack([SR.make_noise(L, 5000 + 10 * P + p, 0.3) for p in range(P)]).to(dev)
        xs, ys = list(X), list(Y)
        cells = sum(SR.n_frames(L, r) * (r[0] // 2 + 1) for r in SR.RESOLUTIONS)
        flop = sum(2 * SR.n_frames(L, r) * 4 * ((r[2] + 7) // 8 * 8) * 32 * (r[0] // 64) for r in SR.RESOLUTIONS)  # both signals, re and im
        row = {"pairs": P, "seconds": sec, "cells_per_pair": cells, "mfma_gflop_per_pair": round(flop / 1e9, 2)}
        impls = {"hip": lambda: obj.compare_sums(xs, ys)}
        if not args.only_hip:
            impls["torch_gpu_stacked"] = lambda: torch_sums(X, Y).cpu()
            impls["torch_gpu_per_pair"] = lambda: torch.cat([torch_sums(X[p:p + 1], Y[p:p + 1]) for p in range(P)]).cpu()
            s = obj.compare_sums(xs, ys)
            ours = torch.sqrt(s[..., 0] / s[..., 1]) + s[..., 2] / s[..., 3]
            theirs = torch_sums(X, Y).cpu().double()[..., 2]
            row["hip_vs_torch_gpu_max_rel_diff"] = float(((ours - theirs).abs() / theirs).max())
            del s, ours, theirs
        inner = {}
        for k, fn in impls.items():
            inner[k] = max(1, min(200, int(0.02 / max(timed(fn, 1), 1e-6))))
        times = {k: [] for k in impls}
        for _ in range(args.reps):
            for k, fn in impls.items():
                times[k].append(timed(fn, inner[k]))
        for k, v in times.items():
            row[k + "_ms"] = round(1e3 * statistics.median(v), 4)
            row[k + "_min_ms"] = round(1e3 * min(v), 4)
            row[k + "_inner"] = inner[k]
        row["hip_mfma_tflops"] = round(P * flop / (1e9 * row["hip_ms"]), 2)
        out["points"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del X, Y, xs, ys
    if not args.only_hip:
        ratios = []
        odd = MultiResolutionSTFT(STFTConfig(resolutions=[SR.ODD])).to(dev)
        all_res = SR.RESOLUTIONS + (SR.ODD,)
        for res in all_res:
            o, ri = (odd, 0) if res == SR.ODD else (obj, SR.RESOLUTIONS.index(res))
            for L in (1025, 1025 + res[1], 2400, 24000, 33 * res[1]):
                for amp in (0.1, 1.0):
                    x = SR.make_clear_noise(L, L + 7 * all_res.index(res) + (100003 if amp == 1.0 else 0), amp, [res])  # the test's inputs
                    m64 = SR.magnitude(x, res).numpy()
                    m32 = SR.magnitude(x, res, torch.float32).numpy().astype(np.float64)
                    got = o.magnitude(x.to(dev), ri).cpu().numpy().astype(np.float64)
                    floor, err = float(np.abs(m32 - m64).max()), float(np.abs(got - m64).max())
                    lfloor, lerr = float(np.abs(np.log(m32) - np.log(m64)).max()), float(np.abs(np.log(got) - np.log(m64)).max())
                    ratios.append({"res": list(res), "L": L, "amp": amp, "floor": floor, "engine": err, "ratio": round(err / floor, 3),
                                   "log_floor": lfloor, "log_engine": lerr, "log_ratio": round(lerr / lfloor, 3)})
        out["parity"] = ratios
        out["parity_ratio_range"] = [min(r["ratio"] for r in ratios), max(r["ratio"] for r in ratios)]
        out["parity_log_ratio_range"] = [min(r["log_ratio"] for r in ratios), max(r["log_ratio"] for r in ratios)]
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
