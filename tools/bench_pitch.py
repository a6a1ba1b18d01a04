"""Pitch-tracking time at (utterances, seconds) = (1, 3), (1, 10), (32, 10), (64, 20): `PitchTracker.track_batch` (one launch of
pitch_track_kernel per 64 utterances, device waveforms in, device tracks out) against the same definition on stock torch GPU ops:
`unfold` into half windows, the broadcast difference against the 256-sample windows at every lag, squares summed in fp32, the
halves added, `cumsum` in fp64, then the lag search with comparisons, `argmax` and `argmin` (128 half windows per step, so that
the (halves, lags, 256) differences stay at 53 MB).  Plus the error ratios of d' on the parity test's inputs.  One JSON line on
stdout, the same object written to --out.

    python tools/bench_pitch.py [--reps 5] [--points 1x3,1x10,32x10,64x20] [--out profiles/pitch_times.json]
    python tools/bench_pitch.py --only-hip --points 64x20 --reps 20      # the run to put under a kernel tracer

Each point is warmed once per implementation, then the implementations alternate rep by rep.  A rep runs the call `inner` times
back to back (chosen per implementation so that a rep lasts about 20 ms or more) and ends in a device synchronise; the figure is
the median over the reps of the rep's wall time / inner.  The waveforms are pitch_ref.make_signal, not speech."""
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
    ap.add_argument("--points", default="1x3,1x10,32x10,64x20", help="UTTERANCESxSECONDS,...")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_times.json"))
    ap.add_argument("--only-hip", action="store_true", help="time the HIP call alone (for a kernel trace); writes no file")
    args = ap.parse_args()
    import numpy as np
    import torch

    import __graft_entry__ as ge

    ge.build()
    import pitch_ref as PR
    from valle_amd import engine as E
    from valle_amd.pitch import TILE_FRAMES, PitchTracker

    if not torch.cuda.is_available():
        raise SystemExit("bench_pitch.py measures on the GPU; none found")
    dev = "cuda:0"
    points = [tuple(int(v) for v in p.split("x")) for p in args.points.split(",")]
    sync = torch.cuda.synchronize
    fmin, fmax, thr = 60.0, 600.0, 0.1
    tau_min, tau_max = PR.lag_range(fmin, fmax)
    tracker = PitchTracker(fmin, fmax, thr).to(dev)
    lags = torch.arange(1, tau_max + 1, dtype=torch.float64, device=dev)
    idx = torch.arange(tau_max + 1, device=dev)[None, :]

    @torch.no_grad()
    def torch_track(ws):
        outs = []
        for w in ws:
            T = PR.num_frames(w.numel())
            xp = torch.zeros((T + 1) * 256 + tau_max, device=dev)
            n = min(w.numel(), xp.numel())
            xp[:n] = w[:n]
            seg = xp.unfold(0, 256 + tau_max, 256)  # (T + 1, 256 + tau_max)
            h = []
            for c in seg.split(128):
                diff = c[:, None, :256] - c.unfold(1, 256, 1)  # (halves, tau_max + 1, 256)
                h.append((diff * diff).sum(-1))
            h = torch.cat(h)
            d = (h[:-1] + h[1:]).double()
            cs = torch.cumsum(d[:, 1:], 1)
            dp = torch.ones((T, tau_max + 1), device=dev)
            dp[:, 1:] = torch.where(cs > 0, d[:, 1:] * lags / cs, 1.0).float()
            under = (dp < thr) & (idx >= tau_min)
            voiced = under.any(1)
            first = torch.where(voiced, under.int().argmax(1), tau_max)
            stops = torch.ones_like(under)
            stops[:, :-1] = ~(dp[:, 1:] < dp[:, :-1])
            stop = (stops & (idx >= first[:, None])).int().argmax(1)
            lag = torch.where(voiced, stop, dp[:, tau_min:].argmin(1) + tau_min)
            outs.append((dp, lag, voiced))
        return outs

    def timed(fn, inner):
        sync()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        return (time.perf_counter() - t0) / inner

    out = {"bench": "pitch", "reps": args.reps, "band_hz": [fmin, fmax], "lags": [tau_min, tau_max], "tile_frames": TILE_FRAMES,
           "points": []}
    for P, sec in points:
        L = 24000 * sec
        ws = [torch.from_numpy(PR.make_signal(L, 10 * P + p)).to(dev) for p in range(P)]
        T = PR.num_frames(L)
        row = {"utterances": P, "seconds": sec, "frames": T, "sub_fma_pairs": P * (T + 1) * (tau_max + 1) * 256}
        impls = {"hip": lambda: tracker.track_batch(ws)}
        if not args.only_hip:
            impls["torch_gpu"] = lambda: torch_track(ws)
            ours, theirs = tracker.track_batch(ws), torch_track(ws)
            row["frames_lag_differs"] = int(sum(int((o.lag != t[1]).sum()) for o, t in zip(ours, theirs)))
            row["frames_voiced"] = int(sum(int(o.voiced.sum()) for o in ours))
            dp = E.op_pitch_diff(ws[-1], fmin, fmax, tau_max)
            row["hip_vs_torch_gpu_dprime_max_abs_diff_last"] = float((dp - theirs[-1][0]).abs().max())
            del ours, theirs, dp
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
        row["hip_g_pairs_per_s"] = round(row["sub_fma_pairs"] / (1e6 * row["hip_ms"]), 1)
        out["points"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if not args.only_hip:
        ratios = []
        for band in PR.BANDS:
            for L in PR.LENGTHS:
                if PR.num_frames(L) == 0:
                    continue
                x = PR.make_signal(L, PR.SEEDS[L])
                ref64 = PR.cmnd(x, *band)
                floor = float(np.abs(PR.cmnd(x, *band, dtype=np.float32).astype(np.float64) - ref64).max())
                got = E.op_pitch_diff(torch.from_numpy(x).to(dev), band[0], band[1], PR.lag_range(*band)[1]).cpu().numpy()
                err = float(np.abs(got.astype(np.float64) - ref64).max())
                ratios.append({"L": L, "band": list(band), "floor": floor, "engine": err, "ratio": round(err / floor, 3)})
        out["parity"] = ratios
        out["parity_ratio_max"] = max(r["ratio"] for r in ratios)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
