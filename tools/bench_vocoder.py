"""Griffin-Lim vocoder time at (B, seconds) = (1, 3), (1, 10), (32, 10), (64, 20), 32 iterations: `GriffinLim.synthesize_batch`
(HIP: one launch for the magnitudes, two per iteration; device log-mels in, device waveforms out) against the same definition
on stock torch GPU ops, batched over the equal-length utterances (exp, matmul with the inverse table, clamp; per iteration
`torch.fft.irfft`, window, `F.fold` as the overlap-add, the floored envelope, zero padding, `unfold`, window, `torch.fft.rfft`, the
momentum update).  One JSON line on stdout, the same object written to --out.

    python tools/bench_vocoder.py [--reps 7] [--points 1x3,1x10,32x10,64x20] [--n-iter 32] [--out profiles/vocoder_times.json]
    python tools/bench_vocoder.py --only-hip --points 64x20 --reps 5      # the run to put under a kernel tracer

Each point is warmed per implementation, then the implementations alternate rep by rep.  A rep runs the call `inner` times back
to back (chosen per implementation so that a rep lasts about 20 ms or more) and ends in a device synchronise; the figure is the
median over the reps of the rep's wall time / inner."""
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", default="1x3,1x10,32x10,64x20", help="BxSECONDS,...")
    ap.add_argument("--n-iter", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocoder_times.json"))
    ap.add_argument("--only-hip", action="store_true", help="time the HIP call alone (for a kernel trace); writes no file")
    args = ap.parse_args()
    write = not args.only_hip
    import torch
    import torch.nn.functional as F

    import __graft_entry__ as ge

    ge.build()
    import fbank_ref as FR
    from valle_amd.fbank import BigVGANFbank
    from valle_amd.vocoder import ENV_FLOOR, TILE_FRAMES, GriffinLim

    if not torch.cuda.is_available():
        raise SystemExit("bench_vocoder.py measures on the GPU; none found")
    dev = "cuda:0"
    points = [tuple(int(v) for v in p.split("x")) for p in args.points.split(",")]
    n_iter, momentum = args.n_iter, 0.99
    gl = GriffinLim(max_batch=max(b for b, _ in points)).to(dev)
    fb = BigVGANFbank(max_batch=max(b for b, _ in points)).to(dev)
    P_t = gl.inverse.to(dev).T.contiguous()  # (n_mels, 513)
    window = torch.hann_window(1024, device=dev)
    sync = torch.cuda.synchronize

    @torch.no_grad()
    def torch_griffinlim(logmel, iters=n_iter):
        """logmel (B, T, 100) on the device -> (B, 256 T): the definition on stock ops."""
        B, T, _ = logmel.shape
        L = 256 * T + 768
        mag = torch.clamp(torch.exp(logmel) @ P_t, min=0.0)
        w2 = (window * window)[None, :, None].expand(1, 1024, T)
        env = F.fold(w2, (1, L), (1, 1024), stride=(1, 256)).reshape(1, L).clamp(min=ENV_FLOOR)
        c = momentum / (1.0 + momentum)

        def inverse(X):
            frames = torch.fft.irfft(X, n=1024, dim=2) * window
            ola = F.fold(frames.transpose(1, 2), (1, L), (1, 1024), stride=(1, 256)).reshape(B, L)
            return (ola / env)[:, : 256 * T]

        ang = torch.ones_like(mag, dtype=torch.complex64)
        tprev = torch.zeros_like(ang)
        for _ in range(iters):
            y = F.pad(inverse(mag * ang), (0, 768))
            reb = torch.fft.rfft(y.unfold(1, 1024, 256) * window, dim=2)
            a = reb - tprev * c
            ang = a / (a.abs() + 1e-16)
            tprev = reb
        return inverse(mag * ang)

    def timed(fn, inner):
        sync()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        return (time.perf_counter() - t0) / inner

    out = {"bench": "vocoder", "reps": args.reps, "n_iter": n_iter, "momentum": momentum, "tile_frames": TILE_FRAMES, "points": []}
    if not args.only_hip:
        try:  # torch.fft on the device needs the FFT library of the torch build
            torch_griffinlim(torch.zeros(1, 5, 100, device=dev))
            sync()
        except RuntimeError as e:
            out["torch_gpu_batched"] = "not measured: " + str(e).splitlines()[0][:200]
            args.only_hip = True
    for B, sec in points:
        wavs = [FR.make_noise(24000 * sec, 500 + b, 0.3).to(dev) for b in range(B)]
        mels = fb.extract_batch(wavs)
        stacked = torch.stack(mels)
        T = stacked.shape[1]
        impls = {"hip": lambda: gl.synthesize_batch(mels, n_iter=n_iter, momentum=momentum)}
        row = {"B": B, "seconds": sec, "frames": T, "samples": 256 * T}
        if not args.only_hip:
            impls["torch_gpu_batched"] = lambda: torch_griffinlim(stacked)
            ours = torch.stack(gl.synthesize_batch(mels, n_iter=0))
            row["hip_vs_torch_gpu_max_abs_diff_n_iter_0"] = float((ours - torch_griffinlim(stacked, 0)).abs().max())
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
        if "torch_gpu_batched" in impls:
            row["torch_over_hip"] = round(row["torch_gpu_batched_ms"] / row["hip_ms"], 3)
        out["points"].append(row)
    if write:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
