"""HiFi-GAN / BigVGAN generator time at (B, seconds) = (1, 3), (1, 10), (32, 10) for the two 24 kHz presets: `GanVocoder.synthesize_batch`
(HIP; device log-mels in, device waveforms out) against the same definition on stock torch GPU ops in fp32, batched over the
equal-length utterances (`F.conv1d`, `F.conv_transpose1d`, and the anti-aliased activation as replicate pad, grouped
`conv_transpose1d`, crop, Snake, replicate pad, grouped strided `conv1d`).  Weights are tests/ganvoc_ref.make_weights' seeded ones.
One JSON line on stdout, the same object written to --out.

    python tools/bench_ganvoc.py [--reps 5] [--points 1x3,1x10,32x10] [--presets bigvgan_base_24khz_100band,bigvgan_24khz_100band]
    python tools/bench_ganvoc.py --only-hip --points 1x10 --reps 3       # the run to put under a kernel tracer

Each point is warmed per implementation, then the implementations alternate rep by rep.  A rep runs the call `inner` times back
to back (chosen per implementation so that a rep lasts about 20 ms or more) and ends in a device synchronise; the figure is the
median over the reps of the rep's wall time / inner.  An implementation that fails at a point (out of memory, a missing library)
is recorded as "not measured" with the reason."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_forward_batched(w, cfg, mel, taps):
    """mel (B, T, n_mels) -> (B, T * hop): ganvoc_ref.forward for a batch of equal lengths, in mel's dtype on mel's device."""
    import torch
    import torch.nn.functional as F

    lrelu, slope, R = cfg["activation"] == "lrelu", cfg["lrelu_slope"], len(cfg["resblock_kernels"])
    f = taps.to(mel.dtype)

    def act(h, name):
        if lrelu:
            return F.leaky_relu(h, slope)
        a = w[name + ".alpha"]
        b = w[name + ".beta"] if cfg["activation"] == "snakebeta" else a
        if cfg["alpha_logscale"]:
            a, b = torch.exp(a), torch.exp(b)
        Cc, L = h.shape[1], h.shape[2]
        k = f.reshape(1, 1, 12).expand(Cc, 1, 12)
        u = 2.0 * F.conv_transpose1d(F.pad(h, (5, 5), mode="replicate"), k, stride=2, groups=Cc)[:, :, 15: 15 + 2 * L]
        v = u + torch.sin(u * a[None, :, None]) ** 2 / (b[None, :, None] + 1e-9)
        return F.conv1d(F.pad(v, (5, 6), mode="replicate"), k, stride=2, groups=Cc)

    x = F.conv1d(mel.transpose(1, 2), w["conv_pre.weight"], w["conv_pre.bias"], padding=3)
    for i, (u, k) in enumerate(zip(cfg["rates"], cfg["kernels"])):
        if lrelu:
            x = F.leaky_relu(x, slope)
        x = F.conv_transpose1d(x, w[f"ups.{i}.weight"], w[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2)
        xs = None
        for r, rk in enumerate(cfg["resblock_kernels"]):
            n, h = i * R + r, x
            for m, d in enumerate(cfg["dilations"][r]):
                xt = act(h, f"resblocks.{n}.activations.{2 * m}")
                xt = F.conv1d(xt, w[f"resblocks.{n}.convs1.{m}.weight"], w[f"resblocks.{n}.convs1.{m}.bias"], dilation=d,
                              padding=d * (rk - 1) // 2)
                xt = act(xt, f"resblocks.{n}.activations.{2 * m + 1}")
                xt = F.conv1d(xt, w[f"resblocks.{n}.convs2.{m}.weight"], w[f"resblocks.{n}.convs2.{m}.bias"], padding=(rk - 1) // 2)
                h = h + xt
            xs = h if xs is None else xs + h
        x = xs / R
    x = F.leaky_relu(x, 0.01) if lrelu else act(x, "activation_post")
    return torch.tanh(F.conv1d(x, w["conv_post.weight"], w.get("conv_post.bias"), padding=3))[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", default="1x3,1x10,32x10", help="BxSECONDS,...")
    ap.add_argument("--presets", default="bigvgan_base_24khz_100band,bigvgan_24khz_100band")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ganvoc_times.json"))
    ap.add_argument("--only-hip", action="store_true", help="time the HIP call alone (for a kernel trace); writes no file")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge

    ge.build()
    import ganvoc_ref as GR
    from valle_amd.ganvoc import PRESETS, GanVocoder

    if not torch.cuda.is_available():
        raise SystemExit("bench_ganvoc.py measures on the GPU; none found")
    dev = "cuda:0"
    points = [tuple(int(v) for v in p.split("x")) for p in args.points.split(",")]
    sync = torch.cuda.synchronize

    def timed(fn, inner):
        sync()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        return (time.perf_counter() - t0) / inner

    out = {"bench": "ganvoc", "reps": args.reps, "weights": "ganvoc_ref.make_weights(seed 1, calib_T 4): seeded, not trained", "points": []}
    for preset in args.presets.split(","):
        c = PRESETS[preset]
        cfg = dict(n_mels=c.n_mels, rates=tuple(c.rates), kernels=tuple(c.kernels), initial_channels=c.initial_channels,
                   resblock_kernels=tuple(c.resblock_kernels), dilations=tuple(tuple(d) for d in c.dilations),
                   activation=c.activation, alpha_logscale=c.alpha_logscale, lrelu_slope=c.lrelu_slope)
        w = GR.make_weights(cfg, 1, calib_T=4)
        voc = GanVocoder(cfg, state_dict=w, max_batch=max(b for b, _ in points), max_total_frames=1 << 17).to(dev)
        wd = {k: v.to(dev) for k, v in w.items()}
        taps = voc.filter.to(dev)
        for B, sec in points:
            T = 24000 * sec // 256
            mels = [GR.logmel(T, seed=b + 1).to(dev) for b in range(B)]
            stacked = torch.stack(mels)
            row = {"preset": preset, "B": B, "seconds": sec, "frames": T, "samples": 256 * T}
            impls = {"hip": lambda: voc.synthesize_batch(mels)}
            if not args.only_hip:
                impls["torch_gpu_batched"] = lambda: torch_forward_batched(wd, cfg, stacked, taps)
            print(f"{preset} {B}x{sec}s", file=sys.stderr, flush=True)
            inner, ok = {}, {}
            for k, fn in impls.items():
                try:
                    with torch.no_grad():
                        t_first = timed(fn, 1)
                        inner[k] = max(1, min(200, int(0.02 / max(timed(fn, 1), 1e-6))))
                    row[k + "_first_call_ms"] = round(1e3 * t_first, 3)
                    ok[k] = fn
                except RuntimeError as e:
                    row[k] = "not measured: " + str(e).splitlines()[0][:200]
                    torch.cuda.empty_cache()
                print(f"  {k} warmed", file=sys.stderr, flush=True)
            if len(ok) == 2:
                with torch.no_grad():
                    ours, theirs = torch.stack(voc.synthesize_batch(mels[:1])), torch_forward_batched(wd, cfg, stacked[:1], taps)
                row["hip_vs_torch_gpu_max_abs_diff"] = float((ours - theirs).abs().max())
                del ours, theirs
            times = {k: [] for k in ok}
            with torch.no_grad():
                for _ in range(args.reps):
                    for k, fn in ok.items():
                        times[k].append(timed(fn, inner[k]))
            for k, v in times.items():
                row[k + "_ms"] = round(1e3 * statistics.median(v), 4)
                row[k + "_min_ms"] = round(1e3 * min(v), 4)
                row[k + "_inner"] = inner[k]
            if len(ok) == 2:
                row["torch_over_hip"] = round(row["torch_gpu_batched_ms"] / row["hip_ms"], 3)
            out["points"].append(row)
            del mels, stacked
            torch.cuda.empty_cache()
            if not args.only_hip:  # kept up to date point by point: a long run that is cut short leaves what it measured
                with open(args.out, "w") as f:
                    json.dump(out, f, indent=1)
                    f.write("\n")
        voc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
