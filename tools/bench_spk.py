"""Speaker encoder time at the default configuration (WavLM base widths, 12 layers, weighted layer sum) for (B, seconds) = (1, 3),
(1, 10), (32, 10) and (64, 20): `SpeakerEncoder.embed` (HIP; device 16 kHz waveforms in, device embeddings out, one ragged call)
against the restatement tests/spk_ref.forward on stock torch GPU ops in fp32.  Torch runs per utterance: a padded batch is a
different function (its GroupNorm statistics take the padding in).  Weights are `spk.synthetic_state_dict(seed 0)`: seeded, not
trained.  One JSON line on stdout, the same object written to --out.

    python tools/bench_spk.py [--reps 3] [--points 1x3,1x10,32x10,64x20]
    python tools/bench_spk.py --only-hip --points 32x10        # the run to put under a kernel tracer

Each point is warmed per implementation, then timed with device events around `inner` back-to-back calls (chosen so that a rep
lasts about 50 ms or more); the figure is the best of the reps.  `hip_share_of_fp32_matrix_peak` is the whole call's: the FLOPs of
every convolution, Linear and attention product, counted from the shapes (`gemm_flops`), over the call's time and the 157.3 TFLOP/s
of the fp32 matrix instruction.  The share the convolution and FFN GEMMs reach on their own comes from kernel times: run the
`--only-hip` form under a kernel tracer and divide `gemm_flops`' stages by the time of their launches
(profiles/spk_kernel_stats_32x10.json).  An implementation that fails at a point (out of memory) is recorded as "not measured" with
the reason."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_F32_MATRIX = 157.3e12


def gemm_flops(c, n_samples):
    """FLOPs (2 per multiply-add) of one utterance's convolution / Linear GEMMs and of its attention products, by stage."""
    out = {}
    L, cin, conv = n_samples, 1, 0
    for i, (co, k, s) in enumerate(zip(c.conv_dim, c.conv_kernel, c.conv_stride)):
        L = (L - k) // s + 1
        if i > 0:
            conv += 2 * L * co * cin * k
        cin = co
    T, d, f = L, c.hidden_size, c.intermediate_size
    out["conv"] = conv
    out["proj"] = 2 * T * d * cin
    out["pos_conv"] = 2 * T * d * (d // c.num_conv_pos_embedding_groups) * c.num_conv_pos_embeddings
    out["qkv_out"] = c.num_hidden_layers * 2 * T * d * 4 * d
    out["ffn"] = c.num_hidden_layers * 2 * T * d * 2 * f
    out["attention"] = c.num_hidden_layers * 4 * T * T * d
    head, cin, Tt = 2 * T * d * c.tdnn_dim[0], c.tdnn_dim[0], T
    for co, k, dl in zip(c.tdnn_dim, c.tdnn_kernel, c.tdnn_dilation):
        Tt -= dl * (k - 1)
        head += 2 * Tt * co * cin * k
        cin = co
    out["head"] = head
    out["total"] = sum(out.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", default="1x3,1x10,32x10,64x20", help="BxSECONDS,...")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spk_times.json"))
    ap.add_argument("--only-hip", action="store_true", help="time the HIP call alone (for a kernel trace); writes no file")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge

    ge.build()
    import spk_cases as SC
    import spk_ref as R
    from valle_amd.spk import PRESETS, SpeakerEncoder, synthetic_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("bench_spk.py measures on the GPU; none found")
    dev = "cuda:0"
    points = [tuple(int(v) for v in p.split("x")) for p in args.points.split(",")]
    cfg = PRESETS["wavlm_base_plus_sv"]
    sd = synthetic_state_dict(cfg, 0)
    rsd = {k: v.to(dev) for k, v in SC.ref_state_dict(sd).items()}

    def timed(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner  # ms

    out = {"bench": "spk", "reps": args.reps, "config": "wavlm_base_plus_sv (WavLMConfig() defaults, weighted layer sum)",
           "weights": "spk.synthetic_state_dict(seed 0): seeded, not trained", "timer": "device events, best of reps", "points": []}
    for B, sec in points:
        n = 16000 * sec
        row = {"B": B, "seconds": sec, "samples": n}
        print(f"{B}x{sec}s", file=sys.stderr, flush=True)
        try:
            enc = SpeakerEncoder(cfg, max_batch=B, max_seconds=sec, state_dict=sd).to(dev)
            row["workspace_bytes"] = enc.workspace_bytes()
            row["frames"] = enc.num_frames(n)
        except Exception as e:  # a geometry the handle refuses
            row["hip"] = "not measured: " + str(e).splitlines()[0][:200]
            out["points"].append(row)
            continue
        g = torch.Generator().manual_seed(B * 100 + sec)
        wavs = [(0.3 * torch.randn(n, generator=g)).to(dev) for _ in range(B)]
        impls = {"hip": lambda: enc.embed(wavs, sr=16000)}
        if not args.only_hip:
            impls["torch_gpu_per_utterance"] = lambda: [R.forward(rsd, cfg, w, torch.float32, "wavlm")["embedding"] for w in wavs]
        inner, ok = {}, {}
        for k, fn in impls.items():
            try:
                with torch.no_grad():
                    first = timed(fn, 1)
                    inner[k] = max(1, min(100, int(50.0 / max(timed(fn, 1), 1e-3))))
                row[k + "_first_call_ms"] = round(first, 3)
                ok[k] = fn
            except RuntimeError as e:
                row[k] = "not measured: " + str(e).splitlines()[0][:200]
                torch.cuda.empty_cache()
        if len(ok) == 2:
            with torch.no_grad():
                ours, theirs = enc.embed(wavs[:1], sr=16000)[0], R.forward(rsd, cfg, wavs[0], torch.float32, "wavlm")["embedding"]
            row["hip_vs_torch_gpu_max_abs_diff"] = float((ours - theirs).abs().max())
            row["embedding_max_abs"] = float(theirs.abs().max())
        times = {k: [] for k in ok}
        with torch.no_grad():
            for _ in range(args.reps):
                for k, fn in ok.items():
                    times[k].append(timed(fn, inner[k]))
        for k, v in times.items():
            row[k + "_ms"] = round(min(v), 4)
            row[k + "_inner"] = inner[k]
        if "hip" in times:
            fl = gemm_flops(cfg, n)
            row["gemm_flops_per_utterance"] = fl
            row["hip_tflops"] = round(B * fl["total"] / (row["hip_ms"] * 1e-3) / 1e12, 2)
            row["hip_share_of_fp32_matrix_peak"] = round(B * fl["total"] / (row["hip_ms"] * 1e-3) / PEAK_F32_MATRIX, 4)
        if len(ok) == 2:
            row["torch_over_hip"] = round(row["torch_gpu_per_utterance_ms"] / row["hip_ms"], 3)
        out["points"].append(row)
        enc.close()
        del wavs
        torch.cuda.empty_cache()
        if not args.only_hip:  # kept up to date point by point: a run that is cut short leaves what it measured
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
