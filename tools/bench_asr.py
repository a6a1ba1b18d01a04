"""CTC recogniser time for (B, seconds) = (1, 3), (1, 10), (32, 10) and (64, 20) at two configurations: `base` (Wav2Vec2Config()
defaults: 12 layers, group / post-norm, the widths of wav2vec2-base-960h) and `large` (24 layers of 1024 / 16 heads / 4096, layer /
stable with convolution biases, the widths of hubert-large-ls960-ft): `SpeechRecognizer.recognize` (HIP; device 16 kHz waveforms in,
transcripts on the host out, one ragged call) against the restatement tests/asr_ref.forward on stock torch GPU ops in fp32 followed
by an argmax.  Torch runs per utterance: a padded batch is a different function (the group flavour's GroupNorm statistics take the
padding in, and both flavours' attention needs a mask).  Weights are `asr.synthetic_state_dict(seed 0)`: seeded, not trained.
One JSON line on stdout, the same object written to --out.

    python tools/bench_asr.py [--reps 3] [--points 1x3,1x10,32x10,64x20] [--configs base,large] [--precision fp32|bf16|both]

`--precision both` times the fp32 handle and the bf16 encoder mode (`SpeechRecognizer(precision="bf16")`, the layer / stable flavour
only: `base` is refused and recorded so) of the same build in one invocation, the timed reps alternating; the rows go to
profiles/asr_bf16_times.json (the default --out of any precision but fp32; profiles/asr_times.json keeps the fp32 record) with the
spread (max - min) of the reps.  The handle has no device-event split: the two modes differ in the encoder layers' launches and in
nothing else, so the difference of the whole calls is the encoder's; `encoder_layer_flops` is B L (2 T (4 d d + 2 d ffn) + 4 T T d).

Each point is warmed per implementation, then timed with device events around `inner` back-to-back calls (chosen so that a rep
lasts about 50 ms or more); the figure is the best of the reps.  The HIP figure includes the copy of the token ids to the host and
their conversion to text; the torch figure ends at the argmax on the device.  An implementation that fails at a point (out of
memory) is recorded as "not measured" with the reason."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = {
    "base": dict(),
    "large": dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=24, feat_extract_norm="layer",
                 do_stable_layer_norm=True, conv_bias=True),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", default="1x3,1x10,32x10,64x20", help="BxSECONDS,...")
    ap.add_argument("--configs", default="base,large")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16", "both"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    precisions = ("fp32", "bf16") if args.precision == "both" else (args.precision,)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "asr_times.json" if args.precision == "fp32" else "asr_bf16_times.json")
    import torch

    import __graft_entry__ as ge

    ge.build()
    import asr_cases as AC
    import asr_ref as R
    from valle_amd.asr import RecognizerConfig, SpeechRecognizer, synthetic_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("bench_asr.py measures on the GPU; none found")
    dev = "cuda:0"
    points = [tuple(int(v) for v in p.split("x")) for p in args.points.split(",")]
    vocab = {t: i for i, t in enumerate(AC.VOCAB32)}

    def timed(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner  # ms

    out = {"bench": "asr", "reps": args.reps, "weights": "asr.synthetic_state_dict(seed 0): seeded, not trained",
           "timer": "device events, best of reps", "points": []}
    for name in args.configs.split(","):
        cfg = RecognizerConfig(**CONFIGS[name])
        sd = synthetic_state_dict(cfg, 0)
        rsd = {k: v.to(dev) for k, v in AC.ref_state_dict(sd).items()}
        for B, sec in points:
            n = 16000 * sec
            row = {"config": name, "B": B, "seconds": sec, "samples": n}
            print(f"{name} {B}x{sec}s", file=sys.stderr, flush=True)
            recs = {}
            try:
                for prec in precisions:
                    recs[prec] = SpeechRecognizer(cfg, vocab, max_batch=B, max_seconds=sec, state_dict=sd, precision=prec).to(dev)
                    row["workspace_bytes" + ("" if prec == "fp32" else "_" + prec)] = recs[prec].workspace_bytes()
                rec = recs[precisions[0]]
                row["frames"] = rec.num_frames(n)
            except Exception as e:  # a geometry the handle refuses
                row["hip"] = "not measured: " + str(e).splitlines()[0][:200]
                out["points"].append(row)
                for r in recs.values():
                    r.close()
                continue
            g = torch.Generator().manual_seed(B * 100 + sec)
            wavs = [(0.3 * torch.randn(n, generator=g)).to(dev) for _ in range(B)]
            impls = {("hip" if prec == "fp32" else "hip_" + prec): (lambda r: lambda: r.recognize(wavs, sr=16000))(recs[prec]) for prec in precisions}
            impls = {**impls, "torch_gpu_per_utterance": lambda: [R.forward(rsd, cfg, w, torch.float32)["logits"].argmax(1) for w in wavs]}
            n_impls = len(impls)
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
            if len(ok) == n_impls:
                with torch.no_grad():
                    ours, theirs = rec.logits(wavs[:1], sr=16000)[0], R.forward(rsd, cfg, wavs[0], torch.float32)["logits"]
                row["hip_vs_torch_gpu_max_abs_diff"] = float((ours - theirs).abs().max())
                row["logits_max_abs"] = float(theirs.abs().max())
            times = {k: [] for k in ok}
            with torch.no_grad():
                for _ in range(args.reps):
                    for k, fn in ok.items():
                        times[k].append(timed(fn, inner[k]))
            for k, v in times.items():
                row[k + "_ms"] = round(min(v), 4)
                row[k + "_ms_spread"] = round(max(v) - min(v), 4)
                row[k + "_inner"] = inner[k]
            if "hip" in times and "hip_bf16" in times:
                T, d, f, L = row["frames"], int(cfg.hidden_size), int(cfg.intermediate_size), int(cfg.num_hidden_layers)
                row["encoder_layer_flops"] = B * L * (2 * T * (4 * d * d + 2 * d * f) + 4 * T * T * d)
                row["hip_fp32_over_bf16"] = round(row["hip_ms"] / row["hip_bf16_ms"], 3)
                row["bf16_faster_by_more_than_the_spread"] = bool(row["hip_ms"] - row["hip_bf16_ms"] > max(row["hip_ms_spread"], row["hip_bf16_ms_spread"]))
                with torch.no_grad():
                    a, b = recs["fp32"].recognize(wavs, sr=16000), recs["bf16"].recognize(wavs, sr=16000)
                row["same_transcript_share"] = sum(x.tokens == y.tokens for x, y in zip(a, b)) / B
            if "hip" in times:
                row["hip_realtime_factor"] = round(B * sec / (row["hip_ms"] * 1e-3), 1)  # seconds of audio per second
            for k in times:
                if k.startswith("hip") and "torch_gpu_per_utterance" in times:
                    row["torch_over_" + k] = round(row["torch_gpu_per_utterance_ms"] / row[k + "_ms"], 3)
            out["points"].append(row)
            for r in recs.values():
                r.close()
            del wavs
            torch.cuda.empty_cache()
            with open(args.out, "w") as f:  # kept up to date point by point: a run that is cut short leaves what it measured
                json.dump(out, f, indent=1)
                f.write("\n")
        del rsd
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
