"""Whisper recogniser time for B x 10 s of audio, B = 1, 8, 32, at two shapes: `tiny` (whisper-tiny: d 384, 6 heads, 4 + 4 layers,
80 mels) and `turbo` (whisper-large-v3-turbo: d 1280, 20 heads, 32 + 4 layers, 128 mels), both with 1500 source and 448 target
positions: `WhisperRecognizer.recognize` (HIP; device 16 kHz waveforms in, token lists on the host out, one ragged call) against
`WhisperForConditionalGeneration` in fp32 on the GPU with the same weights driven by `GenerationMixin.generate(do_sample=False)`.
Weights are `whisper.synthetic_state_dict(seed 0)`: seeded, not trained.  eos is suppressed and the cap is 40 new tokens, so both
sides do the same work.  The transformers figure starts from ready log-mel features (the restatement's, computed outside the timed
region); the HIP figure includes its log-mel.  One JSON line on stdout, the same object written to --out.

    python tools/bench_whisper.py [--reps 3] [--batches 1,8,32] [--configs tiny,turbo] [--precision fp32|bf16|both]

`--precision both` times the fp32 and the bf16 encoder mode (`WhisperRecognizer(precision=...)`) of the same build in one invocation,
the timed calls alternating between the two, and `transformers` in fp32 and in `torch.bfloat16` from the same features, the tokens
checked against each; a row per precision goes to profiles/whisper_bf16_times.json (the default --out of any precision but fp32;
profiles/whisper_times.json keeps the fp32 record), with the spread (max - min) of the repeats, the fp32 / bf16 factor of
`encoder_ms`, and the encoder's bf16 rate: the layers' shape-derived flops, B L (2 P (4 d d + 2 d ffn) + 4 P P d), over the whole
`encoder_ms`, which also holds conv1 / conv2 and the cross-attention projections (fp32), so the figure is a lower bound of the layers'.

Each point is warmed per implementation, then timed with device events; the figure is the best of the reps.  Recorded next to it:
workspace bytes, the device time of log-mel / encoder (cross keys and values included) / token loop from the handle's own events,
and the token loop's time per step against its weight-streaming floor (the decoder's and the head's weight bytes at 8 TB/s)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

_COMMON = dict(max_source_positions=1500, max_target_positions=448, eos_token_id=50257, decoder_start_token_id=50258)
CONFIGS = {
    "tiny": dict(_COMMON, vocab_size=51865, num_mel_bins=80, d_model=384, encoder_layers=4, decoder_layers=4, encoder_attention_heads=6,
                 decoder_attention_heads=6, encoder_ffn_dim=1536, decoder_ffn_dim=1536),
    "turbo": dict(_COMMON, vocab_size=51866, num_mel_bins=128, d_model=1280, encoder_layers=32, decoder_layers=4, encoder_attention_heads=20,
                  decoder_attention_heads=20, encoder_ffn_dim=5120, decoder_ffn_dim=5120),
}
NEW_TOKENS, SECONDS, HBM_BYTES_PER_S = 40, 10, 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--configs", default="tiny,turbo")
    ap.add_argument("--no-transformers", action="store_true")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16", "both"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    precisions = ("fp32", "bf16") if args.precision == "both" else (args.precision,)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "whisper_times.json" if args.precision == "fp32" else "whisper_bf16_times.json")
    import torch

    import __graft_entry__ as ge

    ge.build()
    import whisper_ref as R
    from valle_amd.whisper import WhisperConfig, WhisperRecognizer, mel_filters, synthetic_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("bench_whisper.py measures on the GPU; none found")
    dev = "cuda:0"

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)  # ms

    out = {"bench": "whisper", "reps": args.reps, "weights": "whisper.synthetic_state_dict(seed 0): seeded, not trained",
           "timer": "device events, best of reps" + (", the precisions alternating; spread = max - min of the reps" if len(precisions) > 1 else ""),
           "new_tokens": NEW_TOKENS, "seconds": SECONDS, "points": []}
    for name in args.configs.split(","):
        cfg = WhisperConfig(**CONFIGS[name])
        sd = synthetic_state_dict(cfg, 0)
        prompt = [cfg.decoder_start_token_id, 50259, 50359, 50363]
        gen = dict(suppress_tokens=[cfg.eos_token_id], eos_token_id=cfg.eos_token_id, decoder_start_token_id=cfg.decoder_start_token_id)
        d, f, V, L = cfg.d_model, cfg.decoder_ffn_dim, cfg.vocab_size, cfg.decoder_layers
        step_bytes = 4 * (L * (8 * d * d + 2 * d * f) + V * d)  # self q k v out, cross q out, the FFN, the head; the cross k v are not per step
        enc_flops = cfg.encoder_layers * (2 * cfg.max_source_positions * (4 * d * d + 2 * d * cfg.encoder_ffn_dim)
                                          + 4 * cfg.max_source_positions ** 2 * d)  # per utterance, the layers alone
        hf = None
        hf16 = None
        if not args.no_transformers:
            try:
                import transformers as tf

                hcfg = tf.WhisperConfig(**CONFIGS[name], pad_token_id=cfg.eos_token_id, bos_token_id=cfg.eos_token_id, suppress_tokens=None,
                                        begin_suppress_tokens=None)
                with torch.device("meta"):
                    hf = tf.WhisperForConditionalGeneration(hcfg)
                hf = hf.to_empty(device=dev).eval()
                hf.load_state_dict({k: v.to(dev) for k, v in sd.items()}, strict=True)
                hf.tie_weights()
                if "bf16" in precisions:
                    import copy

                    hf16 = copy.deepcopy(hf).to(torch.bfloat16)
            except Exception as e:  # the comparison is optional
                hf, out["transformers_" + name] = None, "not measured: " + str(e).splitlines()[0][:200]
        for B in [int(b) for b in args.batches.split(",")]:
            print(f"{name} {B}x{SECONDS}s", file=sys.stderr, flush=True)
            g = torch.Generator().manual_seed(B)
            wavs = [(0.3 * torch.randn(16000 * SECONDS, generator=g)).to(dev) for _ in range(B)]
            recs, rows, fns, hyps = {}, {}, {}, {}
            for prec in precisions:
                recs[prec] = WhisperRecognizer(cfg, None, gen, max_batch=B, state_dict=sd, precision=prec).to(dev)
                rows[prec] = {"config": name, "B": B, "precision": prec, "step_weight_bytes": step_bytes,
                              "step_floor_ms": round(step_bytes / HBM_BYTES_PER_S * 1e3, 4), "workspace_bytes": recs[prec].workspace_bytes()}
                fns[prec] = (lambda r: lambda: r.recognize(wavs, sr=16000, prompt_ids=prompt, max_new_tokens=NEW_TOKENS))(recs[prec])
                with torch.no_grad():
                    rows[prec]["hip_first_call_ms"] = round(timed(fns[prec]), 3)
                    hyps[prec] = fns[prec]()
                assert all(len(h.tokens) == NEW_TOKENS for h in hyps[prec])
            ms = {p: [] for p in precisions}
            parts = {p: [] for p in precisions}
            with torch.no_grad():
                for _ in range(args.reps):  # alternating: a drift of the clocks falls on both
                    for prec in precisions:
                        ms[prec].append(timed(fns[prec]))
                        parts[prec].append(recs[prec].timings())
            for prec in precisions:
                row, t = rows[prec], min(parts[prec], key=lambda t: t["encoder_ms"])
                row["hip_ms"] = round(min(ms[prec]), 3)
                row["hip_ms_spread"] = round(max(ms[prec]) - min(ms[prec]), 3)
                row["weight_bytes"] = int(t["weight_bytes"])
                row.update({k: round(min(q[k] for q in parts[prec]), 3) for k in ("logmel_ms", "encoder_ms", "loop_ms")})
                row["encoder_ms_spread"] = round(max(q["encoder_ms"] for q in parts[prec]) - min(q["encoder_ms"] for q in parts[prec]), 3)
                row["steps"] = int(t["steps"])
                row["loop_step_ms"] = round(row["loop_ms"] / max(t["steps"], 1), 4)
                row["loop_step_over_floor"] = round(row["loop_step_ms"] / row["step_floor_ms"], 2)
                row["encoder_layer_flops"] = B * enc_flops
                row["encoder_tflops_lower_bound"] = round(B * enc_flops / (row["encoder_ms"] * 1e-3) / 1e12, 2)
            if len(precisions) > 1:
                a, b = rows["fp32"], rows["bf16"]
                b["encoder_fp32_over_bf16"] = round(a["encoder_ms"] / b["encoder_ms"], 3)
                b["encoder_faster_by_more_than_the_spread"] = bool(a["encoder_ms"] - b["encoder_ms"] > max(a["encoder_ms_spread"], b["encoder_ms_spread"]))
                b["hip_fp32_over_bf16"] = round(a["hip_ms"] / b["hip_ms"], 3)
                b["same_tokens_as_fp32_share"] = sum(x.tokens == y.tokens for x, y in zip(hyps["fp32"], hyps["bf16"])) / B
            if hf is not None:
                try:
                    mel = mel_filters(cfg.num_mel_bins)
                    feats = torch.stack([R.logmel(w.cpu(), cfg.max_source_positions, mel, torch.float32).T for w in wavs]).to(dev)
                    ids = torch.tensor([prompt] * B, device=dev)
                    for model, key, x in ((hf, "transformers", feats), (hf16, "transformers_bf16", feats.to(torch.bfloat16))):
                        if model is None:
                            continue
                        hfn = (lambda m, x: lambda: tf.generation.GenerationMixin.generate(  # noqa: E731
                            m, x, decoder_input_ids=ids, do_sample=False, max_new_tokens=NEW_TOKENS, suppress_tokens=[cfg.eos_token_id],
                            eos_token_id=cfg.eos_token_id, pad_token_id=cfg.eos_token_id))(model, x)
                        with torch.no_grad():
                            first = round(timed(hfn), 3)
                            theirs = hfn()
                            reps = [timed(hfn) for _ in range(args.reps)]
                        for prec in precisions:
                            row = rows[prec]
                            row[key + "_first_call_ms"], row[key + "_ms"] = first, round(min(reps), 3)
                            row[key + "_ms_spread"] = round(max(reps) - min(reps), 3)
                            row[key + "_over_hip"] = round(row[key + "_ms"] / row["hip_ms"], 3)
                            row["same_tokens_share" if key == "transformers" else "same_tokens_share_" + key] = \
                                sum(h.tokens == theirs[i, len(prompt):].tolist() for i, h in enumerate(hyps[prec])) / B
                    del feats
                except RuntimeError as e:
                    for prec in precisions:
                        rows[prec]["transformers"] = "not measured: " + str(e).splitlines()[0][:200]
            for prec in precisions:
                out["points"].append(rows[prec])
                recs[prec].close()
            del wavs
            torch.cuda.empty_cache()
            with open(args.out, "w") as fh:  # kept up to date point by point: a run that is cut short leaves what it measured
                json.dump(out, fh, indent=1)
                fh.write("\n")
        del hf, hf16
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
