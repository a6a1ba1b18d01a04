"""Whisper recogniser time for B x 10 s of audio, B = 1, 8, 32, at two shapes: `tiny` (whisper-tiny: d 384, 6 heads, 4 + 4 layers,
80 mels) and `turbo` (whisper-large-v3-turbo: d 1280, 20 heads, 32 + 4 layers, 128 mels), both with 1500 source and 448 target
positions: `WhisperRecognizer.recognize` (HIP; device 16 kHz waveforms in, token lists on the host out, one ragged call) against
`WhisperForConditionalGeneration` in fp32 on the GPU with the same weights driven by `GenerationMixin.generate(do_sample=False)`.
Weights are `whisper.synthetic_state_dict(seed 0)`: seeded, not trained.  eos is suppressed and the cap is 40 new tokens, so both
sides do the same work.  The transformers figure starts from ready log-mel features (the restatement's, computed outside the timed
region); the HIP figure includes its log-mel.  One JSON line on stdout, the same object written to --out.

    python tools/bench_whisper.py [--reps 3] [--batches 1,8,32] [--configs tiny,turbo]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whisper_times.json"))
    args = ap.parse_args()
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
           "timer": "device events, best of reps", "new_tokens": NEW_TOKENS, "seconds": SECONDS, "points": []}
    for name in args.configs.split(","):
        cfg = WhisperConfig(**CONFIGS[name])
        sd = synthetic_state_dict(cfg, 0)
        prompt = [cfg.decoder_start_token_id, 50259, 50359, 50363]
        gen = dict(suppress_tokens=[cfg.eos_token_id], eos_token_id=cfg.eos_token_id, decoder_start_token_id=cfg.decoder_start_token_id)
        d, f, V, L = cfg.d_model, cfg.decoder_ffn_dim, cfg.vocab_size, cfg.decoder_layers
        step_bytes = 4 * (L * (8 * d * d + 2 * d * f) + V * d)  # self q k v out, cross q out, the FFN, the head; the cross k v are not per step
        hf = None
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
            except Exception as e:  # the comparison is optional
                hf, out["transformers_" + name] = None, "not measured: " + str(e).splitlines()[0][:200]
        for B in [int(b) for b in args.batches.split(",")]:
            row = {"config": name, "B": B, "step_weight_bytes": step_bytes, "step_floor_ms": round(step_bytes / HBM_BYTES_PER_S * 1e3, 4)}
            print(f"{name} {B}x{SECONDS}s", file=sys.stderr, flush=True)
            rec = WhisperRecognizer(cfg, None, gen, max_batch=B, state_dict=sd).to(dev)
            row["workspace_bytes"] = rec.workspace_bytes()
            g = torch.Generator().manual_seed(B)
            wavs = [(0.3 * torch.randn(16000 * SECONDS, generator=g)).to(dev) for _ in range(B)]
            fn = lambda: rec.recognize(wavs, sr=16000, prompt_ids=prompt, max_new_tokens=NEW_TOKENS)  # noqa: E731
            with torch.no_grad():
                row["hip_first_call_ms"] = round(timed(fn), 3)
                hyp = fn()
                row["hip_ms"] = round(min(timed(fn) for _ in range(args.reps)), 3)
            t = rec.timings()
            row.update({k: round(t[k], 3) for k in ("logmel_ms", "encoder_ms", "loop_ms")})
            row["steps"] = int(t["steps"])
            row["loop_step_ms"] = round(t["loop_ms"] / max(t["steps"], 1), 4)
            row["loop_step_over_floor"] = round(row["loop_step_ms"] / row["step_floor_ms"], 2)
            assert all(len(h.tokens) == NEW_TOKENS for h in hyp)
            if hf is not None:
                try:
                    mel = mel_filters(cfg.num_mel_bins)
                    feats = torch.stack([R.logmel(w.cpu(), cfg.max_source_positions, mel, torch.float32).T for w in wavs]).to(dev)
                    ids = torch.tensor([prompt] * B, device=dev)
                    hfn = lambda: tf.generation.GenerationMixin.generate(hf, feats, decoder_input_ids=ids, do_sample=False,  # noqa: E731
                                                                         max_new_tokens=NEW_TOKENS, suppress_tokens=[cfg.eos_token_id],
                                                                         eos_token_id=cfg.eos_token_id, pad_token_id=cfg.eos_token_id)
                    with torch.no_grad():
                        row["transformers_first_call_ms"] = round(timed(hfn), 3)
                        theirs = hfn()
                        row["transformers_ms"] = round(min(timed(hfn) for _ in range(args.reps)), 3)
                    row["transformers_over_hip"] = round(row["transformers_ms"] / row["hip_ms"], 3)
                    row["same_tokens_share"] = sum(h.tokens == theirs[i, len(prompt):].tolist() for i, h in enumerate(hyp)) / B
                    del feats
                except RuntimeError as e:
                    row["transformers"] = "not measured: " + str(e).splitlines()[0][:200]
            out["points"].append(row)
            rec.close()
            del wavs
            torch.cuda.empty_cache()
            with open(args.out, "w") as fh:  # kept up to date point by point: a run that is cut short leaves what it measured
                json.dump(out, fh, indent=1)
                fh.write("\n")
        del hf
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
