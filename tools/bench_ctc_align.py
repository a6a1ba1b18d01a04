"""CTC forced alignment and text likelihood time for (B, seconds) = (1, 3), (1, 10), (32, 10) and (64, 20): 50 frames a second less
one (the recogniser's count), about 15 characters a second, vocabulary 32, logits 4 x randn on the device.  One JSON line on
stdout, the same object written to --out.

    python tools/bench_ctc_align.py [--reps 3] [--points 1x3,1x10,32x10,64x20] [--no-share]

Per point:
  hip_align_ms       vx_falign with every output (the likelihood, the best path, the spans and the scores), device outputs
  hip_nll_ms         vx_falign with nll_out alone (the sum without the max)
  torch_ctc_loss_ms  the comparator for the likelihood: log_softmax + F.ctc_loss(reduction="none") on the GPU, fp32, a padded batch
  torch_viterbi_ms   the comparator for the path: the same recurrence, one frame per step, then the backtrace, one frame per step,
                     on stock torch GPU ops in fp64, batched over the utterances
  recognize_ms / align_ms / align_share   `SpeechRecognizer.recognize` against `.align` (the same pass plus vx_falign_asr and the
                     host's spans) at the base configuration with seeded weights: the share of a recognize call that align adds
Each is warmed, then timed with device events around `inner` back-to-back calls (chosen so that a rep lasts about 50 ms or more); the
figure is the best of the reps.  Both hip entries wait for the stream before they return; the torch figures end on the device.  No
speed is required of the feature: the figures are reported as measured, behind included."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

V, BLANK, CHARS_PER_SECOND = 32, 0, 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", default="1x3,1x10,32x10,64x20", help="BxSECONDS,...")
    ap.add_argument("--no-share", action="store_true", help="skip the recogniser's share")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_align_times.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F

    import __graft_entry__ as ge

    ge.build()
    import asr_cases as AC
    from valle_amd import engine as e
    from valle_amd.asr import RecognizerConfig, SpeechRecognizer, _FalignOut, synthetic_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("bench_ctc_align.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    lib = e.load_library()
    points = [tuple(int(v) for v in p.split("x")) for p in args.points.split(",")]

    def timed(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner  # ms

    def best(fn, reps):
        with torch.no_grad():
            timed(fn, 1)
            inner = max(1, min(200, int(50.0 / max(timed(fn, 1), 1e-3))))
            return round(min(timed(fn, inner) for _ in range(reps)), 4), inner

    def viterbi(x, z, skip):
        """x (B, T, V) fp32, z (B, S) extended ids, skip (B, S) bool -> the states (B, T) of the best paths that end in S - 1."""
        B, T, _ = x.shape
        S = z.shape[1]
        neg = torch.full((B, 2), float("-inf"), dtype=torch.float64, device=x.device)
        r = torch.gather(x.double(), 2, z[:, None, :].expand(B, T, S))
        v = torch.full((B, S), float("-inf"), dtype=torch.float64, device=x.device)
        v[:, :2] = r[:, 0, :2]
        moves = []
        for t in range(1, T):
            p = torch.cat([neg, v], 1)
            cand = torch.stack([v, p[:, 1:S + 1], torch.where(skip, p[:, :S], neg[:, :1])], 0)
            m, mv = cand.max(0)
            v = m + r[:, t]
            moves.append(mv)
        s = torch.full((B, 1), S - 1, dtype=torch.long, device=x.device)
        states = [s]
        for mv in reversed(moves):
            s = s - torch.gather(mv, 1, s)
            states.append(s)
        return torch.cat(states[::-1], 1)

    out = {"bench": "ctc_align", "reps": args.reps, "vocab": V, "chars_per_second": CHARS_PER_SECOND, "timer": "device events, best of reps",
           "points": []}
    g = np.random.default_rng(0)
    for B, sec in points:
        T, L = 50 * sec - 1, CHARS_PER_SECOND * sec
        row = {"B": B, "seconds": sec, "frames": T, "targets": L}
        print(f"{B}x{sec}s", file=sys.stderr, flush=True)
        x = (4.0 * torch.randn(B * T, V, generator=torch.Generator().manual_seed(B * 100 + sec))).to(dev)
        ys = [[int(t) for t in g.integers(1, V, L)] for _ in range(B)]
        frames = (C.c_int32 * B)(*([T] * B))
        flat = (C.c_int32 * (B * L))(*[t for y in ys for t in y])
        lens = (C.c_int32 * B)(*([L] * B))
        full, only = _FalignOut(B, B * T, B * L, dev, True), _FalignOut(B, B * T, B * L, dev, False)
        stream = e.current_stream_ptr(dev)

        def hip(o):
            e._check(lib.vx_falign(x.data_ptr(), V, BLANK, B, frames, flat, lens, *o.pointers(), stream))

        row["hip_align_ms"], row["hip_align_inner"] = best(lambda: hip(full), args.reps)
        row["hip_nll_ms"], row["hip_nll_inner"] = best(lambda: hip(only), args.reps)
        tgt = torch.tensor(ys, dtype=torch.long, device=dev)
        tl, il = torch.full((B,), L, dtype=torch.long, device=dev), torch.full((B,), T, dtype=torch.long, device=dev)
        xb = x.reshape(B, T, V)

        def ctc_loss():
            return F.ctc_loss(F.log_softmax(xb, 2).transpose(0, 1), tgt, il, tl, blank=BLANK, reduction="none")

        row["torch_ctc_loss_ms"], row["torch_ctc_loss_inner"] = best(ctc_loss, args.reps)
        with torch.no_grad():
            ours, theirs = full.nll[:-1], ctc_loss().double()
        row["nll_hip_vs_torch_fp32_max_rel_diff"] = float(((ours - theirs).abs() / theirs.abs()).max())
        z = torch.full((B, 2 * L + 1), BLANK, dtype=torch.long, device=dev)
        z[:, 1::2] = tgt
        skip = torch.zeros_like(z, dtype=torch.bool)
        skip[:, 2:] = (z[:, 2:] != BLANK) & (z[:, 2:] != z[:, :-2])
        row["torch_viterbi_ms"], row["torch_viterbi_inner"] = best(lambda: viterbi(xb, z, skip), args.reps)
        row["torch_ctc_loss_over_hip_nll"] = round(row["torch_ctc_loss_ms"] / row["hip_nll_ms"], 3)
        row["torch_viterbi_over_hip_align"] = round(row["torch_viterbi_ms"] / row["hip_align_ms"], 3)
        if not args.no_share:
            cfg = RecognizerConfig()
            vocab = {t: i for i, t in enumerate(AC.VOCAB32)}
            rec = SpeechRecognizer(cfg, vocab, max_batch=B, max_seconds=sec, state_dict=synthetic_state_dict(cfg, 0)).to(dev)
            gw = torch.Generator().manual_seed(B * 100 + sec)
            wavs = [(0.3 * torch.randn(16000 * sec, generator=gw)).to(dev) for _ in range(B)]
            letters = AC.VOCAB32[5:]
            texts = ["".join(" " if k % 6 == 5 else letters[int(i)] for k, i in enumerate(g.integers(0, len(letters), L))) for _ in range(B)]
            row["recognize_ms"], row["recognize_inner"] = best(lambda: rec.recognize(wavs, sr=16000), args.reps)
            row["align_ms"], row["align_inner"] = best(lambda: rec.align(wavs, texts, sr=16000), args.reps)
            row["align_share"] = round((row["align_ms"] - row["recognize_ms"]) / row["recognize_ms"], 4)
            row["workspace_bytes"] = rec.workspace_bytes()
            rec.close()
            del wavs
        out["points"].append(row)
        del x, full, only
        torch.cuda.empty_cache()
        with open(args.out, "w") as f:  # kept up to date point by point: a run that is cut short leaves what it measured
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
