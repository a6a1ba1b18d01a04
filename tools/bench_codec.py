"""EnCodec decode time at (B, T) = (1, 753), (32, 753), (64, 1505): the HIP decoder against the same computation on stock torch ops
on the GPU (fp32) and on the host threads, one JSON line on stdout.

    python tools/bench_codec.py [--reps 9] [--points 1x753,32x753,64x1505] [--skip-host]
    python tools/bench_codec.py --only-hip --points 1x753 --reps 20      # the run to put under a kernel tracer

Each point is warmed once per implementation, then the implementations alternate rep by rep; the figure is the median of the
wall times, each ending in a device synchronise.  Implementations: `hip` (the decoder as shipped: LSTM steps launched one by one),
`hip_graph` (the same decoder with the steps replayed as the captured chain), `torch_gpu` (stock conv1d / conv_transpose1d / nn.LSTM, one
utterance after the other), `torch_gpu_batched` (the same ops on the whole (B, C, L) batch in one call: every utterance of a
point has the same length, so padding rules are per row as they should be), `torch_host` (16 threads, two utterances scaled to
B).  The yardsticks are tests/encodec_ref's formula with nn.LSTM in place of its Python loop.

    python tools/bench_codec.py --encode [--points 1x225,32x225,64x225]   # prompt waveform -> codes, T frames = 320 T samples

`--encode` times `encode_batch` (device waveforms in, device codes out) against tests/encodec_enc_ref's formula on stock torch ops
(strided conv1d, nn.LSTM, the quantiser's distance matrix by matmul and argmax) per utterance, in one batched call, and on the host.

    python tools/bench_codec.py --resample [--reps 21]

`--resample` times the prompt's way to 24 kHz mono (`Resampler(48000, 24000)`): one 3 s stereo 48 kHz prompt, and 32 prompts of
1.5 .. 4.6 s with one or two channels in one ragged call, against tests/resample_ref's polyphase form on stock torch GPU ops (channel
mean, pad, conv1d with stride, per utterance), and next to `encode_batch` of the resampled prompts, the step it precedes."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_decoder(sd, geo, device):
    """Stock-op decoder on `device` in fp32: conv1d / conv_transpose1d / nn.LSTM, one utterance per call."""
    import torch
    import torch.nn.functional as F

    import encodec_ref as R

    P = {k: v.to(device) for k, v in R.fold_weight_norm(sd, torch.float32).items()}
    lstm = torch.nn.LSTM(geo.width, geo.width, geo.lstm_layers).to(device)
    for n, p in lstm.named_parameters():
        p.data.copy_(P["decoder.layers.1.lstm." + n])
    up, res, last = R.layer_index(geo)

    def conv(x, w, b):  # (B, C, L): left reflect pad, zero-extended when L <= pad
        pad = w.shape[-1] - 1
        if pad == 0:
            return F.conv1d(x, w, b)
        extra = max(0, pad - x.shape[-1] + 1)
        xp = F.pad(F.pad(x, (0, extra)), (pad, 0), mode="reflect")
        return F.conv1d(xp[..., : xp.shape[-1] - extra], w, b)

    def up_conv(x, w, b, r):
        y = F.conv_transpose1d(x, w, b, stride=r)
        return y[..., : y.shape[-1] - (w.shape[-1] - r)]

    @torch.no_grad()
    def run(codes):
        """codes (n_q, T) or (B, n_q, T) -> (B, 1, hop T)"""
        codes = codes.to(device)
        if codes.dim() == 2:
            codes = codes[None]
        x = sum(P[f"quantizer.layers.{q}.codebook.embed"][codes[:, q]] for q in range(codes.shape[1])).transpose(1, 2)
        x = conv(x, P["decoder.layers.0.conv.weight"], P["decoder.layers.0.conv.bias"])
        x = lstm(x.permute(2, 0, 1))[0].permute(1, 2, 0) + x
        for i, r in enumerate(geo.ratios):
            x = up_conv(F.elu(x), P[f"decoder.layers.{up[i]}.conv.weight"], P[f"decoder.layers.{up[i]}.conv.bias"], r)
            p = f"decoder.layers.{res[i]}."
            h = conv(F.elu(x), P[p + "block.1.conv.weight"], P[p + "block.1.conv.bias"])
            h = conv(F.elu(h), P[p + "block.3.conv.weight"], P[p + "block.3.conv.bias"])
            x = conv(x, P[p + "shortcut.conv.weight"], P[p + "shortcut.conv.bias"]) + h
        return conv(F.elu(x), P[f"decoder.layers.{last}.conv.weight"], P[f"decoder.layers.{last}.conv.bias"])

    return run


def torch_encoder(sd, geo, device):
    """Stock-op encoder on `device` in fp32, (B, 1, L) -> (B, n_q, T); L a multiple of the hop here (no right pad)."""
    import torch
    import torch.nn.functional as F

    import encodec_enc_ref as E
    import encodec_ref as R

    P = {k: v.to(device) for k, v in R.fold_weight_norm(sd, torch.float32).items()}
    res, down, li, last = E.enc_layer_index(geo)
    lstm = torch.nn.LSTM(geo.width, geo.width, geo.lstm_layers).to(device)
    for n, p in lstm.named_parameters():
        p.data.copy_(P[f"encoder.layers.{li}.lstm." + n])
    cbs = [P[f"quantizer.layers.{q}.codebook.embed"] for q in range(geo.n_codebooks)]
    sq = [c.pow(2).sum(1)[None] for c in cbs]

    def conv(x, w, b, stride=1):
        k = w.shape[-1]
        left = k - stride
        extra = -(-x.shape[-1] // stride) * stride - x.shape[-1]
        if left or extra:
            ext = max(0, max(left, extra) - x.shape[-1] + 1)
            xp = F.pad(F.pad(x, (0, ext)), (left, extra), mode="reflect")
            x = xp[..., : xp.shape[-1] - ext]
        return F.conv1d(x, w, b, stride=stride)

    @torch.no_grad()
    def run(wav):
        x = conv(wav.to(device), P["encoder.layers.0.conv.weight"], P["encoder.layers.0.conv.bias"])
        for i, r in enumerate(E.enc_ratios(geo)):
            p = f"encoder.layers.{res[i]}."
            h = conv(F.elu(x), P[p + "block.1.conv.weight"], P[p + "block.1.conv.bias"])
            h = conv(F.elu(h), P[p + "block.3.conv.weight"], P[p + "block.3.conv.bias"])
            x = conv(x, P[p + "shortcut.conv.weight"], P[p + "shortcut.conv.bias"]) + h
            x = conv(F.elu(x), P[f"encoder.layers.{down[i]}.conv.weight"], P[f"encoder.layers.{down[i]}.conv.bias"], r)
        x = lstm(x.permute(2, 0, 1))[0].permute(1, 2, 0) + x
        x = conv(F.elu(x), P[f"encoder.layers.{last}.conv.weight"], P[f"encoder.layers.{last}.conv.bias"])
        B, D, T = x.shape
        r = x.transpose(1, 2).reshape(B * T, D)
        out = []
        for cb, s2 in zip(cbs, sq):
            idx = (-(r.pow(2).sum(1, keepdim=True) - 2 * r @ cb.T + s2)).max(dim=1).indices
            out.append(idx)
            r = r - cb[idx]
        return torch.stack(out).reshape(len(cbs), B, T).transpose(0, 1)

    return run


def main_encode(args):
    import torch

    import __graft_entry__ as ge

    ge.build()
    import encodec_enc_ref as E
    from valle_amd.codec import EncodecDecoder

    if not torch.cuda.is_available():
        raise SystemExit("bench_codec.py measures on the GPU; none found")
    torch.set_num_threads(16)
    points = [tuple(int(v) for v in p.split("x")) for p in args.points.split(",")]
    sd = E.make_enc_weights(E.FULL, 3)
    enc = EncodecDecoder(max_frames=max(t for _, t in points), max_batch=max(b for b, _ in points), encoder=True)
    enc.load_state_dict(sd)
    enc.to("cuda:0")
    gpu_ref = torch_encoder(sd, E.FULL, "cuda:0")
    host_ref = torch_encoder(sd, E.FULL, "cpu")
    sync = torch.cuda.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return time.perf_counter() - t0

    out = {"bench": "codec_encode", "reps": args.reps, "host_threads": torch.get_num_threads(), "points": []}
    for B, T in points:
        host_wavs = [E.make_wave(320 * T, 200 + b) for b in range(B)]
        wavs = [w.to("cuda:0") for w in host_wavs]
        stacked = torch.cat(wavs)
        impls = {"hip": lambda: enc.encode_batch(wavs)}
        row = {"B": B, "T": T, "samples": 320 * T}
        if not args.only_hip:
            impls["torch_gpu"] = lambda: [gpu_ref(w) for w in wavs]
            impls["torch_gpu_batched"] = lambda: gpu_ref(stacked)
            if not args.skip_host:
                impls["torch_host"] = lambda: [host_ref(w) for w in host_wavs[:min(B, 2)]]
            ours = torch.cat(enc.encode_batch(wavs))
            row["hip_vs_torch_gpu_code_agreement"] = float((ours == gpu_ref(stacked)).double().mean())
        for fn in impls.values():
            timed(fn)
        times = {k: [] for k in impls}
        for _ in range(args.reps):
            for k, fn in impls.items():
                times[k].append(timed(fn))
        for k, v in times.items():
            scale = B / min(B, 2) if k == "torch_host" else 1.0
            row[k + "_ms"] = round(1e3 * statistics.median(v) * scale, 3)
            row[k + "_min_ms"] = round(1e3 * min(v) * scale, 3)
        out["points"].append(row)
    print(json.dumps(out))


def main_resample(args):
    import torch
    import torch.nn.functional as F

    import __graft_entry__ as ge

    ge.build()
    import encodec_enc_ref as E
    import resample_ref as RR
    from valle_amd.codec import EncodecDecoder, Resampler

    if not torch.cuda.is_available():
        raise SystemExit("bench_codec.py measures on the GPU; none found")
    orig, new = 48000, 24000
    rs = Resampler(orig, new, max_batch=32).to("cuda:0")
    enc = EncodecDecoder(max_frames=768, max_batch=32, encoder=True)
    enc.load_state_dict(E.make_enc_weights(E.FULL, 3))
    enc.to("cuda:0")
    k64, W = RR.polyphase_kernel(orig, new)
    kern = k64.float()[:, None, :].to("cuda:0")
    o, n, _ = RR.ratio(orig, new)

    @torch.no_grad()
    def torch_one(w):
        y = F.conv1d(F.pad(w.mean(0)[None, None], (W, W + o)), kern, stride=o)
        return y[0].T.reshape(-1)[:RR.out_length(orig, new, w.shape[1])]

    sync = torch.cuda.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return time.perf_counter() - t0

    cases = {"1 prompt, 3 s stereo": [RR.make_noise(3 * orig, 1, channels=2) * 0.1],
             "32 prompts, 1.5 .. 4.6 s, 1 or 2 channels": [RR.make_noise(orig * 3 // 2 + 4801 * b, 10 + b, channels=1 + b % 2) * 0.1
                                                           for b in range(32)]}
    out = {"bench": "codec_resample", "orig_hz": orig, "new_hz": new, "reps": args.reps, "points": []}
    for name, host_wavs in cases.items():
        wavs = [w.to("cuda:0") for w in host_wavs]
        mono = rs.resample_batch(wavs)
        ref = [torch_one(w) for w in wavs]
        row = {"case": name, "B": len(wavs), "input_samples": sum(w.shape[1] for w in wavs),
               "hip_vs_torch_gpu_max_abs_diff": max(float((a[0, 0] - b).abs().max()) for a, b in zip(mono, ref))}
        impls = {"hip": lambda: rs.resample_batch(wavs), "torch_gpu": lambda: [torch_one(w) for w in wavs],
                 "hip_encode_after": lambda: enc.encode_batch(mono)}
        for fn in impls.values():
            timed(fn)
            timed(fn)
        times = {k: [] for k in impls}
        for _ in range(args.reps):
            for k, fn in impls.items():
                times[k].append(timed(fn))
        for k, v in times.items():
            row[k + "_ms"] = round(1e3 * statistics.median(v), 3)
            row[k + "_min_ms"] = round(1e3 * min(v), 3)
        out["points"].append(row)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--points", default=None, help="BxT,...; default 1x753,32x753,64x1505, with --encode 1x225,32x225,64x225")
    ap.add_argument("--encode", action="store_true", help="time the encoder (waveform -> codes) instead of the decoder")
    ap.add_argument("--resample", action="store_true", help="time the resampler in front of the encoder (48 kHz stereo -> 24 kHz mono)")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--only-hip", action="store_true", help="time the HIP decoder alone (for a kernel trace)")
    args = ap.parse_args()
    if args.resample:
        return main_resample(args)
    if args.points is None:
        args.points = "1x225,32x225,64x225" if args.encode else "1x753,32x753,64x1505"
    if args.encode:
        return main_encode(args)
    import torch

    import __graft_entry__ as ge

    ge.build()
    import encodec_ref as R
    from valle_amd.codec import EncodecDecoder

    if not torch.cuda.is_available():
        raise SystemExit("bench_codec.py measures on the GPU; none found")
    torch.set_num_threads(16)
    points = [tuple(int(v) for v in p.split("x")) for p in args.points.split(",")]
    sd = R.make_weights(R.FULL, 3)
    cap = dict(max_frames=max(t for _, t in points), max_batch=max(b for b, _ in points))
    dec = EncodecDecoder(**cap)
    dec.load_state_dict(sd)
    dec.to("cuda:0")
    if not args.only_hip:
        plain = EncodecDecoder(lstm_graph=True, **cap)
        plain.load_state_dict(sd)
        plain.to("cuda:0")
        gpu_ref = torch_decoder(sd, R.FULL, "cuda:0")
        host_ref = torch_decoder(sd, R.FULL, "cpu")
    sync = torch.cuda.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return time.perf_counter() - t0

    out = {"bench": "codec_decode", "reps": args.reps, "host_threads": torch.get_num_threads(), "points": []}
    for B, T in points:
        codes = [R.make_codes(R.FULL, 8, T, 100 + b) for b in range(B)]
        impls = {"hip": lambda: dec.decode_batch(codes)}
        row = {"B": B, "T": T}
        if not args.only_hip:
            stacked = torch.stack(codes).to("cuda:0")
            impls["hip_graph"] = lambda: plain.decode_batch(codes)
            impls["torch_gpu"] = lambda: [gpu_ref(c) for c in codes]
            impls["torch_gpu_batched"] = lambda: gpu_ref(stacked)
            if not args.skip_host:
                impls["torch_host"] = lambda: [host_ref(c) for c in codes[:min(B, 2)]]  # per utterance; scaled to B below
            ours = torch.cat(dec.decode_batch(codes))  # every utterance of the batch (all groups) against stock torch
            ref = gpu_ref(stacked)
            row["hip_vs_torch_gpu_rel_diff"] = float((ours - ref).abs().max() / ref.abs().max())
            row["hip_equals_hip_graph"] = bool(torch.equal(ours, torch.cat(plain.decode_batch(codes))))
        for fn in impls.values():
            timed(fn)
        times = {k: [] for k in impls}
        for _ in range(args.reps):
            for k, fn in impls.items():
                times[k].append(timed(fn))
        for k, v in times.items():
            scale = B / min(B, 2) if k == "torch_host" else 1.0
            row[k + "_ms"] = round(1e3 * statistics.median(v) * scale, 3)
            row[k + "_min_ms"] = round(1e3 * min(v) * scale, 3)
        out["points"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
