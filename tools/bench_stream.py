"""Continuous vs static batching at BASELINE configs[2] geometry (d=1024 nhead=16 L=12, 32 slots, bf16), one JSON line on stdout.

    python tools/bench_stream.py [--n 128] [--slots 32] [--poll 4,8,16,32] [--refill 1,2,4,8]
    python tools/bench_stream.py --kv-cache bf16,fp8 [--slots 64 --text-len 94] [--reps 2]
    python tools/bench_stream.py --ab-half-done [--lib path/to/libvallex.so]
    python tools/bench_stream.py --model-name VALL-F [...]
    python tools/bench_stream.py --step-times [--model-name VALL-F,VALL-E] [--reps 3]
    python tools/bench_stream.py --vallf-rows [--reps 2] [--nar-only]

Default mode: a seeded queue of --n utterances, S uniform in [10, 94], P = 225 (synthetic weights: every utterance stops by the
length rule, T = 16 S + 1 frames), decoded end to end (AR + 7 NAR stages) once through inference_batch, group by group, and once
per (poll_steps, refill_at) setting through inference_stream.  Reported per run: codec-tokens/s (frames of all utterances over the
wall time of the whole queue), slot occupancy (live slot-steps / launched slot-steps) and the mean / p95 latency of an utterance
from queue start to its codes, the device time per batched step (step_us) and the bytes of the model's slot KV caches.

--kv-cache: the slot-cache formats to run (comma-separated: bf16, fp8).  With both, each format gets its own model on the same
queue and the runs alternate between them rep by rep (static, then stream, per format).

--ab-half-done: device time per batched step with all 32 slots live, and with half of them done (teacher-forced lengths 753 and
1), through vx_batch_decode, so that the same measurement runs on a library without the continuous-batching entry points.

--model-name: VALL-E (default) or VALL-F (the cross-attention variant; its slots are prefilled and admitted one by one and its NAR
stages run per utterance).  --step-times: for each of the comma-separated model names, in one process, the device time per
batched step with all slots live (S = 47, P = 225, 753 teacher-forced tokens, vx_batch_decode) and of the batch-1 step on the same
utterance (vx_ar_decode; not with --skip-batch1), --reps times each after a warm-up.

--vallf-rows: one VALL-F model built with batched_rows=True (VX_FLAG_VALLF_ROWS), two A/Bs alternating in one process: the NAR
stages of --slots utterances (S = 47, P = 225, T = 753) as one vx_nar_batch pass against the loop of vx_nar over the same
utterances (device ms of the passes), and the --n utterance queue through inference_stream with batched_admit / batched_nar on
against the same queue with both off (the path of a model without the option).  Also written to profiles/vallf_rows_times.json.
--nar-only: the NAR A/B alone, one repetition (e.g. under a kernel trace)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model(args, max_audio, kv_cache="bf16", name=None, **opts):
    if args.lib:  # a library built from another revision: bind only the entry points it exports (the static batched path)
        import ctypes as C

        import valle_amd  # noqa: F401
        from valle_amd import engine

        probe = C.CDLL(os.path.abspath(args.lib))
        engine._SIGS = {k: v for k, v in engine._SIGS.items() if hasattr(probe, k)}
        engine.load_library(os.path.abspath(args.lib))
    else:
        import __graft_entry__ as ge

        ge.build()
    from valle_amd.config import ModelConfig
    from valle_amd.models import VALLE, VALLF
    from valle_amd.weights import synthetic_state_dict

    name = name or args.model_name
    cls = VALLF if name.lower() in ("vall-f", "vallf") else VALLE
    cfg = ModelConfig(model_name=cls.MODEL_NAME, decoder_dim=1024, nhead=16, num_decoder_layers=12, prefix_mode=1)
    m = cls(1024, 16, 12, prefix_mode=1, precision=args.precision, max_text=128, max_audio=max_audio, print_eos=False,
            max_batch=args.slots, **({"kv_cache": kv_cache} if kv_cache != "bf16" else {}), **opts)
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    return m.to("cuda:0").eval()


def queue(n, seed, text_len=None):
    import torch
    from valle_amd.weights import synthetic_inputs

    g = torch.Generator().manual_seed(seed)
    S = [text_len] * n if text_len else torch.randint(10, 95, (n,), generator=g).tolist()
    return [synthetic_inputs(s, 225, 8, seed=1000 + i) for i, s in enumerate(S)], S


def count_steps(eng):
    """Counts the batched steps the engine launches (vx_batch_decode / vx_batch_run) and their device ms, from its timings."""
    box = [0, 0.0]
    for name in ("batch_decode", "batch_run"):
        orig = getattr(eng, name)

        def wrap(*a, _orig=orig, **k):
            r = _orig(*a, **k)
            t = eng.timings()
            box[0] += t["batch_launches"]
            box[1] += t["batch_decode_ms"]
            return r

        setattr(eng, name, wrap)
    return box


def summary(kind, t0, done_at, frames, steps, slots, **extra):
    import numpy as np

    wall = max(done_at.values()) - t0
    lat = np.array([done_at[i] - t0 for i in sorted(done_at)])
    return dict(kind=kind, tok_per_s=round(sum(frames) / wall, 1), wall_s=round(wall, 3),
                occupancy=round(sum(frames) / (steps * slots), 4), steps=int(steps),
                latency_mean_s=round(float(lat.mean()), 3), latency_p95_s=round(float(np.percentile(lat, 95)), 3), **extra)


def slot_cache_bytes(eng):
    """bytes of an engine's slot KV caches: max_batch x L x (K, V) x heads x (max_text + max_audio) rows x 64 channels, 2 bytes a
    value in bf16, 1 byte + 1/16 scale byte in fp8"""
    c = eng.cfg
    vals = eng.max_batch * c.num_decoder_layers * 2 * c.decoder_dim * (eng.max_text + eng.max_audio)
    return vals * 2 if eng.kv_cache == "bf16" else vals + vals // 16


def run_queue(args):
    import torch

    kvs = args.kv_cache.split(",")
    utts, S = queue(args.n, args.seed, args.text_len)
    frames = [16 * s + 1 for s in S]
    seeds = list(range(1, args.n + 1))
    B = args.slots
    polls = [int(v) for v in args.poll.split(",")]
    refills = [int(v) for v in args.refill.split(",")]
    models = {}
    for kv in kvs:
        m = model(args, 1792, kv)
        eng = m.engine()
        models[kv] = (m, count_steps(eng), slot_cache_bytes(eng))
        # warm-up: every shape class the timed runs use (graph capture, row buffers, NAR at the group's row count)
        w, _ = queue(B, args.seed + 1, args.text_len)
        m.inference_batch(w, top_k=10, seeds=list(range(B)))
        for _ in m.inference_stream(w, top_k=10, seeds=list(range(B))):
            pass
        torch.cuda.synchronize()
    runs = []

    def extra(kv):
        steps = models[kv][1]
        return dict(kv_cache=kv, slot_cache_bytes=models[kv][2], step_us=round(1e3 * steps[1] / max(steps[0], 1), 2))

    def static(kv):
        m, steps, _ = models[kv]
        steps[0], steps[1] = 0, 0.0
        done_at = {}
        t0 = time.perf_counter()
        for g0 in range(0, args.n, B):  # inference_batch's own grouping, timed group by group
            out = m.inference_batch(utts[g0 : g0 + B], top_k=10, seeds=seeds[g0 : g0 + B])
            torch.cuda.synchronize()
            now = time.perf_counter()
            for i in range(len(out)):
                done_at[g0 + i] = now
        return summary("static", t0, done_at, frames, steps[0], B, **extra(kv))

    def stream(kv, poll, refill):
        m, steps, _ = models[kv]
        steps[0], steps[1] = 0, 0.0
        done_at = {}
        t0 = time.perf_counter()
        for i, codes in m.inference_stream(utts, top_k=10, seeds=seeds, poll_steps=poll, refill_at=refill):
            done_at[i] = time.perf_counter()  # codes are on the device, written by work already synchronised by the engine
        return summary("stream", t0, done_at, frames, steps[0], B, poll_steps=poll, refill_at=refill, **extra(kv))

    for rep in range(args.reps):
        for kv in kvs:  # the formats alternate rep by rep on the same queue
            runs.append(static(kv))
            for p in polls:
                runs.append(stream(kv, p, refills[0]))
            for r in refills[1:]:
                runs.append(stream(kv, polls[0], r))
    # codes of the two paths: identical AR tokens (same seeds, per-slot arithmetic) - checked once on the timed queue, per format
    same = {}
    for kv in kvs:
        m = models[kv][0]
        ref = m.inference_batch(utts[:B], top_k=10, seeds=seeds[:B], batched_prefill=False)
        got = dict(m.inference_stream(utts[:B], top_k=10, seeds=seeds[:B], batched_admit=False))
        same[kv] = all(torch.equal(ref[i][0, :, 0], got[i][0, :, 0]) for i in range(len(ref)))
    return dict(mode="queue", model=args.model_name, geometry=f"d=1024 nhead=16 L=12 {args.precision}", slots=B, n=args.n,
                S_range=[args.text_len] * 2 if args.text_len else [10, 94], P=225, frames=sum(frames),
                ar_codes_equal_static=same if len(kvs) > 1 else same[kvs[0]], runs=runs)


def run_ab(args):
    import torch

    kv = args.kv_cache.split(",")[0]
    m = model(args, 1024, kv)
    eng = m.engine()
    B = args.slots
    from valle_amd.weights import synthetic_inputs

    utts = [synthetic_inputs(47, 225, 8, seed=2000 + i) for i in range(B)]
    texts = [u[0][0] for u in utts]
    proms = [u[2][0, :, 0].contiguous() for u in utts]
    g = torch.Generator().manual_seed(3)
    full = [torch.randint(0, 1024, (753,), generator=g).cuda() for _ in range(B)]
    out = {}
    for name, forced in (("all_live", full), ("half_done", [f if b % 2 == 0 else f[:1] for b, f in enumerate(full)])):
        vals = []
        for rep in range(args.reps + 1):
            eng.batch_prefill_all(texts, proms)
            eng.batch_decode(B, top_k=10, forced=forced)
            t = eng.timings()
            if rep:  # the first is warm-up
                vals.append(1e3 * t["batch_decode_ms"] / t["batch_launches"])
        out[name] = dict(step_us=[round(v, 2) for v in vals], mean_us=round(sum(vals) / len(vals), 2))
    return dict(mode="ab_half_done", lib=args.lib or "libvallex.so", kv_cache=kv, slots=B, S=47, P=225, T=753, **out)


def run_step_times(args):
    import torch
    from valle_amd.weights import synthetic_inputs

    B = args.slots
    utts = [synthetic_inputs(47, 225, 8, seed=2000 + i) for i in range(B)]
    g = torch.Generator().manual_seed(3)
    full = [torch.randint(0, 1024, (753,), generator=g) for _ in range(B)]
    res = dict(mode="step_times", slots=B, S=47, P=225, T=753, models={})
    for name in args.model_name.split(","):
        m = model(args, 1024, "bf16", name)
        eng = m.engine()
        slot_us, b1_us = [], []
        for rep in range(args.reps + 1):  # the first is warm-up (graph capture)
            for b, u in enumerate(utts):
                eng.batch_prefill(b, u[0][0], u[2][0, :, 0].contiguous())
            eng.batch_decode(B, top_k=10, forced=[f.cuda() for f in full])
            t = eng.timings()
            if rep:
                slot_us.append(1e3 * t["batch_decode_ms"] / t["batch_launches"])
            if args.skip_batch1:
                continue
            eng.ar_prefill(utts[0][0][0], utts[0][2][0, :, 0].contiguous())
            eng.ar_decode(top_k=10, forced=full[0])
            t = eng.timings()
            if rep:
                b1_us.append(1e3 * t["decode_ms"] / t["launches"])
        s_mean = sum(slot_us) / len(slot_us)
        if args.skip_batch1:
            res["models"][name] = dict(slot_step_us=[round(v, 2) for v in slot_us], slot_step_mean_us=round(s_mean, 2))
            continue
        b_mean = sum(b1_us) / len(b1_us)
        res["models"][name] = dict(slot_step_us=[round(v, 2) for v in slot_us], slot_step_mean_us=round(s_mean, 2),
                                   batch1_step_us=[round(v, 2) for v in b1_us], batch1_step_mean_us=round(b_mean, 2),
                                   slot_tok_per_s=round(B * 1e6 / s_mean, 1), batch1_tok_per_s=round(1e6 / b_mean, 1),
                                   slot_vs_batch1_tok_per_s=round(B * b_mean / s_mean, 2))
        del m, eng
        torch.cuda.synchronize()
    return res


def run_vallf_rows(args):
    import torch
    from valle_amd.weights import synthetic_inputs

    B = args.slots
    m = model(args, 1792, "bf16", "VALL-F", batched_rows=True)
    eng = m.engine()
    res = dict(mode="vallf_rows", geometry=f"d=1024 nhead=16 L=12 {args.precision}", slots=B)
    # the NAR stages of B utterances: one batched pass against the per-utterance loop, device ms (vx_get_timings)
    S, P, T = 47, 225, 753
    utts = [synthetic_inputs(S, P, 8, seed=2000 + i) for i in range(B)]
    g = torch.Generator().manual_seed(3)
    texts = [u[0][0] for u in utts]
    proms = [u[2][0].contiguous() for u in utts]
    toks = [torch.randint(0, 1024, (T,), generator=g) for _ in range(B)]
    batched_ms, loop_ms = [], []
    for rep in range((1 if args.nar_only else args.reps) + 1):  # the first is warm-up (row buffers grow to the batch's rows)
        eng.nar_batch(texts, proms, toks, out_device="cuda")
        b = eng.timings()["nar_ms"]
        one = 0.0
        for i in range(B):
            eng.nar(texts[i], proms[i], toks[i], out_device="cuda")
            one += eng.timings()["nar_ms"]
        if rep:
            batched_ms.append(b)
            loop_ms.append(one)
    mean = lambda v: sum(v) / len(v)
    res["nar"] = dict(utterances=B, S=S, P=P, T=T, batched_ms=[round(v, 3) for v in batched_ms], per_utterance_loop_ms=[round(v, 3) for v in loop_ms],
                      batched_mean_ms=round(mean(batched_ms), 3), loop_mean_ms=round(mean(loop_ms), 3),
                      loop_over_batched=round(mean(loop_ms) / mean(batched_ms), 2))
    if not args.nar_only:
        queue_utts, Sq = queue(args.n, args.seed, args.text_len)
        frames = [16 * s + 1 for s in Sq]
        seeds = list(range(1, args.n + 1))
        poll, refill = int(args.poll.split(",")[0]), int(args.refill.split(",")[0])
        steps = count_steps(eng)
        w, _ = queue(B, args.seed + 1, args.text_len)
        for on in (True, False):  # warm-up of both paths
            for _ in m.inference_stream(w, top_k=10, seeds=list(range(B)), batched_admit=on, batched_nar=on):
                pass
        torch.cuda.synchronize()
        runs = []
        for rep in range(args.reps):
            for on in (True, False):  # alternating on the same queue
                steps[0], steps[1] = 0, 0.0
                done_at = {}
                t0 = time.perf_counter()
                for i, codes in m.inference_stream(queue_utts, top_k=10, seeds=seeds, poll_steps=poll, refill_at=refill, batched_admit=on,
                                                   batched_nar=on):
                    done_at[i] = time.perf_counter()
                runs.append(summary("stream", t0, done_at, frames, steps[0], B, batched_rows=on, poll_steps=poll, refill_at=refill,
                                    step_us=round(1e3 * steps[1] / max(steps[0], 1), 2)))
        tps = lambda on: mean([r["tok_per_s"] for r in runs if r["batched_rows"] == on])
        res["queue"] = dict(n=args.n, S_range=[args.text_len] * 2 if args.text_len else [10, 94], P=225, frames=sum(frames), runs=runs,
                            tok_per_s_batched=round(tps(True), 1), tok_per_s_per_utterance=round(tps(False), 1),
                            batched_over_per_utterance=round(tps(True) / tps(False), 2))
        with open(os.path.join(ROOT, "profiles", "vallf_rows_times.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--poll", default="8", help="comma-separated poll_steps values (the first is used for the refill sweep)")
    ap.add_argument("--refill", default="4", help="comma-separated refill_at values (the first is used for the poll sweep)")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--ab-half-done", action="store_true")
    ap.add_argument("--lib", default=None, help="--ab-half-done: load this libvallex.so instead of the package's")
    ap.add_argument("--kv-cache", default="bf16", help="slot-cache formats, comma-separated: bf16, fp8 (both: an A/B on one queue)")
    ap.add_argument("--precision", default="bf16", help="bf16 | fp8nar")
    ap.add_argument("--text-len", type=int, default=None, help="every utterance S = this (default: S uniform in [10, 94])")
    ap.add_argument("--model-name", default="VALL-E", help="VALL-E | VALL-F (--step-times: comma-separated)")
    ap.add_argument("--step-times", action="store_true")
    ap.add_argument("--skip-batch1", action="store_true", help="--step-times: the batched step only (e.g. under a kernel trace)")
    ap.add_argument("--vallf-rows", action="store_true", help="VALL-F with batched_rows=True: batched NAR / admission against per utterance")
    ap.add_argument("--nar-only", action="store_true", help="--vallf-rows: the NAR A/B alone, one repetition")
    args = ap.parse_args()
    if not args.kv_cache or any(kv not in ("bf16", "fp8") for kv in args.kv_cache.split(",")):
        ap.error("--kv-cache: comma-separated bf16 / fp8")
    res = run_vallf_rows(args) if args.vallf_rows else run_ab(args) if args.ab_half_done else run_step_times(args) if args.step_times else run_queue(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
