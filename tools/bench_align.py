"""Alignment timings (vx_align) at the BASELINE configs[1] geometry (d 1024 / 16 heads / 12 layers, S 47, P 225, 753 aligned
frames) and at configs[4] (S 94, 1505 frames), bf16, with every layer tapped and with one layer tapped, next to the AR scoring pass
of the same utterance (out[10] of vx_get_timings: the same row pass with a final norm, predict layer and nll instead of the taps
and the path).  Device times are HIP events on the engine's stream; each figure is the median of 20 calls after 3 warm-ups.

    python tools/bench_align.py [--out profiles/align_times.json]

--batch N[,N...]: the batched call instead (vx_align_batch, every layer tapped, paths included): n copies of each of the two
utterances through align_batch, next to ``align`` called n times in a loop (the sum of its n device times) and to the AR scoring
pass of the same batch (score_batch, out[10]).  Writes profiles/align_batch_times.json.

    python tools/bench_align.py --batch 1,8,32 [--out profiles/align_batch_times.json]
"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge
ge.build()
from valle_amd.config import ModelConfig
from valle_amd.models import VALLE
from valle_amd.weights import synthetic_inputs, synthetic_state_dict

L, H, P = 12, 16, 225
cfg = ModelConfig(decoder_dim=1024, nhead=H, num_decoder_layers=L)
sd = synthetic_state_dict(cfg, 0)
m = VALLE(1024, H, L, precision="bf16", max_text=128, max_audio=1792, print_eos=False)
m.load_state_dict(sd); m.to("cuda:0").eval()
e = m.engine()
med = statistics.median
out = {"geometry": "d1024 h16 L12 bf16, P 225, synthetic weights", "protocol": "median of 20 after 3 warm-ups, HIP events on the engine stream"}
one = torch.zeros(L, H)
one[L // 2] = 1.0 / H  # one layer tapped: the middle one


def timed(fn, read, n=20, warm=3):
    dev, wall = [], []
    for i in range(n + warm):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        if i >= warm:
            dev.append(read()); wall.append((t1 - t0) * 1e3)
    return {"device_median": med(dev), "device_min": min(dev), "device_max": max(dev), "host_wall_median": med(wall)}


CASES = (("cfg1_S47_T753", 47, 753), ("cfg4_S94_T1505", 94, 1505))
if "--batch" in sys.argv:
    for name, S, T in CASES:
        x, xl, y = synthetic_inputs(S, P + T, seed=1)
        text, codes = x[0].cuda(), y[0].contiguous().cuda()
        out[name] = {"S": S, "T": T}
        for n in [int(v) for v in sys.argv[sys.argv.index("--batch") + 1].split(",")]:
            texts, cs, Ps = [text] * n, [codes] * n, [P] * n
            loop_ms = []

            def loop():
                loop_ms.append(0.0)
                for _ in range(n):
                    e.align(text, codes, P)
                    loop_ms[-1] += e.align_ms()

            r = {"align_loop_ms": timed(loop, lambda: loop_ms[-1]),
                 "score_batch_ar_ms": timed(lambda: e.score_batch(texts, texts, cs, Ps, nar=False), lambda: e.score_timings()["score_ar_ms"]),
                 "align_batch_ms": timed(lambda: e.align_batch(texts, cs, Ps), e.align_ms)}
            r["loop_to_align_batch_ratio"] = r["align_loop_ms"]["device_median"] / r["align_batch_ms"]["device_median"]
            r["align_batch_to_score_batch_ar_ratio"] = r["align_batch_ms"]["device_median"] / r["score_batch_ar_ms"]["device_median"]
            out[name][f"n{n}"] = r
            print(json.dumps({name: {f"n{n}": r}}), flush=True)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "align_batch_times.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    sys.exit(0)
for name, S, T in CASES:
    x, xl, y = synthetic_inputs(S, P + T, seed=1)
    text, codes = x[0].cuda(), y[0].contiguous().cuda()
    r = {"S": S, "T": T}
    r["score_ar_ms"] = timed(lambda: e.score(text, text, codes, P, nar=False), lambda: e.score_timings()["score_ar_ms"])
    r["align_all_layers_ms"] = timed(lambda: e.align(text, codes, P), e.align_ms)
    r["align_one_layer_ms"] = timed(lambda: e.align(text, codes, P, head_w=one), e.align_ms)
    r["align_all_layers_no_path_ms"] = timed(lambda: e.align(text, codes, P, path=False), e.align_ms)
    r["align_to_score_ar_ratio"] = r["align_all_layers_ms"]["device_median"] / r["score_ar_ms"]["device_median"]
    r["align_one_layer_to_score_ar_ratio"] = r["align_one_layer_ms"]["device_median"] / r["score_ar_ms"]["device_median"]
    out[name] = r
    print(json.dumps({name: r}), flush=True)
path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "align_times.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
