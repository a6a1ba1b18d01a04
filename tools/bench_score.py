"""Scoring timings at BASELINE configs[1] geometry (d 1024 / 16 heads / 12 layers, S 47, P 225, 753 scored frames, bf16):
vx_score (AR part, NAR part, both), the forced decode + logits read that gives the same AR numbers step by step, and
vx_score_batch at 32 utterances.  Device times are HIP events on the engine's stream (vx_get_timings).

    python tools/bench_score.py [--out profiles/score_times.json]
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

cfg = ModelConfig(decoder_dim=1024, nhead=16, num_decoder_layers=12)
sd = synthetic_state_dict(cfg, 0)
x, xl, y = synthetic_inputs(47, 978, seed=1)
text, codes, P = x[0].cuda(), y[0].contiguous().cuda(), 225
m = VALLE(1024, 16, 12, precision="bf16", max_text=128, max_audio=1792, print_eos=False, trace_logits=True)
m.load_state_dict(sd); m.to("cuda:0").eval()
e = m.engine()
med = statistics.median
out = {"geometry": "d1024 h16 L12 bf16, S 47, P 225, T 753 (A 978), synthetic weights", "protocol": "median of 20 after 3 warm-ups, HIP events on the engine stream"}

def run(ar, nar, n=20, warm=3):
    a, b, w = [], [], []
    for i in range(n + warm):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        e.score(text, text, codes, P, ar=ar, nar=nar)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        t = e.score_timings()
        if i >= warm:
            a.append(t["score_ar_ms"]); b.append(t["score_nar_ms"]); w.append((t1 - t0) * 1e3)
    return a, b, w

a, _, w = run(True, False)
out["score_ar_only_ms"] = {"device_median": med(a), "device_min": min(a), "device_max": max(a), "host_wall_median": med(w)}
_, b, w = run(False, True)
out["score_nar_only_ms"] = {"device_median": med(b), "device_min": min(b), "device_max": max(b), "host_wall_median": med(w)}
a, b, w = run(True, True)
both = [p + q for p, q in zip(a, b)]
out["score_both_ms"] = {"device_median": med(both), "device_min": min(both), "device_max": max(both), "host_wall_median": med(w)}
print(json.dumps(out), flush=True)

# the parent commit's only route to the same AR numbers: a forced decode of the 753 tokens + a read of every logits row
dev, wall = [], []
for i in range(7):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    e.ar_prefill(text, codes[:P, 0].contiguous())
    e.ar_decode(top_k=1, forced=codes[P:, 0].contiguous())
    toks, _, n_pass = e.ar_result()
    lg = e.read("ar_logits", (n_pass, 1025))
    t1 = time.perf_counter()
    if i >= 2:
        t = e.timings(); dev.append(t["prefill_ms"] + t["decode_ms"]); wall.append((t1 - t0) * 1e3)
out["forced_decode_ms"] = {"n_pass": n_pass, "device_prefill_plus_decode_median": med(dev), "host_wall_incl_logits_read_median": med(wall),
                           "protocol": "median of 5 after 2 warm-ups"}
print(json.dumps(out["forced_decode_ms"]), flush=True)

# the two routes give the same numbers
an, ak, _, _ = e.score(text, text, codes, P, nar=False)
tg = torch.cat([codes[P:, 0].cpu(), torch.tensor([1024])])
ref = torch.nn.functional.cross_entropy(lg.double(), tg, reduction="none")
out["row_pass_vs_step_path"] = {"mean_abs_nll_diff": float((an.cpu().double() - ref).abs().mean()), "max_abs_nll_diff": float((an.cpu().double() - ref).abs().max()),
                                "loss_row_pass": float(an.sum()), "loss_step_path": float(ref.sum())}

# 32 utterances in one call
n = 32
a, b = [], []
for i in range(6):
    e.score_batch([text] * n, [text] * n, [codes] * n, [P] * n)
    torch.cuda.synchronize()
    t = e.score_timings()
    if i >= 1:
        a.append(t["score_ar_ms"]); b.append(t["score_nar_ms"])
out["score_batch_32_ms"] = {"ar_device_median": med(a), "nar_device_median": med(b), "both_device_median": med([p + q for p, q in zip(a, b)]),
                            "protocol": "median of 5 after 1 warm-up; 32 copies of the utterance, 32 x 1025 rows per pass"}
path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "score_times.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
