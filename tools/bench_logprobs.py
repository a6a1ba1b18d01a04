"""What VX_FLAG_LOGPROBS costs, at the bench geometry (d 1024 / 16 heads / 12 layers, bf16, S 47, P 225, 753 frames): two engines
of the same build and the same weights, one created with the flag and one without, timed in turn (off, on, off, on, ...) so that
whatever else the machine is doing lands on both.  Device times are HIP events on the engine's stream (vx_get_timings).

    batch-1 AR step     ar_decode of 753 tokens (top-k 10), us per pass = decode ms / launches
    32-slot step        batch_decode of 32 utterances, 256 tokens each, us per step = batch decode ms / launches
    batched NAR pass    nar_batch of 32 utterances x 753 frames, all seven stages, ms

    python tools/bench_logprobs.py [--out profiles/logprob_times.json] [--reps 7]
"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge
ge.build()
from valle_amd.config import ModelConfig
from valle_amd.engine import Engine
from valle_amd.weights import synthetic_inputs, synthetic_state_dict

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
S, P, T, B = 47, 225, 753, 32
cfg = ModelConfig(decoder_dim=1024, nhead=16, num_decoder_layers=12)
sd = synthetic_state_dict(cfg, 0)  # EOS row zeroed: no decode ends early
eng = {}
for name, flag in (("off", False), ("on", True)):
    eng[name] = Engine(cfg, "bf16", max_text=64, max_audio=1024, max_batch=B, logprobs=flag)
    eng[name].load_state_dict(sd)
x, _, y = synthetic_inputs(S, P + T, seed=1)
text, prompt = x[0].cuda(), y[0, :P].contiguous().cuda()
texts = [synthetic_inputs(40 + b % 15, P, seed=10 + b)[0][0].cuda() for b in range(B)]  # ragged S in [40, 54], as bench.py --batch 32
gen = y[0, P:, 0].contiguous().cuda()
med = statistics.median


def step_b1(e):
    e.ar_prefill(text, prompt[:, 0].contiguous())
    e.ar_decode(top_k=10, seed=1, max_new_tokens=T)
    toks, _, n_pass = e.ar_result()
    t = e.timings()
    return 1e3 * t["decode_ms"] / t["launches"], t["step_kernels"], toks


def step_b32(e):
    e.batch_prefill_all(texts, [prompt[:, 0].contiguous()] * B)
    e.batch_decode(B, top_k=10, seeds=list(range(1, B + 1)), max_new_tokens=256)
    t = e.timings()
    return 1e3 * t["batch_decode_ms"] / t["batch_launches"], t["batch_launches"], e.batch_result(B - 1)[0]


def nar_b32(e):
    e.nar_batch(texts, [prompt] * B, [gen] * B)
    return e.timings()["nar_ms"], None, None


out = {"geometry": f"d1024 h16 L12 bf16, S {S} (32-slot: ragged 40..54), P {P}, T {T}, synthetic weights",
       "protocol": f"flag off and on alternate in one process, {reps} timed repetitions each after 2 warm-ups; median (min .. max); "
                   "HIP events on the engine stream"}
for key, fn, unit in (("ar_step_batch1", step_b1, "us_per_pass"), ("ar_step_32_slots", step_b32, "us_per_step"),
                      ("nar_batch_32x753", nar_b32, "ms")):
    vals, extra, last = {"off": [], "on": []}, {}, {}
    for i in range(reps + 2):
        for name in ("off", "on"):
            v, k, toks = fn(eng[name])
            extra[name], last[name] = k, toks
            if i >= 2:
                vals[name].append(v)
    r = {name: {"median": med(v), "min": min(v), "max": max(v)} for name, v in vals.items()}
    r["unit"] = unit
    r["on_minus_off_median"] = r["on"]["median"] - r["off"]["median"]
    r["off_spread"] = r["off"]["max"] - r["off"]["min"]
    if key == "ar_step_batch1":
        r["step_kernels"] = extra
    if last["off"] is not None:
        r["same_tokens"] = bool(torch.equal(last["off"], last["on"]))
    out[key] = r
    print(json.dumps({key: r}), flush=True)
path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "logprob_times.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
