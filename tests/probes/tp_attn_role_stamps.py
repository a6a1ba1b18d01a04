"""The attention launch's stamps told apart BY ROLE (ar_tp.hpp: workgroups j = local index % 16 < 8 of a head run a key split, the
other eight do not): does a workgroup's row arrive later the more bytes its own CU queued at kernel start, and how far does the
split that takes the newest key (j = 7) trail the other seven?

    python vall-e_amd/csrc/build.py --stamps && python tests/probes/tp_attn_role_stamps.py [out.json]

Per role and phase: min / median / max over the role's 128 workgroups of the time since the launch's first stamp, in us, averaged
over layers 1..11 of the last decode step.  Phases: row_arrived (slot 7), ln_done (1), qkv_published (2); for the split role also
head_gathered (3) and partial_published (4), the latter once more for split 7 alone and for splits 0..6; for the other role
partials_gathered (5) and out_stored (6).  Two context lengths, as tp_attn_split_stamps.py.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

import valle_amd  # noqa: F401
from valle_amd.engine import load_probe_library

lib = load_probe_library(stamps=True)
lib.vx_debug_fqstamps.argtypes = [C.c_void_p, C.c_int64]
from valle_amd.config import ModelConfig
from valle_amd.models import VALLE
from valle_amd.weights import synthetic_inputs, synthetic_state_dict

L = 12
cfg = ModelConfig(decoder_dim=1024, nhead=16, num_decoder_layers=L, prefix_mode=1)
m = VALLE(1024, 16, L, prefix_mode=1, precision="bf16", max_text=64, max_audio=1024, print_eos=False)
m.load_state_dict(synthetic_state_dict(cfg, seed=0))
m.to("cuda:0").eval()
x, xl, y = synthetic_inputs(47, 225, 8, seed=1)
x, xl, y = x.cuda(), xl.cuda(), y.cuda()
for i in range(2):
    torch.manual_seed(1234 + i)
    m.inference(x, xl, y, None, top_k=10)
JJ = (np.arange(256) >> 3) & 15  # workgroup b: local index i = b / 8, j = i % 16
SPLIT = JJ < 8
COMMON = (("row_arrived", 7), ("ln_done", 1), ("qkv_published", 2))


def mmm(rel, sel):
    """rel (layers, 256) -> [min, median, max] over the selected workgroups, averaged over the layers"""
    r = rel[:, sel]
    return [round(float(r.min(axis=1).mean()), 2), round(float(np.median(r, axis=1).mean()), 2), round(float(r.max(axis=1).mean()), 2)]


res = {}
for n_new in (100, 700):
    assert lib.vx_debug_fqstamps(None, 0) == 0
    torch.manual_seed(7)
    m.inference(x, xl, y, None, top_k=10, max_new_tokens=n_new)
    t = m.engine().timings()
    buf = np.zeros((2, 16, 256, 16), dtype=np.uint64)
    assert lib.vx_debug_fqstamps(buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0
    st = buf[0, 1:L].astype(np.int64)             # attention half, layers 1..11: (layer, workgroup, slot)
    first = st[:, :, 0].min(axis=1)[:, None]
    rel = lambda ph: (st[:, :, ph] - first) * 0.01
    out = dict(step_us=round(1e3 * t["decode_ms"] / t["launches"], 2))
    out["split"] = {n: mmm(rel(ph), SPLIT) for n, ph in COMMON + (("head_gathered", 3), ("partial_published", 4))}
    out["other"] = {n: mmm(rel(ph), ~SPLIT) for n, ph in COMMON + (("partials_gathered", 5), ("out_stored", 6))}
    out["partial_published_split7"] = mmm(rel(4), JJ == 7)
    out["partial_published_splits0to6"] = mmm(rel(4), JJ < 7)
    out["head_gathered_split7"] = mmm(rel(3), JJ == 7)
    out["head_gathered_splits0to6"] = mmm(rel(3), JJ < 7)
    res[n_new] = out
    print(n_new, json.dumps(out), flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
