"""Writes tests/golden/kv8/<case>.npz: the logits an AR decoder with fp8 slot caches (tests/kv8_ref.py) gives at the probe passes
of the committed fixtures tests/golden/<case>.npz, teacher-forced with those fixtures' codes.  Reads only the repository (the
fixtures regenerate their synthetic weights and inputs from seeds); CPU only.

    python tools/gen_kv8_golden.py [case ...]      default: the four pre-norm, head_dim 64 fixtures the batched decode serves

Each file holds: probe_steps (n,), kv8_logits (n, 1025) fp32, plain_logits (n, 1025) (the fixture's reference logits), and
rel_err (n,) = max |kv8 - plain| / max |plain| per probe row.  The fixtures live in a subdirectory so that the suites iterating
over tests/golden/*.npz do not take them for reference fixtures.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

CASES = ["cfg0_greedy", "cfg0_topk10", "cfg1_topk10", "cfg4_s94_topk10"]
OUT = os.path.join(ROOT, "tests", "golden", "kv8")


def kv8_case(name: str):
    """(probe_steps, kv8_logits, plain_logits, rel_err) of one fixture, computed live."""
    from conftest import Golden
    from kv8_ref import kv8_forced_logits

    g = Golden(name)
    c = g.cfg
    assert c.norm_first and not c.add_prenet and not c.prepend_bos and c.decoder_dim // c.nhead == 64, name
    m = g.oracle()
    forced = g.codes[0, :, 0].contiguous()
    steps = list(g.ar_probe_steps)
    got = kv8_forced_logits(m, g.x[0], g.y[0, :, 0].contiguous(), forced, steps)
    plain = g.ar_probe_logits
    rel = (got - plain).abs().amax(1) / plain.abs().amax(1)
    return np.array(steps, np.int32), got.numpy().astype(np.float32), plain.numpy().astype(np.float32), rel.numpy().astype(np.float32)


def main(names):
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for name in names:
        t0 = time.time()
        steps, got, plain, rel = kv8_case(name)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), probe_steps=steps, kv8_logits=got, plain_logits=plain, rel_err=rel)
        print(f"{name}: probe passes {steps.tolist()} rel err {[round(float(r), 5) for r in rel]} ({time.time() - t0:.0f} s)")


if __name__ == "__main__":
    main(sys.argv[1:] or CASES)
