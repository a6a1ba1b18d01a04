"""GPU: the three small handles (vx_fbank, vx_resampler, vx_dtw) under VX_POISON.

VX_POISON=1 fills every fresh device allocation with 0xFF bytes (NaN as fp32, -1 as integers) before its owner initialises it -
for these handles inside DevBuf::alloc and CallStage::init (csrc/host.hpp).  Tables, staged arrays and workspaces must all be
written before they are read: the same bits with and without the poison, and nothing non-finite.  The shapes are the smallest
that touch every staged array, ragged tile offsets and the regrowth of the DTW workspace."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SCRIPT = (
    "import sys, json, hashlib, torch; sys.path.insert(0, %r)\n"
    "import __graft_entry__ as ge; ge.build()\n"
    "from valle_amd.codec import Resampler\n"
    "from valle_amd.dtw import DTW\n"
    "from valle_amd.fbank import BigVGANFbank\n"
    "g = torch.Generator().manual_seed(0)\n"
    "rnd = lambda *s: torch.randn(*s, generator=g)\n"
    "outs = {}\n"
    "outs['fbank'] = BigVGANFbank(max_batch=2).to('cuda:0').extract_batch([rnd(300), rnd(1000)])\n"
    "outs['resample'] = Resampler(16000, 24000, max_batch=2).to('cuda:0').resample_batch([rnd(200), rnd(2, 777)])\n"
    "dtw = DTW(dim=8, n_ceps=3, max_frames=64, max_batch=2).to('cuda:0')\n"
    "pairs = lambda *shapes: [(rnd(ta, 8).cuda(), rnd(tb, 8).cuda()) for ta, tb in shapes]\n"
    "for name, ps in (('dtw', pairs((5, 7), (9, 4))), ('dtw_grown', pairs((40, 33)))):\n"
    "    res = dtw.compare_batch(ps, return_path=True)\n"
    "    outs[name] = [torch.tensor([r.total for r in res], dtype=torch.float64), torch.tensor([r.length for r in res])]\n"
    "    outs[name] += [r.path for r in res]\n"
    "torch.cuda.synchronize()\n"
    "digest = lambda ts: hashlib.sha256(b''.join(t.cpu().contiguous().numpy().tobytes() for t in ts)).hexdigest()\n"
    "finite = all(bool(torch.isfinite(t).all()) for ts in outs.values() for t in ts)\n"
    "sizes = {k: [list(t.shape) for t in ts] for k, ts in outs.items()}\n"
    "print(json.dumps({'hash': {k: digest(ts) for k, ts in outs.items()}, 'finite': finite, 'sizes': sizes}))\n" % ROOT)


def test_small_handles_do_not_depend_on_uninitialised_memory():
    outs = []
    for poison in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", SCRIPT], env=dict(os.environ, VX_POISON=poison), capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for o in outs:
        assert o["finite"] is True
        assert o["sizes"]["fbank"] == [[1, 100], [4, 100]] and o["sizes"]["resample"] == [[1, 1, 300], [1, 1, 1166]]
        assert o["sizes"]["dtw"][:2] == [[2], [2]] and o["sizes"]["dtw_grown"][:2] == [[1], [1]]
    assert outs[0]["hash"] == outs[1]["hash"]
