"""GPU: the seven small handles (vx_fbank, vx_resampler, vx_dtw, vx_pitch, vx_stft, vx_vocoder, vx_gan) under VX_POISON.

VX_POISON=1 fills every fresh device allocation with 0xFF bytes (NaN as fp32, -1 as integers) before its owner initialises it -
for these handles inside DevBuf::alloc and CallStage::init (csrc/host.hpp).  Tables, staged arrays and workspaces must all be
written before they are read: the same bits with and without the poison, and nothing non-finite.  The shapes are the smallest
that touch every staged column (two utterances of unequal length, every optional pointer column given), ragged tile offsets and
the regrowth of the DTW workspace.  The Griffin-Lim workspace grows in steps of 1024 frames, so next to the 40-frame call only
the 1030-frame one replaces it."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SCRIPT = (
    "import sys, json, hashlib, math, os, torch; sys.path[:0] = [%r, os.path.join(%r, 'tests')]\n"
    "import __graft_entry__ as ge; ge.build()\n"
    "import ganvoc_ref as GR\n"
    "from valle_amd.codec import Resampler\n"
    "from valle_amd.dtw import DTW\n"
    "from valle_amd.fbank import BigVGANFbank\n"
    "from valle_amd.ganvoc import GanVocoder\n"
    "from valle_amd.pitch import PitchTracker\n"
    "from valle_amd.stft import MultiResolutionSTFT, STFTConfig\n"
    "from valle_amd.vocoder import GriffinLim\n"
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
    "tone = lambda L: (torch.sin(2 * math.pi * 200 / 24000 * torch.arange(L)) + 0.01 * rnd(L)).cuda()\n"
    "pt = PitchTracker(max_frames=64, max_batch=2).to('cuda:0')\n"
    "tr = pt.track_batch([tone(600), tone(2000)])\n"
    "outs['pitch'] = [t for r in tr for t in (r.f0, r.aperiodicity, r.lag, r.voiced)]\n"
    "diag = torch.arange(min(tr[0].f0.numel(), tr[1].f0.numel()), dtype=torch.int32).repeat(2, 1).t().contiguous().cuda()\n"
    "outs['pitch_cmp'] = [pt.compare_sums([(tr[0].f0, tr[1].f0, diag)])]\n"
    "st = MultiResolutionSTFT(STFTConfig(resolutions=((512, 128, 512), (1024, 256, 1024)), max_samples=4096), max_batch=2).to('cuda:0')\n"
    "outs['stft'] = [st.compare_sums([rnd(1500).cuda(), rnd(3000).cuda()], [rnd(1300).cuda(), rnd(3000).cuda()])]\n"
    "outs['stft_mag'] = st.magnitude_batch([rnd(1500).cuda(), rnd(3000).cuda()], res=1)\n"
    "gl = GriffinLim(max_batch=2, max_total_frames=2048).to('cuda:0')\n"
    "for name, Ts in (('gl', (3, 9)), ('gl_40', (40,)), ('gl_grown', (1030,))):\n"
    "    wavs, phases = gl.synthesize_batch([GR.logmel(T).cuda() for T in Ts], n_iter=2, rand_init=True, return_phase=True)\n"
    "    outs[name] = wavs + phases\n"
    "cfg = GR.GEOMETRIES['g1_snakebeta']\n"
    "gan = GanVocoder(cfg, state_dict=GR.make_weights(cfg, 1), max_batch=2, max_total_frames=50).to('cuda:0')\n"
    "outs['gan'] = gan.synthesize_batch([GR.logmel(3).cuda(), GR.logmel(7).cuda()])\n"
    "torch.cuda.synchronize()\n"
    "digest = lambda ts: hashlib.sha256(b''.join(t.cpu().contiguous().numpy().tobytes() for t in ts)).hexdigest()\n"
    "finite = all(bool(torch.isfinite(t).all()) for ts in outs.values() for t in ts)\n"
    "sizes = {k: [list(t.shape) for t in ts] for k, ts in outs.items()}\n"
    "print(json.dumps({'hash': {k: digest(ts) for k, ts in outs.items()}, 'finite': finite, 'sizes': sizes}))\n" % (ROOT, ROOT))


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
        z = o["sizes"]
        assert z["pitch"] == [[2]] * 4 + [[8]] * 4 and z["pitch_cmp"] == [[1, 11]]
        assert z["stft"] == [[2, 2, 4]] and z["stft_mag"] == [[6, 513], [12, 513]]
        assert z["gl"] == [[768], [2304], [3, 513, 2], [9, 513, 2]] and z["gl_40"] == [[10240], [40, 513, 2]]
        assert z["gl_grown"] == [[263680], [1030, 513, 2]] and z["gan"] == [[12], [28]]
    assert outs[0]["hash"] == outs[1]["hash"]
