"""Writes tests/golden/codec/ from `transformers.EncodecModel` (run where transformers is installed; the tests never need it).

    python tools/gen_codec_golden.py

narrow.npz  geometry hidden 16 / 4 filters / codebook 64 x 16: the weights (w:<key>, weight norm removed, fp32), and for
            T in 1, 2, 6, 7, 40 the codes (codes_T) and EncodecModel.decode's fp64 waveform (wav_T).
full.npz    the 24 kHz geometry: weight seed, codes_T and wav_T only; the weights are rebuilt from the seed by
            tests/encodec_ref.make_weights (7.4 M decoder weights are too large to commit).
The model runs in fp64 on the weights loaded through its own parametrised (weight-norm) names."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import encodec_ref as R  # noqa: E402

LENGTHS = (1, 2, 6, 7, 40)
SEEDS = {"narrow": 11, "full": 3}


def model_for(geo, sd):
    from transformers import EncodecConfig, EncodecModel

    cfg = EncodecConfig(hidden_size=geo.hidden, num_filters=geo.filters, codebook_dim=geo.hidden, codebook_size=geo.codebook_size)
    m = EncodecModel(cfg).double().eval()
    msd = m.state_dict()
    for k, v in sd.items():  # g = |v| in fp64: the model's folded weight is the committed fp32 tensor to 1 ulp of fp64
        if k.endswith(".conv.weight"):
            base = k[: -len("weight")] + "parametrizations.weight.original"
            assert msd[base + "1"].shape == v.shape, k
            msd[base + "1"] = v.double()
            msd[base + "0"] = v.double().flatten(1).norm(dim=1).reshape(-1, 1, 1)
        else:
            assert msd[k].shape == v.shape, k
            msd[k] = v.double()
    m.load_state_dict(msd)
    return m


def main():
    out = os.path.join(ROOT, "tests", "golden", "codec")
    os.makedirs(out, exist_ok=True)
    for name, geo in (("narrow", R.NARROW), ("full", R.FULL)):
        sd = R.make_weights(geo, SEEDS[name])
        m = model_for(geo, sd)
        z = {"weight_seed": np.int64(SEEDS[name])}
        if name == "narrow":
            z.update({"w:" + k: v.numpy() for k, v in sd.items()})
        for T in LENGTHS:
            codes = R.make_codes(geo, geo.n_codebooks, T, 5)
            with torch.no_grad():
                wav = m.decode(codes[None, None], [None])[0]
            assert wav.shape == (1, 1, geo.hop * T)
            z[f"codes_{T}"] = codes.numpy()
            z[f"wav_{T}"] = wav.numpy()
        np.savez_compressed(os.path.join(out, name + ".npz"), **z)
        print(name, os.path.getsize(os.path.join(out, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
