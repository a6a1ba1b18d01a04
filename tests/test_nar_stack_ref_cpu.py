"""CPU: tests/nar_stack_ref.py (the layer-by-layer fp64 NAR forward of test_gpu_nar_stack.py) agrees with the oracle's own
teacher-forced NAR forward (score_ref.nar_score_logits) to fp64 rounding, pre- and post-norm, and each of its named wrong
answers is a different answer."""
import pytest
import torch

from nar_stack_ref import WRONG, NarRef
from score_ref import nar_score_logits


@pytest.mark.parametrize("norm_first", [True, False])
def test_layer_loop_equals_the_oracle_forward(norm_first):
    from valle_amd.config import ModelConfig
    from valle_amd.weights import synthetic_state_dict

    cfg = ModelConfig(decoder_dim=128, nhead=2, num_decoder_layers=2, prefix_mode=1, num_quantizers=3, norm_first=norm_first)
    sd = synthetic_state_dict(cfg, 5)
    g = torch.Generator().manual_seed(5)
    text, codes, P = torch.randint(3, 100, (9,), generator=g), torch.randint(0, 1024, (40, 3), generator=g), 13
    ref = NarRef(cfg, sd, "cpu")
    want = nar_score_logits(ref.m, text, codes, P)
    for stage in range(2):
        r = ref.forward(text, codes, P, stage)
        assert r["logits"].dtype == torch.float64 and r["logits"].shape == (27, 1024)
        assert float((r["logits"] - want[stage]).abs().max()) < 1e-11 * float(want[stage].abs().max())
        assert r["x"].shape == r["x_abs"].shape == (49, 128) and bool((r["x_abs"] > 0).all())
        assert bool((r["head_abs"] >= r["logits"].abs() * (1 - 1e-12)).all())
        for w in WRONG:
            assert float((ref.forward(text, codes, P, stage, w)["logits"] - r["logits"]).abs().max()) > 1e-4, w
