"""CPU: the fp64 restatement of alignment (align_ref.py) is what the reference's attention module returns, its path search is
the optimum (brute force), and the host side of VALLE.align (spans, head weights, argument checks) is right.  What needs an engine
runs in test_gpu_align.py."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import align_ref as ar
import score_ref as sr


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


def test_align_symbols_exist_and_refuse_null_without_gpu(lib):
    from valle_amd import engine

    for name in ("vx_align", "vx_op_attn_text_rows", "vx_op_mono_path"):
        assert hasattr(lib, name) and name in engine.declared_symbols()
    assert lib.vx_align(None, None, 0, None, 0, 0, 0, 0, None, None, None, None, None, None, None) == 1
    assert b"null" in lib.vx_last_error()
    assert lib.vx_op_mono_path(None, 4, 4, None, None, None) == 1 and b"null" in lib.vx_last_error()
    assert lib.vx_op_mono_path(8, 4, 5000, 8, 8, None) == 4 and b"4096" in lib.vx_last_error()  # refused before any HIP call
    a = [0, 8, 64, 8, 64, 64, 4, 0, 1, 64, 7, 1, 2, 9, 8, 8, None, None, 1, None]  # window [2, 9) of 7 text tokens
    assert lib.vx_op_attn_text_rows(*a) == 1 and b"window" in lib.vx_last_error()


def _small(model_name="VALL-E", norm_first=True, bos=False):
    from valle_amd.config import ModelConfig
    from valle_amd.weights import synthetic_inputs, synthetic_state_dict

    cfg = ModelConfig(model_name=model_name, decoder_dim=64, nhead=4, num_decoder_layers=2, norm_first=norm_first, prepend_bos=bos,
                      num_quantizers=2)
    sd = synthetic_state_dict(cfg, 0)
    x, _, y = synthetic_inputs(6, 11, 2, seed=3)
    return cfg, sr.oracle(cfg, sd), x[0], y[0]


@pytest.mark.parametrize("norm_first", [True, False])
def test_text_attention_is_what_torch_multi_head_attention_returns(norm_first):
    """Layer 0, head mean, against F.multi_head_attention_forward(need_weights=True, average_attn_weights=True) - the call the
    reference's module makes (modules/activation.py:205-251) - on the same input and mask, in fp64."""
    from oracle import valle_oracle as vo

    cfg, m, text, codes = _small(norm_first=norm_first)
    P, S, A, d = 3, text.shape[0], codes.shape[0], m.d
    probs, smax = ar.text_attention(m, text, codes, P)
    assert probs.shape == (2, 4, A - P, S) and smax.shape == (2, 4, A - P) and probs.dtype == torch.float64
    x = torch.cat([m.ar_text(text), m.ar_audio(codes[:, 0])], 0)
    L = m.ar_layers[0]
    inp = (L.norm(0, x, None) if norm_first else x).unsqueeze(1)  # (N, 1, d)
    mask = vo.ar_mask(S, A)
    _, w = F.multi_head_attention_forward(inp, inp, inp, d, m.nhead, L.in_w, L.in_b, None, None, False, 0.0, L.out_w, L.out_b,
                                          training=False, need_weights=True, attn_mask=mask, average_attn_weights=True)
    want = w[0, S + P - 1 : S + A - 1, :S]  # the rows that predict frames P .. A-1
    assert float((probs[0].mean(0) - want).abs().max()) <= 1e-12
    assert bool((probs.sum(-1) < 1.0).all()) and bool((probs >= 0).all())  # the rest of each row's mass is on the audio keys


def test_text_attention_vallf_is_the_cross_attention():
    cfg, m, text, codes = _small(model_name="VALL-F", bos=True)
    P, S, A, d = 0, text.shape[0], codes.shape[0], m.d
    probs, _ = ar.text_attention(m, text, codes, P)
    assert probs.shape == (2, 4, A, S)
    assert float((probs.sum(-1) - 1.0).abs().max()) <= 1e-12  # every key of the cross-attention is a text token
    # layer 0 against torch's module call on the oracle's own query input and memory
    L = m.ar_layers[0]
    yy = F.pad(codes[:, 0], (1, 0), value=sr.EOS + 1)
    x, mem = m.ar_audio(yy), m.ar_text(text)
    n = yy.shape[0]
    tgt_mask = torch.triu(torch.ones(n, n, dtype=torch.bool), diagonal=1)
    from oracle import valle_oracle as vo

    x1 = x + vo.self_attention(L.norm(0, x, None), L.in_w, L.in_b, L.out_w, L.out_b, m.nhead, tgt_mask)[0]
    qin = L.norm(1, x1, None).unsqueeze(1)
    _, w = F.multi_head_attention_forward(qin, mem.unsqueeze(1), mem.unsqueeze(1), d, m.nhead, L.cin_w, L.cin_b, None, None, False, 0.0,
                                          L.cout_w, L.cout_b, training=False, need_weights=True, average_attn_weights=True)
    assert float((probs[0].mean(0) - w[0, :A]).abs().max()) <= 1e-12


def _brute(a):
    T, Sw = a.shape
    best, best_p = -np.inf, None
    la = np.log(np.maximum(a.astype(np.float64), ar.FLT_MIN))
    for steps in itertools.product((0, 1), repeat=T - 1):
        if sum(steps) != Sw - 1:
            continue
        p = np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)
        s = la[np.arange(T), p].sum()
        if s > best:
            best, best_p = s, p
    return best_p, best


def test_mono_path_is_the_brute_force_optimum():
    rng = np.random.default_rng(0)
    for T in range(1, 9):
        for Sw in range(1, 5):
            a = rng.random((T, Sw)).astype(np.float32)
            a[rng.random((T, Sw)) < 0.15] = 0.0  # zeros are clamped at FLT_MIN, not -inf
            path, score = ar.mono_path(a)
            if T < Sw:
                assert path is None and score == float("-inf")
                continue
            bp, bs = _brute(a)
            assert ar.valid_path(path, T, Sw)
            assert score == pytest.approx(bs, rel=1e-12) and ar.path_score(a, path) == pytest.approx(bs, rel=1e-12)


def test_mono_path_tie_rule_and_diagonal():
    path, _ = ar.mono_path(np.full((7, 3), 0.25, dtype=np.float32))
    assert path.tolist() == [0, 1, 2, 2, 2, 2, 2]  # equal predecessors: stay, so every advance happens as early as it can
    path, score = ar.mono_path(np.random.default_rng(1).random((4, 4)))
    assert path.tolist() == [0, 1, 2, 3] and np.isfinite(score)
    assert ar.mono_path(np.ones((3, 4))) == (None, float("-inf"))


def test_spans_from_a_hand_made_path():
    from valle_amd.models import make_alignment, path_spans

    path = torch.tensor([0, 0, 0, 1, 2, 2, 3], dtype=torch.int32)
    assert path_spans(path, 4).tolist() == [[0, 3], [3, 4], [4, 6], [6, 7]]
    attn = torch.zeros(7, 4)
    attn[torch.arange(7), path.long()] = 0.5
    al = make_alignment(attn, torch.ones(7), path, torch.tensor([-4.85]))
    assert al.spans.dtype == torch.int32 and al.spans.tolist() == [[0, 3], [3, 4], [4, 6], [6, 7]]
    assert torch.allclose(al.seconds, al.spans.float() / 75.0) and al.seconds[3, 1].item() == pytest.approx(7 / 75.0)
    assert al.token_mass.tolist() == [1.5, 0.5, 1.0, 0.5] and al.path_score == pytest.approx(-4.85)
    none = make_alignment(attn[:3], torch.ones(3), torch.full((3,), -1, dtype=torch.int32), torch.tensor([float("-inf")]))
    assert none.path is None and none.spans is None and none.seconds is None and none.path_score == float("-inf")


def test_head_weights():
    from valle_amd.models import head_weights

    assert head_weights(None, 2, 4) is None
    w = head_weights([(1, 2), (0, 0)], 2, 4)
    assert w.dtype == torch.float32 and w.tolist() == [[0.5, 0, 0, 0], [0, 0, 0.5, 0]]
    w = head_weights(torch.tensor([[1.0, 3.0], [0.0, 4.0]]), 2, 2)
    assert w.tolist() == [[0.125, 0.375], [0.0, 0.5]]
    for bad in ([], [(2, 0)], [(0, 4)], [(0, 1), (0, 1)], [(0,)], torch.zeros(2, 4), torch.ones(2, 3), -torch.ones(2, 4),
                torch.full((2, 4), float("nan"))):
        with pytest.raises(ValueError):
            head_weights(bad, 2, 4)


def test_align_argument_checks_before_any_engine():
    """A bad `heads`, a window outside the text and prompt_frames=0 without BOS raise ValueError on a model that has no device
    (an engine could not even be created: that would be the RuntimeError of the last case)."""
    from valle_amd.models import VALLE

    m = VALLE(128, 2, 2).eval()
    x, x_lens = torch.randint(3, 50, (1, 6)), torch.tensor([6])
    y = torch.randint(0, 1024, (1, 10, 8))
    with pytest.raises(ValueError, match="head"):
        m.align(x, x_lens, y, 3, heads=[(0, 2)])
    with pytest.raises(ValueError, match="heads"):
        m.align(x, x_lens, y, 3, heads=torch.zeros(2, 2))
    with pytest.raises(ValueError, match="window"):
        m.align(x, x_lens, y, 3, enroll_x_lens=torch.tensor([6]))
    with pytest.raises(ValueError, match="prepend_bos"):
        m.align(x, x_lens, y, 0)
    with pytest.raises(ValueError, match="prompt_frames"):
        m.align(x, x_lens, y, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.align(x, x_lens, y, 3)
