"""GPU: the geometry of the XCD-sharded attention launch (ar_tp.hpp tp_attn_kernel): 8 key splits per head among a head's 16
workgroups, and an out-projection slice cut per head (64 rows x 64 channels per workgroup).

(1) Each pass's logits of the sharded step against the five-launch step (VX_AR_TP=0 engine in the same process) on one
    d = 1024 / 16-head / 2-layer model (layer 0 = the FIRST instantiation, layer 1 the other; the head is launch 4 of the
    three-accumulator rotation), synthetic weights with the q rows sharpened as in test_gpu_ar_step.py so that single keys
    matter, teacher-forced tokens.  Tolerances are those of test_gpu_engine.py: fp32 2e-5 of a row's largest logit + 1e-6 and
    equal argmax where the margin exceeds 4e-5 (its sharded-versus-plain test); bf16 3 % of a row's largest logit and equal
    argmax where the margin exceeds twice that (its bf16 rule: both steps round the newest K / V rows to bf16 on their own).
    Cached-row counts n (= the newest row's index; keys 0..n-1 are split [j ceil(n/8), ...), the newest key goes to split 7):
      2..9        splits without a key, with exactly one, the first split with two (n = 9).  n = 0 and 1 cannot be reached
                  through the C ABI: a prefill holds at least one text and one audio row and computes pass 0 itself, so the
                  first decode pass has n >= 2;
      127..129    with bos;
      1023..1033  the last slot of the preloaded pass in bf16 (8 x 128 rows), the first key of a second pass (n = 1025);
      2048..2050  three passes in bf16 (n >= 2049), five and more in fp32.
    Measured on the MI355X: worst error 2.6e-7 of a row's largest logit in fp32 and 2.5e-7 in bf16 (no newest-row element
    rounded the other way in these passes).
    A decode whose hand-overs time out fails with VX_ERR_STATE (the error word): every decode here must return normally, and
    the step graph must hold 2 L + 2 kernels (sharded) / 5 L + 2 (five-launch) - tp_setup falls back silently.
(2) The out-projection's re-laid-out copy read back ("tp_wo") against the index formula of tp_repack_kernel for a matrix of
    distinct values (fp32: value = 1024 row + column; bf16: two loads, the row and then the column as the bit pattern)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

L = 2
Q_SHARPEN = 4.0
# (prepend_bos, prompt rows P, forced tokens): text S = 1, so the first decode pass has n = 1 + bos + P cached rows
RUNS = [(True, 0, 8), (True, 125, 3), (False, 1022, 11), (False, 2047, 3)]
MAX_AUDIO = 2047 + 8


def _engine(monkeypatch, precision, bos, tp, sd=None):
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.config import ModelConfig
    from valle_amd.engine import Engine
    from valle_amd.weights import synthetic_state_dict

    if tp:
        monkeypatch.delenv("VX_AR_TP", raising=False)
    else:
        monkeypatch.setenv("VX_AR_TP", "0")
    cfg = ModelConfig(decoder_dim=1024, nhead=16, num_decoder_layers=L, prefix_mode=1, prepend_bos=bos, num_quantizers=1)
    if sd is None:
        sd = synthetic_state_dict(cfg, 5)
        for li in range(L):
            sd[f"ar_decoder.layers.{li}.self_attn.in_proj_weight"][:1024] *= Q_SHARPEN
    e = Engine(cfg, precision, max_text=16, max_audio=MAX_AUDIO + 8, trace_logits=True)
    e.load_state_dict(sd)
    return e, sd


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_sharded_step_matches_plain_step_at_split_boundaries(monkeypatch, precision):
    fails = []
    for bos in (True, False):
        logits = {}
        sd = None
        for tp in (True, False):
            e, sd = _engine(monkeypatch, precision, bos, tp, sd)
            try:
                for run, (b, P, n) in enumerate(RUNS):
                    if b != bos:
                        continue
                    g = torch.Generator().manual_seed(100 + run)
                    text = torch.randint(3, 100, (1,), generator=g)
                    prompt = torch.randint(0, 1024, (P,), generator=g)
                    forced = torch.randint(0, 1024, (n,), generator=g)
                    e.ar_prefill(text, prompt)
                    e.ar_decode(top_k=1, forced=forced)  # raises if the error word of the hand-overs is set
                    toks, _, n_pass = e.ar_result()
                    assert torch.equal(toks, forced) and n_pass == n + 1
                    want = 2 * L + 2 if tp else 5 * L + 2
                    assert e.timings()["step_kernels"] == want, (tp, e.timings()["step_kernels"])
                    logits[(tp, run)] = e.read("ar_logits", (n_pass, 1025)).clone()
            finally:
                e.close()
        for run, (b, P, n) in enumerate(RUNS):
            if b != bos:
                continue
            a, ref = logits[(True, run)], logits[(False, run)]
            scale = ref.abs().amax(1)
            err = (a - ref).abs().amax(1)
            if precision == "fp32":
                tol, margin = 2e-5 * scale + 1e-6, 4e-5 * scale
            else:
                tol = 0.03 * scale
                margin = 2 * tol
            n0 = 1 + int(b) + P  # cached rows of decode pass 1 (pass 0 is the prefill's)
            print(f"\n{precision} bos={b} n={n0}..{n0 + n - 1}: worst err / scale {float((err / scale).max()):.3g}")
            top2 = ref.topk(2, dim=1)[0]
            decided = (top2[:, 0] - top2[:, 1]) > margin
            for p in range(n + 1):
                if float(err[p]) > float(tol[p]):
                    fails.append(f"bos={b} n={n0 + p - 1} (pass {p}): err {float(err[p]):.4g} > {float(tol[p]):.4g}")
                if bool(decided[p]) and int(a[p].argmax()) != int(ref[p].argmax()):
                    fails.append(f"bos={b} n={n0 + p - 1} (pass {p}): argmax differs")
    assert not fails, "; ".join(fails[:20])


def _expected_words(vec):
    """Source (row, first column) of every 16-byte word of the re-laid-out out-projection, in destination order:
    word [(32 x + i) * OCH + m][t], i = 16 hl + j, = rows 64 j + t / 4, columns 64 (2 x + hl) + (t % 4 + 4 m) * VEC."""
    och = 16 // vec
    w = torch.arange(1024 * 1024 // vec)
    t, blk = w % 256, w // 256
    m, wg = blk % och, blk // och
    x, i = wg // 32, wg % 32
    row = 64 * (i % 16) + t // 4
    col = 64 * (2 * x + i // 16) + (t % 4 + 4 * m) * vec
    return row, col


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_out_projection_repack_layout(monkeypatch, precision):
    key = "ar_decoder.layers.0.self_attn.out_proj.weight"
    r = torch.arange(1024).view(1024, 1).expand(1024, 1024)
    c = torch.arange(1024).view(1, 1024).expand(1024, 1024)
    e, sd = _engine(monkeypatch, precision, True, True)
    try:
        if precision == "fp32":
            vec = 4
            row, col = _expected_words(vec)
            sd[key] = (1024 * r + c).float()
            e.load_state_dict(sd)
            got = e.read("tp_wo", (1024 * 1024 // vec, vec)).long()
            want = (1024 * row + col).view(-1, 1) + torch.arange(vec).view(1, vec)
            assert torch.equal(got, want)
        else:
            vec = 8
            row, col = _expected_words(vec)
            for code, want in ((r, row.view(-1, 1).expand(-1, vec)), (c, col.view(-1, 1) + torch.arange(vec).view(1, vec))):
                # the value whose bf16 bit pattern is 0x4000 + code: finite, exact in bf16
                sd[key] = ((0x4000 + code).to(torch.int32) << 16).contiguous().view(torch.float32)
                e.load_state_dict(sd)
                got = e.read("tp_wo", (1024 * 1024 // vec, vec), dtype=torch.int16).long() - 0x4000
                assert torch.equal(got, want)
    finally:
        e.close()
