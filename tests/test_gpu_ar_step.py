"""GPU: the batch-1 AR decode step pass by pass against the fp64 reference of tests/ar_step_ref.py.

Each case builds an engine with synthetic weights (the q rows of every in_proj scaled by Q_SHARPEN so that the softmax is peaked),
prefills it, teacher-forces a run that straddles the attention kernels' register-pass boundaries, and reads the traced logits and
the final KV cache ("ar_kv").  The reference reads the engine's own cache rows, so every checked pass stands on its own:

  (a) logits within C_LOGIT units of 2^-24 sum_k |w_jk| |h_k| (the head's product): fp32 arithmetic on the engine's exact
      operands; the constant covers the layers in front of the head, and the __expf of the bf16 sharded step;
  (b) the newest cache row (row t, K and V, every layer): fp32 within C_KV units of 2^-24 (sum |w| |h| + |b|) of the QKV row; bf16
      equal to the bf16 rounding of the fp64 value, or to its other neighbour only where the fp64 value lies within that budget of
      the rounding midpoint (ar_step_ref.bf16_miss; near zero the budget may also reach the bf16 values of the other sign).  Row t
      of layer l + 1 probes layer l's output;
  (c) every wrong answer of ar_step_ref.WRONG (one key fewer at either end, the newest key twice, row t - 1 for row t, one split's
      key range dropped) at least SEP bounds from the engine's logits.

The prefill rows 0..n0-1 of every layer are checked against an fp64 forward of the prompt under the AR mask, in units of
u (sum |w| |h| + |b|), u = 2^-8 on bf16 engines (bf16 activations in the row kernels), 2^-24 on fp32 ones.  Every case asserts
which step ran from the kernels per pass of the captured step graph (sharded: 2 L + 2; five-launch: 5 L + 2, + 3 with the
audio prenet): tp_setup falls back to the five-launch step silently."""
import pytest
import torch

from ar_step_ref import U16, U32, WRONG, StepRef, bf16_miss

pytestmark = pytest.mark.gpu

# Worst errors measured on the MI355X (units as above; all eight cases) and the bounds at about 4x:
#   logits              0.824 (five-launch bf16, head_dim 16; sharded bf16 0.621, fp32 0.483 / 0.523)  -> C_LOGIT 3.5
#   newest cache rows   fp32 0.545; bf16: the engine's value is the fp64 value's bf16 rounding except within
#                       0.226 units of a midpoint                                                       -> C_KV 2.5
#   prefill rows        bf16 0.291 units of 2^-8, fp32 2.79 units of 2^-24                              -> C_PREFILL
# The nearest wrong answer measured 60 bounds away (the five-launch bf16 step at ctx 3072, newest key dropped or doubled).
Q_SHARPEN = 4.0
C_LOGIT = 3.5
C_KV = 2.5
C_PREFILL = {"bf16": 1.25, "fp32": 12.0}
SEP = 4.0
L = 2


def _units(err: torch.Tensor, scale: torch.Tensor) -> float:
    """max err / scale; where scale is 0 (the zeroed EOS row of the head) only err == 0 passes."""
    m = scale > 0
    if bool((err[~m] != 0).any()):
        return float("inf")
    return float((err[m] / scale[m]).max())


def _rows(*parts):
    return [list(p) if isinstance(p, range) else [p] for p in parts]


# rows: groups of checked newest rows t (the sharded step's n_old = t; the five-launch step's ctx = t + 1)
CASES = {
    "tp_bf16": dict(tp=True, precision="bf16", d=1024, H=16, S=1, P=0, bos=True, n=4100,
                    rows=_rows(range(2, 7), range(14, 19), range(2045, 2052), range(4093, 4101), 300, 1000, 3000)),
    "tp_fp32": dict(tp=True, precision="fp32", d=1024, H=16, S=1, P=0, bos=True, n=2052,
                    rows=_rows(range(2, 7), range(14, 19), range(1021, 1028), range(2045, 2052), 500, 1500)),
    "plain_bf16": dict(tp=False, precision="bf16", d=1024, H=16, S=1, P=0, bos=True, n=3076,
                       rows=_rows(range(2, 9), range(1533, 1539), range(3069, 3075), 700, 2300)),
    "plain_fp32": dict(tp=False, precision="fp32", d=1024, H=16, S=1, P=0, bos=True, n=772,
                       rows=_rows(range(2, 9), range(765, 771), 300)),
    "plain_bf16_d512": dict(tp=False, precision="bf16", d=512, H=8, S=6, P=10, bos=False, n=1530,
                            rows=_rows(range(16, 21), range(1533, 1539), 800)),
    "plain_bf16_hd16": dict(tp=False, precision="bf16", d=256, H=16, S=6, P=10, bos=False, n=1530,
                            rows=_rows(range(16, 21), range(1533, 1539), 800)),
    "plain_bf16_postnorm": dict(tp=False, precision="bf16", d=512, H=8, S=6, P=10, bos=False, n=1530, norm_first=False,
                                rows=_rows(range(16, 21), range(1533, 1539), 800)),
    "plain_bf16_prenet": dict(tp=False, precision="bf16", d=512, H=8, S=6, P=10, bos=False, n=1530, add_prenet=True,
                              rows=_rows(range(16, 21), range(1533, 1539), 800)),
}


def _decode(monkeypatch, c, seed):
    """(state dict, text, prompt, forced, traced logits (n_pass, 1025) fp64, cache (L, 2, H, rows, hd) fp64, step kernels)."""
    import __graft_entry__ as ge

    ge.build()
    from valle_amd.config import ModelConfig
    from valle_amd.engine import Engine, VxError
    from valle_amd.weights import synthetic_state_dict

    if c["tp"]:
        monkeypatch.delenv("VX_AR_TP", raising=False)
    else:
        monkeypatch.setenv("VX_AR_TP", "0")
    d, H = c["d"], c["H"]
    cfg = ModelConfig(decoder_dim=d, nhead=H, num_decoder_layers=L, prefix_mode=1, prepend_bos=c["bos"], num_quantizers=1,
                      norm_first=c.get("norm_first", True), add_prenet=c.get("add_prenet", False))
    sd = synthetic_state_dict(cfg, seed)
    for li in range(L):
        sd[f"ar_decoder.layers.{li}.self_attn.in_proj_weight"][:d] *= Q_SHARPEN
    g = torch.Generator().manual_seed(seed)
    text = torch.randint(3, 100, (c["S"],), generator=g)
    prompt = torch.randint(0, 1024, (c["P"],), generator=g)
    forced = torch.randint(0, 1024, (c["n"],), generator=g)
    max_text, max_audio = 16, int(c["bos"]) + c["P"] + c["n"] + 8
    e = Engine(cfg, c["precision"], max_text=max_text, max_audio=max_audio, trace_logits=True)
    try:
        e.load_state_dict(sd)
        e.ar_prefill(text, prompt)
        e.ar_decode(top_k=1, forced=forced)
        toks, _, n_pass = e.ar_result()
        assert torch.equal(toks, forced) and n_pass == c["n"] + 1
        kernels = e.timings()["step_kernels"]
        logits = e.read("ar_logits", (n_pass, 1025)).double()
        kv = e.read_ar_kv()
        esz = kv.element_size()
        with pytest.raises(VxError, match="out of range"):  # the tap ends where the cache ends
            e.read("ar_kv", (1,), kv.dtype, offset_bytes=kv.numel() * esz)
    finally:
        e.close()
    return sd, text, prompt, forced, logits, kv.double(), kernels, max_text + max_audio


@pytest.mark.parametrize("name", list(CASES))
def test_decode_step_matches_fp64_pass_by_pass(monkeypatch, name):
    c = CASES[name]
    kind = "tp" if c["tp"] else "plain"
    bf16 = c["precision"] == "bf16"
    d, H, S, bos = c["d"], c["H"], c["S"], int(c["bos"])
    sd, text, prompt, forced, logits, kv, kernels, rows_max = _decode(monkeypatch, c, seed=11)
    want = 2 * L + 2 if c["tp"] else 5 * L + 2 + (3 if c.get("add_prenet") else 0)
    assert kernels == want, f"{name}: {kernels} kernels per pass, the {kind} step has {want}"

    ref = StepRef(sd, d, H, L, c.get("norm_first", True), c.get("add_prenet", False), 1, bool(bos), bf16,
                  pe_rows=max(4000, rows_max))
    fails = []
    # prefill rows
    M = S + bos + c["P"]
    yy = torch.cat([torch.tensor([1025]) if bos else torch.zeros(0, dtype=torch.int64), prompt])
    u = U16 if bf16 else U32
    worst_pf = 0.0
    for li, (k, v, ka, va) in enumerate(ref.prefill_kv(text, yy)):
        for which, r, ab in ((0, k, ka), (1, v, va)):
            units = _units((kv[li, which, :, :M] - r).abs(), u * ab)
            worst_pf = max(worst_pf, units)
            if units > C_PREFILL[c["precision"]]:
                fails.append(f"prefill layer {li} {'KV'[which]}: {units:.3g} units")
    # decode passes
    worst_lg = worst_kv = 0.0
    seps = {w: (float("inf"), -1) for w in WRONG}
    group_sep = []
    for grp in c["rows"]:
        best = {w: 0.0 for w in WRONG}
        for t in grp:
            p = t - (M - 1)
            tok, pos = int(forced[p - 1]), t - S
            r = ref.forward(tok, pos, kv, t, kind=kind)
            got = logits[p]
            units = _units((got - r["logits"]).abs(), U32 * r["head_abs"])
            worst_lg = max(worst_lg, units)
            if units > C_LOGIT:
                fails.append(f"t={t} logits: {units:.4g} units")
            for li in range(L):
                for which, key in ((0, "k"), (1, "v")):
                    g, rr, ab = kv[li, which, :, t], r[key][li], r[key + "_abs"][li]
                    miss = bf16_miss(g, rr) if bf16 else (g - rr).abs()
                    units = _units(miss, U32 * ab)
                    worst_kv = max(worst_kv, units)
                    if units > C_KV:
                        fails.append(f"t={t} layer {li} newest {'KV'[which]}: {units:.4g} units")
            tol = C_LOGIT * U32 * r["head_abs"]
            for w in WRONG:
                sep = _units((ref.forward(tok, pos, kv, t, w, kind)["logits"] - got).abs(), tol)
                best[w] = max(best[w], sep)
                if sep < seps[w][0]:
                    seps[w] = (sep, t)
                if sep < SEP:
                    fails.append(f"t={t} wrong answer {w}: {sep:.3g} bounds")
        group_sep.append((grp[0], grp[-1], best))
    print(f"\n{name}: logits {worst_lg:.3g} units (bound {C_LOGIT}), newest rows {worst_kv:.3g} "
          f"(bound {C_KV}), prefill {worst_pf:.3g} (bound {C_PREFILL[c['precision']]}); nearest wrong answers "
          + ", ".join(f"{w} {s:.3g}@{t}" for w, (s, t) in seps.items()))
    for a, b, best in group_sep:
        print(f"  rows {a}..{b}: best separation " + ", ".join(f"{w} {s:.3g}" for w, s in best.items()))
    assert not fails, f"{name}: " + "; ".join(fails[:40])
