"""GPU: CTC forced alignment and text likelihood (falign_kernels.hpp behind vx_falign / vx_falign_asr, valle_amd.asr) against the
numpy restatement tests/ctc_align_ref.py, which test_ctc_align_cpu.py pins against F.ctc_loss and exhaustive enumeration.

1. vx_falign on the cases of tests/ctc_align_cases.py, one ragged batch per kind of logits (4 x randn; integers in [-3, 3], which tie
   exactly) and vocabulary (5, 32, 70): T in {1, 2, 3, 17, 255, 256, 257, 600} x L in {0, 1, 2, 127, 128, 129} and the longest L that
   T allows, adjacent repeats, T = L + repeats exactly (one path: nll == -path_logprob within the bound), T one less (infeasible),
   T = 0.  The frame tokens and the spans equal the restatement's exactly, ties included; nll and path_logprob stay within
   16 T 2^-52 max(1, |value|) of it (per frame one log, at most three exp and a few additions, each within an ulp or two of a
   magnitude that never exceeds the total); a score within that of its own magnitude plus one fp32 rounding; +inf, -inf, -1 and
   `feasible` hold exactly.  The measured ratios go to the file VX_CTC_ALIGN_PARITY_OUT names (profiles/ctc_align_parity.json comes
   from there).  That the bound tells a wrong lattice from the definition is checked without a GPU in test_ctc_align_cpu.py.
2. a ragged batch is bitwise every utterance alone, a second run is bitwise the first, the likelihood alone (ctc_nll, the sum
   without the max) gives the same bits, nothing is written outside the outputs (valle_amd.asr checks the guard entries).
3. vx_falign_asr on the tiny_group and tiny_layer recognisers with every utterance's own greedy transcript as the target, after
   asserting that no frame's top two logits tie (the greedy labelling is then the one best path, and it collapses to the target):
   every frame's aligned token id, the blank for a frame that emits nothing, is the frame's arg-max; the spans start at
   token_frames; path_logprob
   equals T x the mean log-probability (the restatement's fp64 mean within the bound, the engine's fp32 mean within one more fp32
   rounding: mean_logprob_out is fp32, so the bound alone cannot hold against it); nll <= -path_logprob; the call equals
   vx_falign on the logits read back, bitwise; a target that differs by one character has a larger nll.
4. SpeechRecognizer.align on 24 kHz input through the resampler: words and seconds against a hand composition of the pieces;
   VX_ERR_STATE before any recognize and on a different n; the limits."""
import json
import os

import numpy as np
import pytest
import torch

import asr_cases as AC
import asr_ref as AR
import ctc_align_cases as CC
import ctc_align_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_REC, _PARITY, _GOT = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge

    ge.build()
    yield
    for r in _REC.values():
        r.close()
    _REC.clear()
    out = os.environ.get("VX_CTC_ALIGN_PARITY_OUT")
    if out and _PARITY:
        with open(out, "w") as f:
            json.dump(_PARITY, f, indent=1, sort_keys=True)


def _rec(name):
    from valle_amd.asr import SpeechRecognizer

    if name not in _REC:
        _REC[name] = SpeechRecognizer(AC.config(name), AC.vocab(name), max_batch=8, max_seconds=2.7, state_dict=AC.state_dict(name)).to(DEV)
    return _REC[name]


def _run_group(kind, V):
    from valle_amd.asr import ctc_forced_align

    if (kind, V) not in _GOT:
        names, frames, x, targets, blank = CC.group(kind, V)
        _GOT[(kind, V)] = ctc_forced_align(torch.from_numpy(x).to(DEV), frames, targets, blank)
    return _GOT[(kind, V)]


def _same(a, b):
    """Bitwise equality of two CTCAlignment (no NaN is ever reported, so == on the floats is equality of bits up to the sign of 0)."""
    return (a.nll, a.path_logprob, a.feasible, a.frame_tokens, a.starts, a.ends, a.scores) == \
        (b.nll, b.path_logprob, b.feasible, b.frame_tokens, b.starts, b.ends, b.scores)


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,V", CC.GROUPS)
def test_falign_equals_the_restatement(kind, V):
    names, frames, x, targets, blank = CC.group(kind, V)
    want, got = CC.reference(kind, V), _run_group(kind, V)
    assert len(got) == len(want) == len(names)
    worst = {"nll": 0.0, "path_logprob": 0.0, "score": 0.0, "one_path": 0.0}
    bad, n_feasible = [], 0
    for name, T, y, w, g in zip(names, frames, targets, want, got):
        assert g.feasible == w["feasible"], name
        assert g.frame_tokens == w["frame_tokens"].tolist(), f"{name}: the frame tokens differ"
        assert g.starts == w["starts"].tolist() and g.ends == w["ends"].tolist(), f"{name}: the spans differ"
        if not w["feasible"]:
            assert g.nll == np.inf and g.path_logprob == -np.inf and all(s == -np.inf for s in g.scores), name
            assert all(v == -1 for v in g.frame_tokens + g.starts + g.ends), name
            continue
        if T == 0:
            assert g.nll == 0.0 and g.path_logprob == 0.0, name
            continue
        n_feasible += 1
        for key, a, b in (("nll", g.nll, w["nll"]), ("path_logprob", g.path_logprob, w["path_logprob"])):
            ratio = abs(a - b) / R.bound(T, b)
            worst[key] = max(worst[key], ratio)
            if not ratio <= 1.0:
                bad.append((name, key, a, b, ratio))
        for k, (a, b) in enumerate(zip(g.scores, w["scores"].tolist())):
            ratio = abs(a - b) / (R.bound(T, b) + 2.0 ** -24 * abs(b))
            worst["score"] = max(worst["score"], ratio)
            if not ratio <= 1.0:
                bad.append((name, f"score[{k}]", a, b, ratio))
        if name.endswith(("_exact", "_longest")):  # one feasible path: the sum is its only term
            ratio = abs(g.nll + g.path_logprob) / R.bound(T, g.nll)
            worst["one_path"] = max(worst["one_path"], ratio)
            if not ratio <= 1.0:
                bad.append((name, "nll + path_logprob", g.nll, g.path_logprob, ratio))
        assert g.nll <= -g.path_logprob + R.bound(T, g.nll), name
    print(f"{kind} V{V}: {n_feasible} feasible of {len(names)} utterances; error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    _PARITY[f"{kind}_V{V}"] = dict(worst, utterances=len(names), feasible=n_feasible, frames=int(sum(frames)))
    assert not bad, f"{kind} V{V}: beyond the bound: {bad[:8]}"


# ---- 2. bitwise -------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_is_bitwise_solo_and_repeatable():
    from valle_amd.asr import ctc_forced_align, ctc_nll

    names, frames, x, targets, blank = CC.group("int", 5)
    first = _run_group("int", 5)
    xd = torch.from_numpy(x).to(DEV)
    again = ctc_forced_align(xd, frames, targets, blank)
    assert all(_same(a, b) for a, b in zip(first, again)), "a second run differs"
    only = ctc_nll(xd, frames, targets, blank)
    assert only.tolist() == [a.nll for a in first], "the likelihood alone differs from the likelihood next to the path"
    parts = CC.split(frames, x)
    pick = [i for i, n in enumerate(names) if n in ("T1_L1", "T3_exact", "T17_repeats", "T0_L0", "T0_L3", "T255_L129", "T256_longest", "T257_L128",
                                                    "T600_exact", "T600_one_less", "T600_L2")]
    assert len(pick) == 11
    for i in pick:
        solo = ctc_forced_align(torch.from_numpy(np.ascontiguousarray(parts[i])).to(DEV).reshape(frames[i], 5), [frames[i]], [targets[i]], blank)[0]
        assert _same(solo, first[i]), f"{names[i]} differs from itself alone"


def test_limits():
    from valle_amd.asr import FALIGN_MAX_TARGETS, ctc_forced_align
    from valle_amd.engine import VxError

    L = FALIGN_MAX_TARGETS
    g = np.random.default_rng(3)
    y = [1 + k % 3 for k in range(L)]  # no adjacent repeat
    x = g.integers(-3, 4, (L + 2, 4)).astype(np.float32)
    got = ctc_forced_align(torch.from_numpy(x).to(DEV), [L + 2], [y], 0)[0]
    want = R.align(x, y, 0)
    assert got.frame_tokens == want["frame_tokens"].tolist() and got.starts == want["starts"].tolist() and got.ends == want["ends"].tolist()
    assert abs(got.nll - want["nll"]) <= R.bound(L + 2, want["nll"]) and abs(got.path_logprob - want["path_logprob"]) <= R.bound(L + 2, want["path_logprob"])
    with pytest.raises(VxError, match=f"{L + 1} targets, up to {L} are served") as ei:
        ctc_forced_align(torch.from_numpy(x).to(DEV), [L + 2], [y + [2 if y[-1] != 2 else 3]], 0)
    assert ei.value.code == 4


# ---- 3. on the recogniser's own logits --------------------------------------------------------------------------------------------
_ORDER = (64, 1, 130, 33, 17, 65, 2)


@pytest.mark.parametrize("name", ("tiny_group", "tiny_layer"))
def test_falign_asr_on_the_own_transcript(name):
    from valle_amd.asr import _FalignOut, ctc_forced_align

    rec = _rec(name)
    wavs = [AC.wave(name, f).to(DEV) for f in _ORDER]
    logits = [l.clone() for l in rec.logits(wavs, sr=16000)]
    for l in logits:
        top = l.topk(2, dim=1).values
        assert bool((top[:, 0] > top[:, 1]).all()), "a frame's top two logits tie: the greedy path would not be the only best one"
    hyps = rec.recognize(wavs, sr=16000)  # the handle's logits are this call's
    n, blank = len(wavs), rec.blank_id
    targets = [h.tokens for h in hyps]

    def run(ys):
        out = _FalignOut(n, sum(_ORDER), sum(len(y) for y in ys), rec.device, True)
        with torch.cuda.device(rec.device):
            rec._falign_raw(ys, *out.pointers())
        return out.split(_ORDER, [len(y) for y in ys])

    got = run(targets)
    flat = torch.cat(logits).contiguous()
    direct = ctc_forced_align(flat, _ORDER, targets, blank)
    for u, (T, h, g, d, l) in enumerate(zip(_ORDER, hyps, got, direct, logits)):
        assert _same(g, d), f"utterance {u}: vx_falign_asr differs from vx_falign on the logits read back"
        x = l.cpu().numpy()
        ids = x.argmax(1)
        assert g.feasible and g.starts == h.frames, u
        # without ties the greedy labelling is the one best path, and it collapses to the target: every frame emits its arg-max
        emitted = [h.tokens[k] if k >= 0 else blank for k in g.frame_tokens]
        assert emitted == ids.tolist(), u
        own = AR.ctc_greedy(x, blank)
        want = T * own[2]  # the restatement's mean in fp64
        assert abs(g.path_logprob - want) <= R.bound(T, want), (u, g.path_logprob, want)
        assert abs(g.path_logprob - T * h.logprob) <= R.bound(T, want) + 2.0 ** -24 * abs(want), (u, g.path_logprob, T * h.logprob)
        assert g.nll <= -g.path_logprob
        ref = R.align(x, h.tokens, blank)
        assert abs(g.nll - ref["nll"]) <= R.bound(T, ref["nll"]) and g.frame_tokens == ref["frame_tokens"].tolist()
    # one character changed: less likely
    inv = sorted(set(rec.vocab.values()) - {blank})
    other = []
    for y in targets:
        y = list(y)
        if y:
            y[len(y) // 2] = next(t for t in inv if t != y[len(y) // 2])
        other.append(y)
    worse = run(other)
    changed = 0
    for u, (a, b, y) in enumerate(zip(got, worse, targets)):
        if y:
            changed += 1
            assert b.nll > a.nll, (u, a.nll, b.nll)
    assert changed >= 5


# ---- 4. the recogniser's align ------------------------------------------------------------------------------------------------------
def test_align_is_the_hand_composed_chain():
    from valle_amd.asr import ctc_forced_align, ctc_nll, ids_to_text, text_likelihood
    from valle_amd.codec import Resampler

    rec = _rec("tiny_layer")
    g = torch.Generator().manual_seed(24)
    wav24 = [(0.3 * torch.randn(30000, generator=g)).to(DEV), (0.3 * torch.randn(12345, generator=g)).to(DEV)]
    texts = ["it's a cat, on the mat", "No"]
    got = rec.align(wav24, texts)  # the default rate is 24 kHz
    rs = Resampler(24000, 16000).to(DEV)
    wav16 = [rs(w).reshape(-1) for w in wav24]
    logits = rec.logits(wav16, sr=16000)
    frames = [l.shape[0] for l in logits]
    ids = [rec.text_to_ids(t) for t in texts]
    assert ids[1] == [rec.vocab["N"], rec.vocab["O"]] and rec.vocab["|"] in ids[0]
    raw = ctc_forced_align(torch.cat(logits).contiguous(), frames, ids, rec.blank_id)
    hyps = rec.recognize(wav16, sr=16000)
    spf = 320 / 16000
    for a, r, y, t, h in zip(got, raw, ids, texts, hyps):
        assert a.feasible and a.nll == r.nll and a.path_logprob == r.path_logprob and a.nll_per_char == r.nll / len(y)
        assert a.transcript == h and a.frame_tokens == r.frame_tokens
        assert a.text == AR.normalize_text(t) == ids_to_text(y, rec.id_to_token)
        assert [c.char for c in a.chars] == list(a.text)
        assert [(c.start_s, c.end_s, c.score) for c in a.chars] == [(s * spf, e * spf, sc) for s, e, sc in zip(r.starts, r.ends, r.scores)]
        words = a.text.split()
        assert [w.word for w in a.words] == words
        k = 0
        for w in a.words:
            cs = a.chars[k:k + len(w.word)]
            assert (w.start_s, w.end_s) == (cs[0].start_s, cs[-1].end_s) and w.score == sum(c.score for c in cs) / len(cs)
            k += len(w.word) + 1
        assert all(x.end_s <= y_.start_s for x, y_ in zip(a.chars, a.chars[1:]))
    scores = rec.score_text(wav24, texts)
    assert [s.nll for s in scores] == [a.nll for a in got] == ctc_nll(torch.cat(logits).contiguous(), frames, ids, rec.blank_id).tolist()
    assert text_likelihood(texts[1], wav24[1], rec)[0] == scores[1] and scores[1].n_chars == 2
    with pytest.raises(ValueError, match="'9'"):
        rec.align(wav24[:1], ["at 9"])
    # more characters than frames: reported, not raised
    short = rec.align(wav24[1][:900], "this text is far too long for two frames")[0]
    assert not short.feasible and short.nll == np.inf and short.chars == [] and short.words == []


def test_state_refusals():
    from valle_amd.asr import SpeechRecognizer
    from valle_amd.engine import VxError

    rec = SpeechRecognizer(AC.config("tiny_group"), AC.vocab("tiny_group"), max_batch=4, max_seconds=1.0, state_dict=AC.state_dict("tiny_group")).to(DEV)
    nll = torch.zeros(4, dtype=torch.float64, device=DEV)
    args = (nll.data_ptr(), None, None, None, None, None, None)
    with pytest.raises(VxError, match="before any vx_asr_recognize") as ei:
        rec._falign_raw([[5]], *args)
    assert ei.value.code == 3
    before = rec.workspace_bytes()
    rec.recognize([AC.wave("tiny_group", 17).to(DEV), AC.wave("tiny_group", 33).to(DEV)], sr=16000)
    with pytest.raises(VxError, match="n = 1 utterances, the last vx_asr_recognize served 2") as ei:
        rec._falign_raw([[5]], *args)
    assert ei.value.code == 3
    with torch.cuda.device(rec.device):
        rec._falign_raw([[5], [6, 7]], *args)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(nll[:2]).all()) and rec.workspace_bytes() > before  # the scratch is the handle's and is reported
    rec.close()
