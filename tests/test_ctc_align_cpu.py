"""CPU: CTC forced alignment and text likelihood (vx_falign, vx_falign_asr, valle_amd.asr), the definition and the packaging, no GPU.

1. the restatement tests/ctc_align_ref.py equals F.ctc_loss(reduction="none") in fp64 at 1e-12 relative, up to (T, V, L) =
   (999, 32, 300), with and without repeated labels;
2. it equals exhaustive enumeration of every labelling at T <= 6, V = 3 for the targets [], [1], [1, 1], [1, 2], [2, 1, 2]: the
   sum, the best path's value, and on integer logits (exact ties) the path the tie rule picks: among the best labellings the one
   whose state sequence is largest read from the last frame backwards, which is what "the first of s, s - 1, s - 2" unrolls to;
3. infeasible pairs give +inf, never a NaN;
4. each of ctc_align_ref.MUTATIONS moves nll by at least 1000 x the GPU test's bound on at least 20 of the GPU test's own cases
   (ctc_align_cases): the condition under which that bound tells a wrong lattice from the definition;
5. the new symbols are declared, bound and exported; every host-side refusal gives its code and message before any HIP call;
6. text to ids and word grouping."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import asr_cases as AC
import ctc_align_cases as CC
import ctc_align_ref as R
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library()


# ---- 1. against F.ctc_loss -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,V,L,repeats", ((1, 3, 1, False), (5, 3, 2, True), (17, 5, 6, True), (64, 32, 20, False), (300, 32, 128, True),
                                           (999, 32, 300, False), (999, 32, 300, True), (40, 70, 0, False)))
def test_restatement_equals_ctc_loss(T, V, L, repeats):
    g = np.random.default_rng(T * 131 + L)
    x = (4.0 * g.standard_normal((T, V))).astype(np.float32)
    y = g.integers(1, V, L).tolist()
    if repeats:
        for k in range(1, L, 3):
            y[k] = y[k - 1]
    assert R.feasible(T, y)
    lp = torch.log_softmax(torch.from_numpy(x).double(), 1)[:, None, :]
    want = float(torch.nn.functional.ctc_loss(lp, torch.tensor([y], dtype=torch.long).reshape(1, L), torch.tensor([T]), torch.tensor([L]),
                                              blank=0, reduction="none", zero_infinity=False)[0])
    got = R.nll(x, y, 0)
    rel = abs(got - want) / max(1.0, abs(want))
    print(f"T {T} V {V} L {L} repeats {repeats}: nll {got:.6f}, against F.ctc_loss {rel:.2e} relative")
    assert rel <= 1e-12
    full = R.align(x, y, 0)
    assert full["nll"] == got and full["path_logprob"] <= -got + 1e-9 * max(1.0, abs(got))


# ---- 2. against enumeration ------------------------------------------------------------------------------------------------------
def _states_of(labels, y, blank=0):
    """The state sequence of a labelling that collapses to y (None when it does not)."""
    k, prev, states = -1, None, []
    for c in labels:
        if c == blank:
            states.append(2 * (k + 1))
        elif prev == c and k >= 0:
            states.append(2 * k + 1)
        else:
            k += 1
            if k >= len(y) or y[k] != c:
                return None
            states.append(2 * k + 1)
        prev = c
    return states if k == len(y) - 1 else None


def _enumerate(x, y, blank=0):
    T, V = x.shape
    lse = R.lse_rows(x)
    x64 = x.astype(np.float64)
    logps, best = [], None
    for labels in itertools.product(range(V), repeat=T):
        st = _states_of(labels, y, blank)
        if st is None:
            continue
        raw = 0.0
        for t, c in enumerate(labels):
            raw += x64[t, c]
        logps.append(raw - lse.sum())
        key = (raw, tuple(reversed(st)))
        if best is None or key > best[0]:
            best = (key, st)
    return logps, best


@pytest.mark.parametrize("kind", ("randn", "int"))
@pytest.mark.parametrize("y", ([], [1], [1, 1], [1, 2], [2, 1, 2]))
def test_restatement_equals_enumeration(y, kind):
    g = np.random.default_rng(len(y) * 7 + (kind == "int"))
    for T in range(1, 7):
        for _ in range(4):
            x = g.integers(-2, 3, (T, 3)).astype(np.float32) if kind == "int" else (2.0 * g.standard_normal((T, 3))).astype(np.float32)
            logps, best = _enumerate(x, y)
            got = R.align(x, y, 0)
            assert got["feasible"] == bool(logps) == R.feasible(T, y)
            if not logps:
                assert got["nll"] == np.inf and got["path_logprob"] == -np.inf and (got["frame_tokens"] == -1).all()
                continue
            want = -float(np.logaddexp.reduce(np.array(logps)))
            assert abs(got["nll"] - want) <= 1e-12 * max(1.0, abs(want)), (T, y, got["nll"], want)
            (raw, _), st = best
            assert abs(got["path_logprob"] - (raw - R.lse_rows(x).sum())) <= 1e-12 * max(1.0, abs(raw))
            if kind == "int":  # every sum is exact: the value and the tie rule's path, exactly
                assert got["path_logprob"] == raw - R.lse_rows(x).sum()
                assert got["states"].tolist() == st, (T, y, x.tolist())
            toks = [s // 2 if s % 2 else -1 for s in got["states"].tolist()]
            assert got["frame_tokens"].tolist() == toks
            for k in range(len(y)):
                at = [t for t, v in enumerate(toks) if v == k]
                assert at == list(range(got["starts"][k], got["ends"][k])) and at


def test_tie_rule_by_hand():
    # all-zero logits: every path ties.  T = 4, y = [1]: the last state first (S - 1 = the trailing blank), then staying put for as
    # long as the lattice allows: blank blank, and the token as early as it must be
    x = np.zeros((4, 3), dtype=np.float32)
    got = R.align(x, [1], 0)
    assert got["states"].tolist() == [1, 2, 2, 2] and got["starts"].tolist() == [0] and got["ends"].tolist() == [1]
    assert abs(got["scores"][0] + math.log(3.0)) < 1e-6 and abs(got["path_logprob"] + 4 * math.log(3.0)) < 1e-12
    assert R.align(x, [1, 1], 0)["states"].tolist() == [1, 2, 3, 4]


# ---- 3. infeasible ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,y", ((0, [1]), (1, [1, 2]), (2, [1, 1]), (3, [1, 1, 2]), (4, [2, 2, 2])))
def test_infeasible_is_inf(T, y):
    x = np.random.default_rng(T).standard_normal((T, 3)).astype(np.float32)
    got = R.align(x, y, 0)
    assert got["nll"] == np.inf and not got["feasible"] and got["path_logprob"] == -np.inf
    assert (got["starts"] == -1).all() and (got["ends"] == -1).all() and np.isneginf(got["scores"]).all()
    more = np.random.default_rng(T).standard_normal((T + 1, 3)).astype(np.float32)
    assert np.isfinite(R.nll(more, y, 0)) and R.feasible(T + 1, y)


def test_nothing_against_nothing():
    got = R.align(np.zeros((0, 4), dtype=np.float32), [], 0)
    assert got["nll"] == 0.0 and got["feasible"] and got["path_logprob"] == 0.0


# ---- 4. the mutations ------------------------------------------------------------------------------------------------------------
def test_every_mutation_moves_the_likelihood():
    """Per mutation, over every feasible case of the GPU test: how many cases it moves by at least 1000 x the bound (a mistake in the
    skip rule cannot show on a target without the pattern it mishandles, and a lost start or end state weighs nothing where that
    state carries no probability), and the largest finite move in units of the bound."""
    caught, largest = {m: 0 for m in R.MUTATIONS}, {m: (0.0, "") for m in R.MUTATIONS}
    for kind, V in CC.GROUPS:
        names, frames, x, targets, blank = CC.group(kind, V)
        for name, xi, y, ref in zip(names, CC.split(frames, x), targets, CC.reference(kind, V)):
            T = len(xi)
            if not ref["feasible"] or T == 0:
                continue
            want = ref["nll"]
            for m in R.MUTATIONS:
                got = R.nll(xi, y, blank, mutation=m)
                ratio = abs(got - want) / R.bound(T, want)  # inf where the mistake leaves no path at all
                caught[m] += ratio >= 1000.0
                if np.isfinite(ratio) and ratio > largest[m][0]:
                    largest[m] = (ratio, f"{kind}_V{V}_{name}")
    for m in R.MUTATIONS:
        print(f"{m:15s} moves nll by >= 1000 x the bound on {caught[m]:3d} cases, at most by {largest[m][0]:.3e} x (on {largest[m][1]})")
    print(f"smallest ratio: {min(v[0] for v in largest.values()):.3e}")
    assert all(caught[m] >= 20 for m in R.MUTATIONS), caught
    assert all(largest[m][0] >= 1000.0 for m in R.MUTATIONS), largest


# ---- 5. ABI and refusals ---------------------------------------------------------------------------------------------------------
NAMES = ["vx_falign", "vx_falign_asr"]


def test_header_ctypes_exports(lib):
    from valle_amd import engine

    hdr = open(os.path.join(ROOT, "include", "vallex.h")).read()
    declared = sorted(set(re.findall(r"\b(vx_falign[a-z0-9_]*)\s*\(", hdr)))
    assert declared == NAMES == [s for s in engine.declared_symbols() if s.startswith("vx_falign")]
    for name in NAMES:
        assert hasattr(lib, name), f"{name} declared in vallex.h but not exported"


FAKE = 4096  # never dereferenced: the checks come first


def _falign(lib, vocab, blank, frames, targets, outs=(FAKE,) * 7, logits=FAKE):
    n = len(frames)
    flat = [t for y in targets for t in y]
    arr = lambda v: (C.c_int32 * max(len(v), 1))(*v)  # noqa: E731
    return lib.vx_falign(logits, vocab, blank, n, arr(frames), arr(flat), arr([len(y) for y in targets]), *outs, None)


def test_refusals_before_any_hip_call(lib):
    assert _falign(lib, 5, 0, [3], [[1]], logits=None) == 1 and b"null argument" in lib.vx_last_error()
    assert _falign(lib, 5, 0, [3], [[1]], outs=(None,) * 7) == 1 and b"no output requested" in lib.vx_last_error()
    assert lib.vx_falign(FAKE, 5, 0, 0, (C.c_int32 * 1)(3), (C.c_int32 * 1)(1), (C.c_int32 * 1)(1), *(FAKE,) * 7, None) == 1
    assert b"n 0" in lib.vx_last_error()
    assert _falign(lib, 0, 0, [3], [[1]]) == 1 and b"vocab 0" in lib.vx_last_error()
    assert _falign(lib, 5, 5, [3], [[1]]) == 1 and b"blank 5" in lib.vx_last_error()
    assert _falign(lib, 5, -1, [3], [[1]]) == 1
    assert _falign(lib, 5, 0, [3, -1], [[1], [1]]) == 1 and b"utterance 1: -1 frames" in lib.vx_last_error()
    assert lib.vx_falign(FAKE, 5, 0, 1, (C.c_int32 * 1)(3), (C.c_int32 * 1)(1), (C.c_int32 * 1)(-2), *(FAKE,) * 7, None) == 1
    assert b"-2 targets" in lib.vx_last_error()
    assert lib.vx_falign(FAKE, 5, 0, 1, (C.c_int32 * 1)(3), None, (C.c_int32 * 1)(1), *(FAKE,) * 7, None) == 1
    assert b"null targets" in lib.vx_last_error()
    assert _falign(lib, 5, 2, [3, 9], [[1], [1, 3, 2]]) == 1 and b"utterance 1: target 2 is id 2" in lib.vx_last_error()  # the blank
    assert _falign(lib, 5, 0, [9], [[1, 5]]) == 1 and b"utterance 0: target 1 is id 5" in lib.vx_last_error()
    assert _falign(lib, 5, 0, [9], [[-1]]) == 1 and b"target 0 is id -1" in lib.vx_last_error()
    from valle_amd.asr import FALIGN_MAX_TARGETS

    assert FALIGN_MAX_TARGETS == 1000
    long = [1 + k % 2 for k in range(FALIGN_MAX_TARGETS + 1)]
    assert _falign(lib, 5, 0, [1500], [long]) == 4 and b"1001 targets, up to 1000 are served" in lib.vx_last_error()
    assert _falign(lib, 5, 0, [2 ** 30], [[1] * 8] * 1, outs=(FAKE, FAKE) + (None,) * 5) == 4 and b"workspace limit" in lib.vx_last_error()


def test_handle_refusals_before_any_hip_call(lib):
    from valle_amd import engine as e
    from valle_amd.asr import SpeechRecognizer

    rec = SpeechRecognizer(AC.config("tiny_layer"), AC.vocab("tiny_layer"), max_batch=2, max_seconds=1.0, state_dict=AC.state_dict("tiny_layer"))
    with pytest.raises(e.VxError, match="before any vx_asr_recognize") as ei:
        rec._falign_raw([[5, 6]], FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE)
    assert ei.value.code == 3
    with pytest.raises(e.VxError, match="no output requested") as ei:
        rec._falign_raw([[5, 6]], None, None, None, None, None, None, None)
    assert ei.value.code == 1
    assert lib.vx_falign_asr(None, 1, None, None, *(FAKE,) * 7, None) == 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rec.align(torch.zeros(8000), "hi")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rec.score_text(torch.zeros(8000), "hi")
    rec.close()


# ---- 6. text ---------------------------------------------------------------------------------------------------------------------
def test_text_to_ids_and_words():
    from valle_amd.asr import CharSpan, SpeechRecognizer, group_words

    v = AC.vocab("tiny_group")
    rec = SpeechRecognizer(AC.config("tiny_group"), v, max_batch=1, max_seconds=1.0)
    assert rec.text_to_ids("Hi,  there!") == [v[c] for c in "HI|THERE"]
    assert rec.text_to_ids("") == [] and rec.text_to_ids(" ... ") == []
    assert rec.text_to_ids("it's") == [v["I"], v["T"], v["'"], v["S"]]
    with pytest.raises(ValueError, match="'9'"):
        rec.text_to_ids("at 9 o'clock")
    assert rec.seconds_per_frame == 320 / 16000
    rec.close()
    chars = [CharSpan("H", 0.0, 0.02, -1.0), CharSpan("I", 0.04, 0.08, -3.0), CharSpan(" ", 0.08, 0.1, -9.0), CharSpan(" ", 0.1, 0.12, -9.0),
             CharSpan("A", 0.2, 0.22, -0.5)]
    words = group_words(chars)
    assert [(w.word, w.start_s, w.end_s, w.score) for w in words] == [("HI", 0.0, 0.08, -2.0), ("A", 0.2, 0.22, -0.5)]
    assert group_words([]) == [] and group_words([CharSpan(" ", 0.0, 0.02, -1.0)]) == []


def test_package_exports():
    import valle_amd

    for name in ("TextAlignment", "TextScore", "ctc_forced_align", "ctc_nll", "text_likelihood"):
        assert name in valle_amd.__all__ and getattr(valle_amd, name) is not None
    from valle_amd.asr import SpeechRecognizer
    from valle_amd.codec import EncodecDecoder

    assert callable(EncodecDecoder.roundtrip_text_likelihood) and callable(SpeechRecognizer.align) and callable(SpeechRecognizer.score_text)
