"""fp64 restatement of what generation records on engines created with VX_FLAG_LOGPROBS, and the floor its checks are held to.

    logprob_pick(rows, tokens)    rows (n, V) of any float type, tokens (n,) -> fp64 (n,): rows[i, tokens[i]] - logsumexp(rows[i]),
                                  max-subtracted, -inf entries add 0, a -inf target gives -inf (never NaN)
    floor(rows, tokens)           the worst absolute error of torch.log_softmax in fp32 ON THE HOST over the same rows, at the same
                                  tokens, against logprob_pick: what one careful fp32 implementation loses.  The engine's worst
                                  error must be at most 4 x this (the project's floor rule); it never depends on the code under test
    check(got, rows, tokens)      asserts that rule and returns (engine error, floor, ratio)
    ar_targets(...)               the token every pass of an AR decode is scored at
"""
import torch

EOS = 1024
EOS_STOPS = (1, 2)  # VX_STOP_EOS_ARGMAX, VX_STOP_EOS_SAMPLE


def logprob_pick(rows: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
    lg = rows.double()
    tv = lg.gather(1, tokens.reshape(-1, 1).long())
    m = lg.amax(1, keepdim=True)
    lse = m + torch.log(torch.exp(lg - m).sum(1, keepdim=True))  # exp(-inf) = 0
    return torch.where(torch.isinf(tv) & (tv < 0), torch.full_like(tv, float("-inf")), tv - lse)[:, 0]


def floor(rows: torch.Tensor, tokens: torch.Tensor) -> float:
    ref = logprob_pick(rows, tokens)
    t32 = torch.log_softmax(rows.float().cpu(), dim=1).gather(1, tokens.reshape(-1, 1).long().cpu())[:, 0]
    fin = torch.isfinite(ref)
    return float((t32.double()[fin] - ref[fin]).abs().max())


def check(got: torch.Tensor, rows: torch.Tensor, tokens: torch.Tensor, what: str = ""):
    """got (n,) fp32 from the engine.  Non-finite reference entries (a -inf target) must be reproduced exactly; the others lie
    within 4 x floor.  The figures are printed before the assertion."""
    ref = logprob_pick(rows, tokens)
    got = got.double().cpu()
    fin = torch.isfinite(ref)
    assert torch.equal(got[~fin], ref[~fin]), (what, got[~fin], ref[~fin])
    assert bool(torch.isfinite(got[fin]).all()), (what, got)
    err = float((got[fin] - ref[fin]).abs().max())
    fl = floor(rows, tokens)
    ratio = err / max(fl, 1e-300)
    print(f"logprobs {what}: engine worst |err| {err:.3e}, torch fp32 log_softmax {fl:.3e}, ratio {ratio:.3f} ({int(fin.sum())} rows)")
    assert err <= 4 * fl, (what, err, fl)
    return err, fl, ratio


def ar_targets(sampled: torch.Tensor, n_tokens: int, stop_reason: int, forced=None) -> torch.Tensor:
    """(n_pass,) int64: pass i is scored at forced[i] where teacher forcing supplies a token, at EOS when it is the pass that ended
    the decode on EOS, else at the sampled token."""
    t = sampled.long().clone()
    if forced is not None:
        k = min(int(forced.numel()), t.numel())
        t[:k] = forced[:k].long().cpu()
    if stop_reason in EOS_STOPS:
        assert t.numel() == n_tokens + 1
        t[-1] = EOS
    return t
