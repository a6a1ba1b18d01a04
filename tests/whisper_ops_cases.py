"""The cases of the Whisper token-loop kernel tests, shared by test_whisper_ops_cpu.py (which vets them) and test_gpu_whisper_ops.py
(which only compares): seeded inputs, the fp64 references (whisper_ops_ref, computed once per case and left unchanged) and the floors.

Bound of a real-valued case: the project's rule, kernel max-abs error <= TOL_FACTOR x floor, the floor being the same operation in
torch fp32 on the host against fp64, measured per case (per launch for attention).  An exact case has no bound: its inputs are small
integers, every partial sum of any summation order is an integer below 2^24 (or a dyadic fraction of one), so fp32 gives the same
bits whatever the order, and the kernel's output equals the reference bitwise."""
import torch

import whisper_ops_ref as OR

TOL_FACTOR = 4.0
MUTATION_FACTOR = 10.0   # a deliberate mistake moves a real-valued case by at least this many bounds
LOGPROB_REL = 2.0 ** -22  # the head's log-probabilities: |err| <= LOGPROB_REL max(1, |v|), as in test_gpu_whisper.py
HD = 64

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) % (2 ** 31))


# ---- skinny GEMM ----------------------------------------------------------------------------------------------------------------------
# (M, N, K).  cpw 8: N < 1024; 16: N = 8200; 64: N = 32773 (odd, the last workgroup ragged: 32773 = 512 x 64 + 5).  K 2048 is one
# chunk of exactly 64 KiB, 2064 a short second chunk, 5120 three chunks with a short last one.  M 9 and 17: a ragged second / third row
# tile, 64: eight tiles.
GEMM_EXACT_SHAPES = ((1, 24, 64), (8, 101, 192), (9, 101, 384), (17, 520, 2048), (9, 520, 2064), (64, 104, 5120), (9, 8200, 2064), (3, 32773, 128))
GEMM_EXACT_VARIANTS = tuple((b, r) for b in (False, True) for r in (False, True))  # (bias, residual aliased to the output)
# name -> (M, N, K, act, residual)
GEMM_REAL = {
    "tiny_head_9x51865x384": (9, 51865, 384, OR.ACT_NONE, False),
    "base_fc1_8x2048x512_gelu": (8, 2048, 512, OR.ACT_GELU, False),
    "base_fc2_16x512x2048_res": (16, 512, 2048, OR.ACT_NONE, True),
    "9x520x3072_gelu_res": (9, 520, 3072, OR.ACT_GELU, True),
    "64x520x5120": (64, 520, 5120, OR.ACT_NONE, False),
}
GEMM_SOLO_ROWS_CASE = "64x520x5120"  # row m of the M = 64 call is bitwise the M = 1 call of that row


def gemm_exact_inputs(shape):
    """x in [-4, 4], W in [-8, 8], bias and residual in [-16, 16], all integers: |any partial sum| <= 32 K + 32 < 2^24."""
    def make():
        M, N, K = shape
        g = _gen(1, M, N, K)
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        return dict(x=ri(-4, 4, M, K), W=ri(-8, 8, N, K), bias=ri(-16, 16, N), res=ri(-16, 16, M, N))
    return _once(("gemm_exact", shape), make)


def gemm_exact_want(shape, bias, res, dtype=torch.float64, mut=()):
    def make():
        i = gemm_exact_inputs(shape)
        return OR.gemm(i["x"], i["W"], i["bias"] if bias else None, i["res"] if res else None, OR.ACT_NONE, dtype, mut)
    return _once(("gemm_exact_want", shape, bias, res, dtype, tuple(mut)), make)


def gemm_real_inputs(name):
    def make():
        M, N, K, act, res = GEMM_REAL[name]
        g = _gen(2, M, N, K)
        rn = lambda *s: torch.randn(*s, generator=g)
        return dict(x=rn(M, K), W=rn(N, K) * (1.5 / K ** 0.5), bias=rn(N) * 0.3, res=rn(M, N) if res else None)
    return _once(("gemm_real", name), make)


def gemm_real_want(name, dtype=torch.float64, mut=()):
    def make():
        i, act = gemm_real_inputs(name), GEMM_REAL[name][3]
        return OR.gemm(i["x"], i["W"], i["bias"], i["res"], act, dtype, mut)
    return _once(("gemm_real_want", name, dtype, tuple(mut)), make)


def gemm_real_floor(name):
    return float((gemm_real_want(name, torch.float32).double() - gemm_real_want(name)).abs().max())


# ---- decode attention -----------------------------------------------------------------------------------------------------------------
ATTN_H = 2
ATTN_DOMINANT_T = (1, 2, 3, 5, 257, 448, 1500, 4096)
ATTN_UNIFORM_T = (256, 512, 4096)
ATTN_SELF_T = (1, 4, 33, 255, 256, 257, 300, 448)  # pos + 1 of the eight utterances of the real-valued self-attention launch
ATTN_CROSS_KEYS = (75, 256, 257, 1500)             # one real-valued launch of eight utterances each
ATTN_REAL = {"self": ATTN_SELF_T, **{f"cross{k}": (k,) * 8 for k in ATTN_CROSS_KEYS}}
SCORE_STD = 3.0


def dominant_places(T):
    """Where the dominant key is put: one utterance per place."""
    per = OR.per_quarter(T)
    return sorted({j for j in (0, 255, 256, per - 1, per, T - 1) if 0 <= j < T})


def attn_dominant_inputs(T, self_mode):
    """n = len(dominant_places(T)) utterances x 2 heads.  q is +-4, the keys are in [-1, 1] (|q . k| / 8 <= 32), the dominant key is
    8 sign(q) (q . k / 8 = 256): it leads every other key by at least 224 > 200 and exp(-224) is 0 in fp32 (the smallest
    subnormal is exp(-103.3)), so p is exactly 1 there and 0 elsewhere.  Head 0 of utterance u has it at places[u], head 1 at places[-1 - u].  K, V: (n, T, H, 64); in self mode
    row T - 1 of the cache holds NaN (the poison) and knew / vnew (n, H, 64) hold the key and value."""
    def make():
        places = dominant_places(T)
        n = len(places)
        g = _gen(3, T, int(self_mode))
        q = (torch.randint(0, 2, (n, ATTN_H, HD), generator=g) * 2 - 1).float() * 4
        K = torch.randint(-1, 2, (n, T, ATTN_H, HD), generator=g).float()
        V = torch.randint(-8, 9, (n, T, ATTN_H, HD), generator=g).float()
        dom = torch.tensor([[places[u], places[-1 - u]] for u in range(n)])
        for u in range(n):
            for h in range(ATTN_H):
                K[u, dom[u, h], h] = 8 * torch.sign(q[u, h])
        out = dict(q=q, K=K, V=V, dom=dom, want=torch.stack([torch.stack([V[u, dom[u, h], h] for h in range(ATTN_H)]) for u in range(n)]))
        if self_mode:
            out["knew"], out["vnew"] = K[:, T - 1].clone(), V[:, T - 1].clone()
            K[:, T - 1], V[:, T - 1] = float("nan"), float("nan")
        return out
    return _once(("attn_dom", T, self_mode), make)


def attn_uniform_inputs(T, self_mode):
    """q = 0, integer V, T a power of two: p = 1 / T exactly and the output is the exact mean."""
    def make():
        n = 2
        g = _gen(4, T, int(self_mode))
        K = torch.randint(-3, 4, (n, T, ATTN_H, HD), generator=g).float()
        V = torch.randint(-8, 9, (n, T, ATTN_H, HD), generator=g).float()
        out = dict(q=torch.zeros(n, ATTN_H, HD), K=K, V=V, want=(V.double().sum(1) / T).float())
        if self_mode:
            out["knew"], out["vnew"] = K[:, T - 1].clone(), V[:, T - 1].clone()
            K[:, T - 1], V[:, T - 1] = float("nan"), float("nan")
        return out
    return _once(("attn_uni", T, self_mode), make)


def attn_real_inputs(name):
    """Eight utterances x 2 heads with their own T; K, V: (8, max T, H, 64) (the rows from T on are other data that must not be
    read); in self mode row T - 1 of the cache holds stale random data and knew / vnew the step's own."""
    def make():
        Ts = ATTN_REAL[name]
        n, Tm = len(Ts), max(Ts)
        g = _gen(5, Tm, len(name))
        rn = lambda *s: torch.randn(*s, generator=g)
        out = dict(T=Ts, q=rn(n, ATTN_H, HD) * SCORE_STD, K=rn(n, Tm, ATTN_H, HD), V=rn(n, Tm, ATTN_H, HD))
        if name == "self":
            out["knew"], out["vnew"] = rn(n, ATTN_H, HD), rn(n, ATTN_H, HD)
        return out
    return _once(("attn_real", name), make)


def attn_reference(i, dtype, mut=(), T=None):
    """(n, H, 64) of whisper_ops_ref.attn over a case's inputs."""
    n = i["q"].shape[0]
    Ts = i.get("T", T)
    rows = []
    for u in range(n):
        t = Ts[u] if isinstance(Ts, (tuple, list)) else (Ts or i["K"].shape[1])
        rows.append(torch.stack([OR.attn(i["q"][u, h], i["K"][u, :t, h], i["V"][u, :t, h], dtype, None if "knew" not in i else i["knew"][u, h],
                                         None if "vnew" not in i else i["vnew"][u, h], mut) for h in range(ATTN_H)]))
    return torch.stack(rows)


def attn_real_want(name, dtype=torch.float64, mut=()):
    return _once(("attn_real_want", name, dtype, tuple(mut)), lambda: attn_reference(attn_real_inputs(name), dtype, mut))


def attn_real_floor(name):
    return float((attn_real_want(name, torch.float32).double() - attn_real_want(name)).abs().max())


# ---- the head -------------------------------------------------------------------------------------------------------------------------
HEAD_V = (101, 255, 256, 257, 513, 51865)
HEAD_OUT_STRIDE, HEAD_PROMPT_STRIDE, HEAD_MAX_TARGET = 6, 40, 40


def head_case(V):
    """One batched call on V logits a row.  Suppress map: ids 1, 2, 7 suppressed, 3 and eos = V - 5 begin-suppressed.  Returns
    dict(logits (n, V), smap, prompt, n_prompt, max_new, state (4 lists), eos, rows: what every row is there for)."""
    def make():
        g = _gen(6, V)
        eos = V - 5
        smap = [0] * V
        for i in (1, 2, 7):
            smap[i] = OR.SUPPRESS
        for i in (3, eos):
            smap[i] |= OR.BEGIN_SUPPRESS
        rows, logits, st = [], [], []

        def add(what, row, pos, n_prompt=2, max_new=HEAD_OUT_STRIDE, finished=0, cur=9, count=None):
            rows.append(what); logits.append(row)
            st.append(dict(cur=cur, pos=pos, count=max(pos + 1 - n_prompt, 0) if count is None else count, finished=finished, n_prompt=n_prompt,
                           max_new=max_new))

        def rnd():
            return torch.randn(V, generator=g) * 3.0

        def peak(row, idx, by=1.0):
            top = float(row.max()) + by
            for i in idx:
                row[i] = top
            return row

        far = V > 256  # a thread owns more than one logit
        # inside one thread's stride when the row is long enough; then a thread t < 128 that holds index t + 256 while its partner
        # at w = 128 holds the lower t + 128
        a, b = (5, 5 + 256) if V > 261 else (0, 256) if far else (5, 6)
        lo, hi = (133, 5 + 256) if V > 261 else (128, 256) if far else (5, 133 % V)
        add("plain_g0", rnd(), pos=1)
        add("plain_g1", rnd(), pos=2)
        add("plain_last_index", peak(rnd(), [V - 1]), pos=2)
        add("tie_in_stride", peak(rnd(), [a, b]), pos=2)
        add("tie_across_threads", peak(rnd(), sorted({lo, hi})), pos=2)
        add("tie_everywhere", torch.zeros(V), pos=2)          # every thread's best is equal, empty threads included when V < 256
        add("max_suppressed", peak(peak(rnd(), [20, 20 + (256 if V > 276 else 1)]), [7], by=5.0), pos=2)
        add("begin_suppressed_g0", peak(rnd(), [3], by=4.0), pos=1)
        add("begin_suppressed_g1", logits[-1].clone(), pos=2)
        add("in_prompt", rnd(), pos=0, n_prompt=3, cur=V - 4)
        add("eos", peak(rnd(), [eos], by=2.0), pos=3)
        add("max_new_cap", rnd(), pos=3, max_new=3)
        add("max_target_cap", rnd(), pos=HEAD_MAX_TARGET - 2, n_prompt=HEAD_MAX_TARGET - 3)
        add("finished", peak(rnd(), [11]), pos=3, finished=1, cur=4, count=2)
        n = len(rows)
        prompt = [[V - 4, V - 3, V - 2, V - 1] + [0] * (HEAD_PROMPT_STRIDE - 4) for _ in range(n)]
        return dict(V=V, eos=eos, smap=smap, rows=rows, logits=torch.stack(logits), prompt=prompt, state=st, max_target=HEAD_MAX_TARGET,
                    forced_row="max_suppressed")
    return _once(("head", V), make)


def head_forced(c):
    """The teacher-forced variant of a head case: every row is given token 12, the row `forced_row` the suppressed token 7 (-inf)."""
    return [[7 if what == c["forced_row"] else 12] * HEAD_OUT_STRIDE for what in c["rows"]]


def head_want(V, forced=False, mut=()):
    """Per row (new state, None or dict(g, token, logprob, stop)) of whisper_ops_ref.head_step."""
    def make():
        c = head_case(V)
        f = head_forced(c) if forced else None
        out = []
        for u, s in enumerate(c["state"]):
            state = {k: s[k] for k in ("cur", "pos", "count", "finished")}
            out.append(OR.head_step(c["logits"][u], c["smap"], c["prompt"][u], s["n_prompt"], s["max_new"], None if f is None else f[u], state,
                                    c["eos"], c["max_target"], mut))
        return out
    return _once(("head_want", V, forced, tuple(mut)), make)


# ---- embed ----------------------------------------------------------------------------------------------------------------------------
EMBED_D = (64, 300, 1280)  # below, across and several times the 256-thread stride


def embed_inputs(d):
    def make():
        g = _gen(7, d)
        vocab, max_pos, n = 51, 37, 9
        return dict(tok=torch.randn(vocab, d, generator=g), pos_table=torch.randn(max_pos, d, generator=g) * 1.5,
                    cur=torch.tensor([0, vocab - 1, 5, 5, 17, 50, 1, 2, 3], dtype=torch.int32),
                    pos=torch.tensor([0, max_pos - 1, 5, 6, 0, 36, 1, 2, 3], dtype=torch.int32), n=n)
    return _once(("embed", d), make)
