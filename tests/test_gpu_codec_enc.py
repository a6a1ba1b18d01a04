"""GPU: the EnCodec encoder (csrc/codec_kernels.hpp behind vx_codec_encode / vx_op_codec_conv_strided / vx_op_codec_rvq_encode)
against the fp64 restatement of tests/encodec_enc_ref.py.

* op level against fp64, outputs pre-filled with NaN: the strided convolution at the four encoder shapes (and two narrow ones),
  single and ragged segments including lengths 1, r - 1, r, r + 1; the first convolution; the LSTM with the encoder's weights;
* the whole encoder's embeddings at L = 1, 321, 2240, 72000 (3 s) and 240960 (753 frames);
  tolerance as for the decoder (encodec_ref.TOL_FACTOR = 4): 4 x the fp32 floor, the floor being the same restatement run in
  torch fp32 on the CPU against fp64 on the same inputs;
* the quantiser's search on fp64-rounded embeddings and the whole encoder's codes by the margin rule of
  encodec_enc_ref.decided / compare_codes: every decided (frame, stage) whose earlier stages agree matches exactly (the
  decided share >= 0.98 per stage is asserted on the CPU from fp64 alone); exact ties with duplicated codebook rows: first index;
* a ragged batch against each utterance alone (bitwise), two identical calls (bitwise), a batch of several utterance groups,
  fewer codebooks, an encode on a side stream;
* AudioTokenizer.encode -> VALLE.inference -> AudioTokenizer.decode.

Every comparison prints its figures before it asserts."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import encodec_enc_ref as E
import encodec_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 3


def _lib():
    import __graft_entry__ as ge

    ge.build()
    from valle_amd import engine

    return engine.load_library(), engine


def _segs(lens):
    s = [0]
    for n in lens:
        s.append(s[-1] + n)
    return (C.c_int32 * len(s))(*s), s


def _report(what, got, ref64, ref32):
    assert not torch.isnan(got).any(), f"{what}: NaN sentinel left in the output"
    floor = float((ref32.double() - ref64).abs().max())
    err = float((got.double().cpu() - ref64).abs().max())
    scale = float(ref64.abs().max())
    print(f"{what}: scale {scale:.4g} floor {floor:.3e} engine {err:.3e} ratio {err / max(floor, 1e-300):.2f}")
    assert err <= R.tolerance(floor), f"{what}: {err:.3e} > {R.TOL_FACTOR} x floor {floor:.3e} (scale {scale:.4g})"


def _rows_conv(x, lens, w, b, stride, elu, dtype):
    """Per-segment encoder convolution on time-major rows (rows, C) -> (sum ceil(len / stride), O)."""
    outs, o = [], 0
    for n in lens:
        seg = x[o:o + n].to(dtype).T
        outs.append(E.enc_conv(F.elu(seg) if elu else seg, w.to(dtype), b.to(dtype), stride).T)
        o += n
    return torch.cat(outs)


def _run_conv(x, lens, w, b, stride, elu):
    lib, engine = _lib()
    cout, cin, k = w.shape
    rows_out = sum(-(-n // stride) for n in lens)
    out = torch.full((rows_out, cout), float("nan"), device=DEV)
    seg, _ = _segs(lens)
    xd = x.to(DEV)
    engine._check(lib.vx_op_codec_conv_strided(xd.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), cin, cout, k, stride, elu,
                                               len(lens), seg, None))
    return out


# (c_in, stride): c_out = 2 c_in, k = 2 stride.  The four encoder shapes, then two narrow-geometry ones (scalar operand loads).
STRIDED_SHAPES = [(32, 2), (64, 4), (128, 5), (256, 8), (4, 2), (32, 8)]


@pytest.mark.parametrize("segs", ["one", "ragged", "short"])
@pytest.mark.parametrize("shape", STRIDED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_conv_strided(shape, segs):
    cin, r = shape
    lens = {"one": [37 * r + 3], "ragged": [1, max(1, r - 1), r, r + 1, 21 * r + 2, 2 * r, 1], "short": [r + 1]}[segs]
    g = torch.Generator().manual_seed(cin * 131 + r)
    x = torch.randn(sum(lens), cin, generator=g) * 1.5
    w = torch.randn(2 * cin, cin, 2 * r, generator=g) / (cin * 2 * r) ** 0.5
    b = torch.randn(2 * cin, generator=g) * 0.1
    out = _run_conv(x, lens, w, b, r, 1)
    _report(f"strided conv {shape} {lens}", out, _rows_conv(x, lens, w, b, r, 1, torch.float64), _rows_conv(x, lens, w, b, r, 1, torch.float32))


@pytest.mark.parametrize("lens", [[300], [1, 5, 6, 7, 8, 2, 333]], ids=lambda s: "segs" + "_".join(map(str, s)))
@pytest.mark.parametrize("cout", [32, 4])
def test_op_first_conv(cout, lens):
    g = torch.Generator().manual_seed(cout + len(lens))
    x = torch.randn(sum(lens), 1, generator=g) * 0.3
    w = torch.randn(cout, 1, 7, generator=g) * (6.0 / 7 ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    out = _run_conv(x, lens, w, b, 1, 0)
    _report(f"first conv {cout} {lens}", out, _rows_conv(x, lens, w, b, 1, 0, torch.float64), _rows_conv(x, lens, w, b, 1, 0, torch.float32))


@pytest.mark.parametrize("lens", [[225], [1, 7, 76, 2]], ids=lambda s: "segs" + "_".join(map(str, s)))
def test_op_lstm_with_encoder_weights(lens):
    """The decoder's step kernel on the encoder's weights and on the encoder's own LSTM input (the restatement's last stage)."""
    lib, engine = _lib()
    sd = E.make_enc_weights(E.FULL, SEED)
    P = {k[len("encoder.layers.13.lstm."):]: v for k, v in sd.items() if k.startswith("encoder.layers.13.lstm.")}
    xs = []
    for i, n in enumerate(lens):
        taps = {}
        E.encode_embeddings(sd, E.FULL, E.make_wave(n * 320 - (i % 2) * 100, 30 + i), taps=taps)
        xs.append(taps["stage3"].float())
    x = torch.cat(xs)
    assert x.shape == (sum(lens), 512)
    y = torch.full((sum(lens), 512), float("nan"), device=DEV)
    seg, _ = _segs(lens)
    arr = lambda n: (C.c_void_p * 2)(*[P[f"{n}_l{l}"].data_ptr() for l in range(2)])
    xd = x.to(DEV)
    engine._check(lib.vx_op_codec_lstm(xd.data_ptr(), arr("weight_ih"), arr("weight_hh"), arr("bias_ih"), arr("bias_hh"), y.data_ptr(),
                                       512, 2, len(lens), seg, None))

    def ref(dtype):
        Pd = {k: v.to(dtype) for k, v in P.items()}
        outs, o = [], 0
        for n in lens:
            s = x[o:o + n].to(dtype)
            outs.append(R.lstm(s, Pd, "", 2) + s)
            o += n
        return torch.cat(outs)

    _report(f"encoder lstm {lens}", y, ref(torch.float64), ref(torch.float32))


# ---- the quantiser's search ----------------------------------------------------------------------------------------------------
def _rvq_op(emb32, cbs32):
    lib, engine = _lib()
    n_q, (S, D) = len(cbs32), cbs32[0].shape
    cb = torch.stack(cbs32).contiguous()
    out = torch.full((n_q, emb32.shape[0]), -1, dtype=torch.int32, device=DEV)
    ed = emb32.contiguous().to(DEV)
    engine._check(lib.vx_op_codec_rvq_encode(ed.data_ptr(), cb.data_ptr(), out.data_ptr(), emb32.shape[0], n_q, S, D, None))
    return out.cpu().long()


def _check_codes(what, got, emb64, cbs64, tol):
    want, dec = E.decided(cbs64, emb64, tol)
    assert got.shape == want.shape and got.dtype == torch.int64
    assert int(got.min()) >= 0 and int(got.max()) < cbs64[0].shape[0]
    wrong, held, loose = E.compare_codes(got, want, dec)
    print(f"{what}: codes {got.numel()} equal {int((got == want).sum())} held share per stage {[round(h, 4) for h in held]} "
          f"held-and-wrong {wrong} undecided-and-different {loose}")
    assert wrong == 0, f"{what}: {wrong} decided codes differ from fp64"
    return held


@pytest.mark.parametrize("L", [72000, 240960])
def test_op_rvq_encode_on_fp64_rounded_embeddings(L):
    sd = E.make_enc_weights(E.FULL, SEED)
    emb, floor, _ = E.embedding_floor(sd, E.FULL, E.make_wave(L, 5))
    cbs = E.codebooks(sd, E.FULL, 8)
    got = _rvq_op(emb.float(), [c.float() for c in cbs])
    held = _check_codes(f"rvq op L={L}", got, emb, cbs, R.tolerance(floor))
    assert min(held) >= 0.98


def test_op_rvq_encode_narrow_shape_and_row_tail():
    """64 x 16 codebooks (two 32-code tiles for four waves: two waves idle) and 45 rows (a partial workgroup)."""
    sd = E.make_enc_weights(E.NARROW, SEED)
    emb, floor, _ = E.embedding_floor(sd, E.NARROW, E.make_wave(45 * 320, 6))
    cbs = E.codebooks(sd, E.NARROW, 8)
    got = _rvq_op(emb.float(), [c.float() for c in cbs])
    _check_codes("rvq op narrow", got, emb, cbs, R.tolerance(floor))


def _tied_codebook(base, offsets, S):
    """S rows out of `base`'s: walking j upwards, a free row j takes the next base row and so does every free row j + d, d in
    `offsets`.  Returns (codebook, owner: base row of every j)."""
    owner = torch.full((S,), -1, dtype=torch.long)
    u = 0
    for j in range(S):
        if owner[j] >= 0:
            continue
        owner[j] = u
        for d in offsets:
            if j + d < S and owner[j + d] < 0:
                owner[j + d] = u
        u += 1
    return base[owner].contiguous(), owner


# Where the copies of a row sit relative to it.  The kernel gives code j to wave (j / 32) % 4, lane j % 32, tile pass j / 128:
#   1, 3, 5, 17   other lanes of the same wave and pass: the shuffle reduction meets equal distances, with the smaller index on either
#                 side of every xor partner pair
#   32, 64, 96    other waves, same pass: the reduction over the four waves through LDS
#   160, 224      another pass AND another wave; with 224 (= 128 + 96) and 96 the smaller index sits in the HIGHER wave (j in wave 1,
#                 j + 96 in wave 0 of the next pass), so taking waves in order is not enough
#   512           same wave and lane, a later pass: the per-lane loop
#   (1, 33, 130, 515) four copies across lane, wave and pass at once; "random": 4 copies each at random places
TIE_OFFSETS = [(1,), (3,), (5,), (17,), (32,), (64,), (96,), (160,), (224,), (512,), (1, 33, 130, 515), "random"]


@pytest.mark.parametrize("offsets", TIE_OFFSETS, ids=lambda o: o if isinstance(o, str) else "d" + "_".join(map(str, o)))
def test_op_rvq_encode_ties_take_the_first_index(offsets):
    """Exact ties: codebook rows that are copies of each other give bitwise equal distances (same operands, same k order, same
    |e|^2) wherever they sit, and the smallest index among the copies must win, at every level of the arg-min.  The expected row
    is not taken from a matmul over the tied codebook (whose columns need not tie bitwise in a blocked product) but from the
    margin rule over the DISTINCT rows, mapped to the first copy; and that the answer is the first of ITS copies is asserted for
    every frame and stage, decided or not."""
    S, D, rows = 1024, 128, 200
    g = torch.Generator().manual_seed(11)
    base = torch.randn(S, D, generator=g)
    cbs, owners = [], []
    for stage in range(2):
        if offsets == "random":
            owner = torch.randperm(S, generator=g) % (S // 4)
            cb = base[owner].contiguous()
        else:
            cb, owner = _tied_codebook(base.flip(0) if stage else base, offsets, S)
            if stage:
                cb = cb * 0.9
        cbs.append(cb)
        owners.append(owner)
    emb = torch.randn(rows, D, generator=g) * 1.2
    got = _rvq_op(emb, cbs)
    firsts, uniq = [], []
    for cb, owner in zip(cbs, owners):
        first = torch.full((int(owner.max()) + 1,), S, dtype=torch.long)
        first.scatter_reduce_(0, owner, torch.arange(S), reduce="amin")
        assert int((torch.bincount(owner) > 1).sum()) >= S // 8  # there are ties to break
        firsts.append(first)
        uniq.append(cb[first].double())
    # every answer is the first of its copies
    for q in range(2):
        assert torch.equal(got[q], firsts[q][owners[q][got[q]]]), f"stage {q}: a later copy of a tied row was returned"
    # and it is the right row: the margin rule over the distinct rows (teacher-forced, fp32-rounded inputs: tolerance 1e-5)
    want_u, dec = E.decided(uniq, emb.double(), 1e-5)
    want = torch.stack([firsts[q][want_u[q]] for q in range(2)])
    wrong, held, _ = E.compare_codes(got, want, dec)
    print(f"ties {offsets}: held share {held} wrong {wrong}")
    assert wrong == 0 and min(held) > 0.9


def test_last_embeddings_refuses_rows_beyond_the_last_encode():
    from valle_amd.engine import VxError

    enc, _ = _codec()
    enc.encode(E.make_wave(640, 1))
    assert enc.last_embeddings(2).shape == (2, 128)
    with pytest.raises(VxError) as e:
        enc.last_embeddings(3)
    assert e.value.code == 1
    enc.decode(torch.zeros(8, 4, dtype=torch.int64))  # reuses the buffer: nothing of an encode is left to read
    with pytest.raises(VxError):
        enc.last_embeddings(1)


# ---- the whole encoder -------------------------------------------------------------------------------------------------------------
_ENC = {}


def _codec(geo=E.FULL, max_frames=768, max_batch=8):
    _lib()
    from valle_amd.codec import CodecConfig, EncodecDecoder

    key = (geo, max_frames, max_batch)
    if key not in _ENC:
        d = EncodecDecoder(CodecConfig(hidden=geo.hidden, filters=geo.filters, codebook_size=geo.codebook_size,
                                       n_codebooks=geo.n_codebooks), max_frames=max_frames, max_batch=max_batch, encoder=True)
        d.load_state_dict(E.make_enc_weights(geo, SEED), strict=True)
        _ENC[key] = d.to(DEV)
    return _ENC[key], E.make_enc_weights(geo, SEED)


@pytest.mark.parametrize("L", E.GPU_LENGTHS)
def test_encoder_embeddings_and_codes(L):
    enc, sd = _codec()
    wav = E.make_wave(L, 5)
    T = E.n_frames(E.FULL, L)
    emb, floor, scale = E.embedding_floor(sd, E.FULL, wav)
    codes = enc.encode(wav)
    assert codes.shape == (1, 8, T) and codes.dtype == torch.int64 and codes.is_cuda
    got = enc.last_embeddings(T)
    err = float((got.double().cpu() - emb).abs().max())
    print(f"encoder L={L} T={T}: scale {scale:.4g} floor {floor:.3e} ({floor / scale:.2e} rel) engine {err:.3e} ratio {err / floor:.2f}")
    assert torch.isfinite(got).all()
    assert err <= R.tolerance(floor), f"L={L}: engine {err:.3e} > {R.TOL_FACTOR} x floor {floor:.3e}"
    _check_codes(f"encode L={L}", codes[0].cpu(), emb, E.codebooks(sd, E.FULL, 8), R.tolerance(floor))


@pytest.mark.parametrize("L", [1, 319, 320, 321, 2240, 24001])
def test_encoder_narrow_geometry(L):
    enc, sd = _codec(E.NARROW, max_frames=128, max_batch=2)
    wav = E.make_wave(L, 7)
    emb, floor, scale = E.embedding_floor(sd, E.NARROW, wav)
    codes = enc.encode(wav)
    got = enc.last_embeddings(emb.shape[0])
    err = float((got.double().cpu() - emb).abs().max())
    print(f"narrow encoder L={L}: scale {scale:.4g} floor {floor:.3e} engine {err:.3e} ratio {err / floor:.2f}")
    assert err <= R.tolerance(floor)
    _check_codes(f"narrow encode L={L}", codes[0].cpu(), emb, E.codebooks(sd, E.NARROW, 8), R.tolerance(floor))


def test_fewer_codebooks():
    enc, sd = _codec()
    wav = E.make_wave(24001, 8)
    emb, floor, _ = E.embedding_floor(sd, E.FULL, wav)
    c3 = enc.encode(wav, n_q=3)
    assert c3.shape == (1, 3, 76)
    assert torch.equal(c3, enc.encode(wav)[:, :3])
    _check_codes("encode n_q=3", c3[0].cpu(), emb, E.codebooks(sd, E.FULL, 3), R.tolerance(floor))


def test_ragged_batch_equals_alone_and_repeats_bitwise():
    """311 frames in one call: more than one workgroup of rows in every kernel (32 frames in the search, 64 / 128 rows in the
    GEMMs), utterances of 1 sample, 1 sample past a frame, whole frames and a length whose every stage rounds up."""
    enc, sd = _codec()
    lens = [1, 321, 2240, 24001, 72000, 319]
    wavs = [E.make_wave(L, 40 + i) for i, L in enumerate(lens)]
    together = [c.clone() for c in enc.encode_batch(wavs)]
    emb_together = enc.last_embeddings(sum(E.n_frames(E.FULL, L) for L in lens)).clone()
    again = enc.encode_batch(wavs)
    o = 0
    for i, L in enumerate(lens):
        T = E.n_frames(E.FULL, L)
        alone = enc.encode(wavs[i])
        assert together[i].shape == (1, 8, T)
        assert torch.equal(together[i], alone), f"utterance {i} (L={L}) differs between the ragged batch and alone"
        assert torch.equal(enc.last_embeddings(T), emb_together[o:o + T]), f"utterance {i} (L={L}): embeddings differ"
        assert torch.equal(together[i], again[i]), f"utterance {i}: two identical calls differ"
        o += T
    emb, floor, _ = E.embedding_floor(sd, E.FULL, wavs[3])
    _check_codes("ragged utterance 3", together[3][0].cpu(), emb, E.codebooks(sd, E.FULL, 8), R.tolerance(floor))


def test_batch_spanning_several_groups_equals_alone():
    """The convolution stack runs over groups of whole utterances of at most max(max_frames, 8192) frames: these eight make two
    groups (6 + 2), each with its own row tables per stage and its own offset into the LSTM's input.  Every utterance must be
    bitwise its alone encode; the short one of the second group is held against fp64."""
    frames = [1505, 1400, 1, 1536, 1300, 1100, 1358, 2]
    assert sum(frames) > 8192 and sum(frames[:6]) <= 8192 < sum(frames[:7])
    enc, sd = _codec(E.FULL, max_frames=1536, max_batch=8)
    lens = [T * 320 - (37 * i) % 300 for i, T in enumerate(frames)]
    assert [E.n_frames(E.FULL, L) for L in lens] == frames
    wavs = [E.make_wave(L, 60 + i) for i, L in enumerate(lens)]
    together = [c.clone() for c in enc.encode_batch(wavs)]
    for i in range(len(lens)):
        assert torch.equal(together[i], enc.encode(wavs[i])), f"utterance {i} differs between the multi-group batch and alone"
    emb, floor, _ = E.embedding_floor(sd, E.FULL, wavs[7])
    _check_codes("second group's short utterance", together[7][0].cpu(), emb, E.codebooks(sd, E.FULL, 8), R.tolerance(floor))


def test_encode_follows_the_callers_stream():
    enc, _ = _codec()
    wav = E.make_wave(24000, 9).to(DEV)
    want = enc.encode(wav).cpu()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        junk = torch.randn(4096, 4096, device=DEV) @ torch.randn(4096, 4096, device=DEV)
        w2 = wav * 1.0  # produced on the side stream right before the encode reads it
        got = enc.encode(w2)
        host = got.to("cpu", non_blocking=False)
    side.synchronize()
    assert torch.equal(host, want) and torch.isfinite(junk).all()


def test_prompt_to_waveform_round_trip():
    """tokenize_audio -> inference -> decode as the reference's infer.py chains them: AudioTokenizer.encode((1, 1, L)) ->
    [(codes (1, 8, T), None)], inference(y=codes.transpose(2, 1)), decode([(frames.transpose(2, 1), None)])."""
    _lib()
    from valle_amd.codec import AudioTokenizer
    from valle_amd.config import ModelConfig
    from valle_amd.models import VALLE
    from valle_amd.weights import synthetic_inputs, synthetic_state_dict

    enc, sd = _codec()
    tok = AudioTokenizer(enc)
    wav = E.make_wave(72000, 5)
    encoded = tok.encode(wav.to(DEV))
    assert isinstance(encoded, list) and len(encoded) == 1 and encoded[0][1] is None
    codes = encoded[0][0]
    assert codes.shape == (1, 8, 225) and codes.dtype == torch.int64 and codes.is_cuda
    emb, floor, _ = E.embedding_floor(sd, E.FULL, wav)
    _check_codes("round trip prompt", codes[0].cpu(), emb, E.codebooks(sd, E.FULL, 8), R.tolerance(floor))

    cfg = ModelConfig(decoder_dim=256, nhead=4, num_decoder_layers=4, prefix_mode=1)
    x, x_lens, _ = synthetic_inputs(4, 30)
    m = VALLE(256, 4, 4, prefix_mode=1, precision="fp32", max_text=64, max_audio=512, print_eos=False)
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    m.to(DEV).eval()
    y = codes.transpose(2, 1)  # (1, T, 8), as infer.py passes audio_prompts
    frames = m.inference(x.to(DEV), x_lens.to(DEV), y, None, top_k=1)
    assert frames.dim() == 3 and frames.shape[0] == 1 and frames.shape[2] == 8 and frames.dtype == torch.int64
    out = tok.decode([(frames.transpose(2, 1), None)])
    assert out.shape == (1, 1, 320 * frames.shape[1]) and out.dtype == torch.float32 and out.is_cuda
    assert torch.isfinite(out).all()
