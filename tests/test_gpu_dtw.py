"""GPU: dynamic time warping (dtw_kernels.hpp behind vx_dtw_compare, valle_amd.dtw) against the restatement of tests/dtw_ref.py.

1. the warp is exact: vx_op_dtw_path on caller matrices gives the reference's total bit for bit and its path cell for cell, on
   shapes that straddle the 256 cells a workgroup takes of a diagonal per step, with random costs, costs 0..2 (ties everywhere:
   the tie rule decides) and a constant; ten matrices in one launch equal each alone;
2. cepstra and local cost (vx_op_dtw_cost) against fp64.  Floor: the same chain in numpy fp32.  Bound: engine error <= 4 x
   floor (dtw_ref.TOL_FACTOR, the project's rule) for every configuration and shape; every ratio is printed before it is
   asserted.  Identical rows cost exactly 0.0.  Measured: ratios 0.19 .. 1.00;
3. end to end (DTW.compare_batch): |total - total_ref64| <= (Ta + Tb - 1) x 4 x floor of the pair (a path has at most that many
   cells, so the optimum moves by at most that many times the largest local-cost error); the exact cases B = A and B = A's rows
   doubled; every returned path is a path and re-sums, in fp64 over the kernel's own cost matrix, to `total` exactly;
4. a ragged batch at odd pointer offsets equals each pair alone bitwise, repeats bitwise, follows the caller's stream, writes
   nothing outside its outputs, and a larger call after a small one (the workspace grows) gives the shared pair the same bits;
5. mel_cepstral_distortion is the hand-composed chain, with sr= resample-then-chain; mel_distance(warp=True)."""
import numpy as np
import pytest
import torch

import dtw_ref as DR
import fbank_ref as FR
import resample_ref as RR
from valle_amd import engine as E
from valle_amd.dtw import DTW, MCD_DB, mel_cepstral_distortion
from valle_amd.fbank import mel_distance

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATH_SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 300), (300, 3), (255, 257), (256, 256), (257, 255), (513, 700))
COST_SHAPES = ((1, 1), (33, 65), (255, 257))
E2E_SHAPES = ((1, 1), (40, 55), (255, 257), (700, 513))
_CACHE = {}


def _build():
    import __graft_entry__ as ge

    ge.build()


def _dtw(key=(100, 13)):
    _build()
    if key not in _CACHE:
        _CACHE[key] = DTW(key[0], key[1], max_batch=8).to(DEV)
    return _CACHE[key]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


# ---- 1. the warp ---------------------------------------------------------------------------------------------------------------
def _path_case(kind):
    """The ten matrices of a kind and their reference results, computed once."""
    if ("path", kind) not in _CACHE:
        g = np.random.default_rng({"random": 11, "ties": 12, "constant": 13}[kind])
        mats = []
        for Ta, Tb in PATH_SHAPES:
            if kind == "random":
                c = g.random((Ta, Tb), dtype=np.float32) * 3.0
            elif kind == "ties":
                c = g.integers(0, 3, (Ta, Tb)).astype(np.float32)
            else:
                c = np.full((Ta, Tb), 0.75, dtype=np.float32)
            mats.append(c)
        _CACHE[("path", kind)] = (mats, [DR.warp(c) for c in mats])
    return _CACHE[("path", kind)]


@pytest.mark.parametrize("kind", ("random", "ties", "constant"))
def test_warp_is_exact(kind):
    _build()
    mats, refs = _path_case(kind)
    flat = _dev(np.concatenate([np.full(3, np.nan, np.float32)] + [c.reshape(-1) for c in mats]))  # the matrices start 3 floats in
    desc, off = [], 3
    for c in mats:
        desc.append((c.shape[0], c.shape[1], off))
        off += c.size
    total, length, paths = E.op_dtw_path(flat, desc)
    total, length = total.cpu().numpy(), length.cpu().numpy()
    for z, ((Ta, Tb), (t_ref, p_ref)) in enumerate(zip(PATH_SHAPES, refs)):
        assert _bits(total[z]) == _bits(t_ref), f"{kind} {Ta}x{Tb}: total {total[z]!r} != {t_ref!r}"
        assert int(length[z]) == len(p_ref) and np.array_equal(paths[z].cpu().numpy(), p_ref), f"{kind} {Ta}x{Tb}: path differs"
        t1, l1, p1 = E.op_dtw_path(_dev(mats[z].reshape(-1)), [(Ta, Tb, 0)])
        assert _bits(t1.cpu().numpy()[0]) == _bits(total[z]) and int(l1[0]) == int(length[z]) and torch.equal(p1[0], paths[z]), \
            f"{kind} {Ta}x{Tb}: alone differs from the launch of ten"
    t2, l2, none = E.op_dtw_path(flat, desc, want_path=False)  # without a path: the same totals and lengths
    assert none is None and np.array_equal(_bits(t2.cpu().numpy()), _bits(total)) and np.array_equal(l2.cpu().numpy(), length)


def test_warp_with_more_than_64_kb_of_diagonals():
    """Ta above 2730 frames: the three diagonals exceed the 64 KB a launch gets without asking (another branch of the launcher)."""
    _build()
    g = np.random.default_rng(14)
    mats = [g.random((Ta, Tb), dtype=np.float32) for Ta, Tb in ((2800, 5), (4096, 3), (2, 4096))]
    desc, off = [], 0
    for c in mats:
        desc.append((c.shape[0], c.shape[1], off))
        off += c.size
    total, length, paths = E.op_dtw_path(_dev(np.concatenate([c.reshape(-1) for c in mats])), desc)
    for z, c in enumerate(mats):
        t_ref, p_ref = DR.warp(c)
        assert _bits(total.cpu().numpy()[z]) == _bits(t_ref) and np.array_equal(paths[z].cpu().numpy(), p_ref), c.shape


# ---- 2. cepstra and local cost -------------------------------------------------------------------------------------------------
def _cost_inputs(D, Ta, Tb):
    A, B = DR.make_feats(Ta, D, 100 * D + Ta), DR.make_feats(Tb, D, 100 * D + Tb + 5000)
    same = [] if Ta * Tb == 1 else [(0, 0), (Ta - 1, Tb - 2), (Ta // 2, 3)]  # identical rows (not in the matrix of one cell)
    for i, j in same:
        B[j] = A[i]
    return A, B, same


@pytest.mark.parametrize("D,n_ceps", ((100, 13), (100, 0), (5, 4)))
def test_cost_against_fp64(D, n_ceps):
    _build()
    failures = []
    for Ta, Tb in COST_SHAPES:
        A, B, same = _cost_inputs(D, Ta, Tb)
        ref64 = DR.chain(A, B, n_ceps)[0]
        ref32 = DR.chain(A, B, n_ceps, np.float32)[0]
        got = E.op_dtw_cost(_dev(A), _dev(B), n_ceps).cpu().numpy()
        assert got.shape == (Ta, Tb) and got.dtype == np.float32 and np.isfinite(got).all()
        for i, j in same:
            assert got[i, j] == 0.0 and ref64[i, j] == 0.0, f"identical rows ({i}, {j}) cost {got[i, j]!r}"
        floor = float(np.abs(ref32.astype(np.float64) - ref64).max())
        err = float(np.abs(got.astype(np.float64) - ref64).max())
        print(f"dtw cost D={D} n_ceps={n_ceps} {Ta}x{Tb}: max cost {ref64.max():.2f} floor {floor:.3e} engine {err:.3e} "
              f"ratio {err / max(floor, 1e-300):.2f}")
        if not err <= DR.tolerance(floor):
            failures.append(f"{Ta}x{Tb}: engine {err:.3e} > {DR.TOL_FACTOR} x floor {floor:.3e}")
    assert not failures, failures


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------
def _e2e_pairs():
    if "e2e" not in _CACHE:
        pairs = [(DR.make_feats(Ta, 100, 7 * Ta + 1), DR.make_feats(Tb, 100, 7 * Tb + 2)) for Ta, Tb in E2E_SHAPES]
        refs = []
        for A, B in pairs:
            c64, t64, _ = DR.chain(A, B, 13)
            c32 = DR.chain(A, B, 13, np.float32)[0]
            refs.append((t64, float(np.abs(c32.astype(np.float64) - c64).max())))
        _CACHE["e2e"] = (pairs, refs)
    return _CACHE["e2e"]


def _check_path(res, A, B, n_ceps):
    """The path is one, and re-sums over the kernel's own cost matrix to the total."""
    Ta, Tb = A.shape[0], B.shape[0]
    path = res.path.cpu().numpy()
    assert res.path.dtype == torch.int32 and res.path.device.type == "cuda" and res.length == path.shape[0]
    assert DR.path_is_valid(path, Ta, Tb), f"{Ta}x{Tb}: not a path"
    cost = E.op_dtw_cost(A, B, n_ceps).cpu().numpy()
    assert _bits(DR.path_sum(cost, path)) == _bits(res.total), f"{Ta}x{Tb}: the path sums to {DR.path_sum(cost, path)!r}, total {res.total!r}"
    assert res.mean == res.total / res.length


def test_end_to_end_against_fp64():
    dtw = _dtw()
    pairs, refs = _e2e_pairs()
    dev = [(_dev(A), _dev(B)) for A, B in pairs]
    res = dtw.compare_batch(dev, return_path=True)
    plain = dtw.compare_batch(dev)
    failures = []
    for (Ta, Tb), (A, B), r, q, (t64, floor) in zip(E2E_SHAPES, dev, res, plain, refs):
        bound = (Ta + Tb - 1) * DR.TOL_FACTOR * floor
        print(f"dtw e2e {Ta}x{Tb}: total {r.total:.6f} ref {t64:.6f} diff {abs(r.total - t64):.3e} floor {floor:.3e} bound {bound:.3e} "
              f"len {r.length} mcd {r.mcd_db:.3f} dB")
        if not abs(r.total - t64) <= bound:
            failures.append(f"{Ta}x{Tb}: |total - ref| {abs(r.total - t64):.3e} > {bound:.3e}")
        _check_path(r, A, B, 13)
        assert q.path is None and _bits(q.total) == _bits(r.total) and q.length == r.length
        assert r.mcd_db == MCD_DB * r.mean and max(Ta, Tb) <= r.length <= Ta + Tb - 1
    assert not failures, failures


@pytest.mark.parametrize("n_ceps", (13, 0))
def test_exact_cases(n_ceps):
    dtw = _dtw((100, n_ceps))
    A = _dev(DR.make_feats(300, 100, 9))
    B2 = A.repeat_interleave(2, dim=0)
    same, doubled, flipped = dtw.compare_batch([(A, A.clone()), (A, B2), (B2, A)], return_path=True)
    k = torch.arange(300, dtype=torch.int32, device=DEV)
    assert same.total == 0.0 and same.length == 300 and torch.equal(same.path, torch.stack([k, k], 1))
    k = torch.arange(600, dtype=torch.int32, device=DEV)
    assert doubled.total == 0.0 and doubled.length == 600 and torch.equal(doubled.path, torch.stack([k // 2, k], 1))
    assert flipped.total == 0.0 and flipped.length == 600
    for r, (a, b) in ((same, (A, A)), (doubled, (A, B2)), (flipped, (B2, A))):
        _check_path(r, a, b, n_ceps)
        assert (r.mcd_db == 0.0) if n_ceps else (r.mcd_db is None)
    # more pairs than max_batch: served in several calls
    small = DTW(100, n_ceps, max_frames=600, max_batch=2).to(DEV)
    many = small.compare_batch([(A, B2)] * 5)
    assert len(many) == 5 and all(m.total == 0.0 and m.length == 600 for m in many)
    with pytest.raises(E.VxError) as e:
        small.compare(A, torch.cat([B2, A]))
    assert e.value.code == 4
    small.close()


# ---- 4. ragged batch and isolation ---------------------------------------------------------------------------------------------
def _raw_call(dtw, pairs, fill=float("nan")):
    """vx_dtw_compare on features that start one float past a 16-byte boundary inside buffers of `fill`, into results and paths
    inside guarded buffers.  -> (totals bits, lengths, paths) after checking that nothing around the outputs changed."""
    n = len(pairs)
    ins = []
    for A, B in pairs:
        for x in (A, B):
            buf = torch.full((x.size + 9,), fill, device=DEV)
            buf[5:5 + x.size] = _dev(x.reshape(-1))
            ins.append(buf)
    total = torch.full((n + 4,), float("nan"), dtype=torch.float64, device=DEV)
    length = torch.full((n + 4,), -7, dtype=torch.int32, device=DEV)
    caps = [A.shape[0] + B.shape[0] - 1 for A, B in pairs]
    paths = [torch.full((2 * cap + 6,), -7, dtype=torch.int32, device=DEV) for cap in caps]
    dtw._compare_raw([ins[2 * i].data_ptr() + 20 for i in range(n)], [A.shape[0] for A, _ in pairs],
                     [ins[2 * i + 1].data_ptr() + 20 for i in range(n)], [B.shape[0] for _, B in pairs],
                     total.data_ptr() + 16, length.data_ptr() + 8, [p.data_ptr() + 12 for p in paths])
    torch.cuda.synchronize()
    assert bool(torch.isnan(total[:2]).all()) and bool(torch.isnan(total[2 + n:]).all()), "written around the totals"
    assert bool((length[:2] == -7).all()) and bool((length[2 + n:] == -7).all()), "written around the lengths"
    lens = length[2:2 + n].tolist()
    out = []
    for p, cap, ln in zip(paths, caps, lens):
        assert bool((p[:3] == -7).all()) and bool((p[3 + 2 * cap:] == -7).all()), "written around a path"
        out.append(p[3:3 + 2 * ln].reshape(ln, 2).clone())
    for buf, x in zip(ins, [x for pr in pairs for x in pr]):
        edge = torch.cat([buf[:5], buf[5 + x.size:]])
        assert bool(torch.isnan(edge).all()) if fill != fill else bool((edge == fill).all()), "an input's surroundings changed"
    return total[2:2 + n].cpu().numpy().view(np.int64), lens, out


def test_ragged_batch_equals_alone_repeats_and_stays_inside_its_outputs():
    dtw = _dtw()
    pairs, refs = _e2e_pairs()
    t0, l0, p0 = _raw_call(dtw, pairs)
    t1, l1, p1 = _raw_call(dtw, pairs, fill=0.0)  # what surrounds the inputs does not matter, and two calls agree
    assert np.array_equal(t0, t1) and l0 == l1 and all(torch.equal(a, b) for a, b in zip(p0, p1))
    for i, (A, B) in enumerate(pairs):
        alone = dtw.compare(_dev(A), _dev(B), return_path=True)
        assert _bits(alone.total) == t0[i] and alone.length == l0[i] and torch.equal(alone.path, p0[i]), f"pair {i} differs alone"
        assert np.isfinite(alone.total) and abs(alone.total - refs[i][0]) <= (A.shape[0] + B.shape[0] - 1) * DR.TOL_FACTOR * refs[i][1]
    # the batch in another order: a pair's bits do not depend on its place in the launch
    t2, l2, p2 = _raw_call(dtw, pairs[::-1])
    assert np.array_equal(t2[::-1], t0) and l2[::-1] == l0 and all(torch.equal(a, b) for a, b in zip(p2[::-1], p0))


def test_workspace_grows_with_the_call():
    _build()
    pairs, _ = _e2e_pairs()
    dev = [(_dev(A), _dev(B)) for A, B in pairs]
    dtw = DTW(100, 13, max_batch=4).to(DEV)
    small = dtw.compare(*dev[1], return_path=True)            # 40 x 55 cells
    big = dtw.compare_batch(dev, return_path=True)            # 700 x 513 and the others: a larger workspace
    again = dtw.compare(*dev[1], return_path=True)
    for r in (big[1], again):
        assert _bits(r.total) == _bits(small.total) and r.length == small.length and torch.equal(r.path, small.path)
    want = _dtw().compare_batch(dev)
    assert [_bits(r.total) for r in big] == [_bits(r.total) for r in want]
    dtw.close()


def test_follows_the_callers_stream():
    dtw = _dtw()
    A, B = _dev(DR.make_feats(700, 100, 21)), _dev(DR.make_feats(650, 100, 22))
    want = dtw.compare(A, B, return_path=True)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        junk = torch.randn(4096, 4096, device=DEV) @ torch.randn(4096, 4096, device=DEV)
        A2, B2 = A * 1.0, B * 1.0  # produced on the side stream right before the call reads them
        got = dtw.compare(A2, B2, return_path=True)
        path = got.path.to("cpu")
    side.synchronize()
    assert _bits(got.total) == _bits(want.total) and torch.equal(path, want.path.cpu()) and torch.isfinite(junk).all()


# ---- 5. the Python chain -------------------------------------------------------------------------------------------------------
def test_mel_cepstral_distortion_is_the_hand_composed_chain():
    _build()
    from valle_amd.codec import Resampler
    from valle_amd.fbank import BigVGANFbank

    fb = BigVGANFbank(max_batch=8).to(DEV)
    wa, wb = FR.make_noise(24000, 31, 0.3).to(DEV), FR.make_noise(26000, 32, 0.3).to(DEV)
    ma, mb = fb.extract_batch([wa, wb])
    want = _dtw().compare(ma, mb)
    got = mel_cepstral_distortion(wa, wb)
    assert (got.total, got.length, got.mean, got.mcd_db) == (want.total, want.length, want.mean, want.mcd_db) and got.path is None
    assert got.total > 0 and got.mcd_db == MCD_DB * got.total / got.length and 102 <= got.length <= 94 + 102 - 1
    both = mel_cepstral_distortion([wa, wb], [wb, wb])
    assert isinstance(both, list) and both[0].total == want.total and both[1].total == 0.0 and both[1].length == 102
    seven = mel_cepstral_distortion(wa, wb, n_ceps=7)
    assert seven.total == DTW(100, 7).to(DEV).compare(ma, mb).total and seven.total < got.total
    # stereo at 48 kHz: mixed down and resampled first
    sa, sb = (RR.make_noise(48000, 33, channels=2) * 0.1).to(DEV), (RR.make_noise(50000, 34, channels=2) * 0.1).to(DEV)
    rs = Resampler(48000, 24000).to(DEV)
    m2a, m2b = fb.extract_batch([rs(sa), rs(sb)])
    want2 = _dtw().compare(m2a, m2b)
    got2 = mel_cepstral_distortion(sa, sb, sr=48000)
    assert (got2.total, got2.length) == (want2.total, want2.length) and got2.total > 0
    with pytest.raises(ValueError):
        mel_cepstral_distortion(wa, wb[:100])


def test_mel_distance_along_the_warp():
    _build()
    from valle_amd.fbank import BigVGANFbank

    a = BigVGANFbank().to(DEV).extract_batch([FR.make_noise(24000, 41, 0.3).to(DEV)])[0]
    b = a.repeat_interleave(2, dim=0)
    d = mel_distance(a, a.clone(), warp=True)
    assert d.dim() == 0 and d.device.type == "cuda" and float(d) == 0.0
    assert float(mel_distance(a, b, warp=True)) == 0.0 and float(mel_distance(a, b)) > 0.1
    c = BigVGANFbank().to(DEV).extract_batch([FR.make_noise(30000, 42, 0.3).to(DEV)])[0]
    path = DTW(100, 0).to(DEV).compare(a, c, return_path=True).path.long()
    assert torch.equal(mel_distance(a, c, warp=True), (a[path[:, 0]] - c[path[:, 1]]).abs().mean())
    assert torch.equal(mel_distance(a, c), (a - c[:a.shape[0]]).abs().mean())  # the default is what it was
