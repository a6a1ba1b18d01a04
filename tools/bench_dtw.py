"""Dynamic-time-warping time at (pairs, seconds A, seconds B) = (1, 3, 3), (1, 10, 11), (32, 10, 10), (64, 20, 20), at 13 cepstra
and at the raw 100 mels: `DTW.compare_batch` (cepstra, cost and warp kernels, device features in, totals and lengths on the host)
against (a) the same definition on stock torch GPU ops - cepstra by matmul, the local cost by `torch.cdist` on differences pair
by pair, the recurrence in fp64 one anti-diagonal per step over the stacked pairs (totals only: no back-pointers, no path) - and
(b) the host restatement of tests/dtw_ref.py (numpy fp64, one pair timed, path included).  Plus the error ratios of the parity
test's inputs.  One JSON line on stdout, the same object written to --out.

    python tools/bench_dtw.py [--reps 5] [--points 1x3x3,1x10x11,32x10x10,64x20x20] [--out profiles/dtw_times.json]
    python tools/bench_dtw.py --only-hip --points 64x20x20 --reps 20      # the run to put under a kernel tracer

Each point is warmed once per implementation, then the implementations alternate rep by rep.  A rep runs the call `inner` times
back to back (chosen per implementation so that a rep lasts about 20 ms or more) and ends in a device synchronise; the figure is
the median over the reps of the rep's wall time / inner.  The features are Gaussian log-mel-like rows, not audio."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", default="1x3x3,1x10x11,32x10x10,64x20x20", help="PAIRSxSECONDS_AxSECONDS_B,...")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_times.json"))
    ap.add_argument("--only-hip", action="store_true", help="time the HIP call alone (for a kernel trace); writes no file")
    args = ap.parse_args()
    import numpy as np
    import torch

    import __graft_entry__ as ge

    ge.build()
    import dtw_ref as DR
    import fbank_ref as FR
    from valle_amd import engine as E
    from valle_amd.dtw import DIAG_CHUNK, DTW

    if not torch.cuda.is_available():
        raise SystemExit("bench_dtw.py measures on the GPU; none found")
    dev = "cuda:0"
    points = [tuple(int(v) for v in p.split("x")) for p in args.points.split(",")]
    sync = torch.cuda.synchronize

    @torch.no_grad()
    def torch_cost(A, B, tab):
        """A (P, Ta, D), B (P, Tb, D) -> (P, Ta, Tb) fp32, on differences (one cdist call per pair)."""
        if tab is not None:
            A, B = A @ tab, B @ tab
        return torch.stack([torch.cdist(a, b, p=2.0, compute_mode="donot_use_mm_for_euclid_dist") for a, b in zip(A, B)])

    @torch.no_grad()
    def torch_warp(cost):
        """cost (P, Ta, Tb) -> totals (P,) fp64: G over a frame of +inf, one anti-diagonal of all pairs per step."""
        P, Ta, Tb = cost.shape
        G = torch.full((P, Ta + 1, Tb + 1), float("inf"), dtype=torch.float64, device=cost.device)
        c = cost.double()
        G[:, 1, 1] = c[:, 0, 0]
        rows = torch.arange(Ta, device=cost.device)
        for d in range(1, Ta + Tb - 1):
            i = rows[max(0, d - (Tb - 1)):min(d, Ta - 1) + 1]
            j = d - i
            best = torch.minimum(torch.minimum(G[:, i, j], G[:, i, j + 1]), G[:, i + 1, j])
            G[:, i + 1, j + 1] = best + c[:, i, j]
        return G[:, Ta, Tb]

    def timed(fn, inner):
        sync()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        return (time.perf_counter() - t0) / inner

    out = {"bench": "dtw", "reps": args.reps, "diag_chunk": DIAG_CHUNK, "workspace_bytes_per_cell": 5, "points": []}
    for n_ceps in (13, 0):
        dtw = DTW(100, n_ceps).to(dev)
        tab = torch.from_numpy(DR.dct_table(100, n_ceps)).to(dev) if n_ceps else None
        for P, sa, sb in points:
            Ta, Tb = FR.n_frames(24000 * sa), FR.n_frames(24000 * sb)
            feats = [(DR.make_feats(Ta, 100, 2 * p), DR.make_feats(Tb, 100, 2 * p + 1)) for p in range(P)]
            pairs = [(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)) for a, b in feats]
            A, B = torch.stack([a for a, _ in pairs]), torch.stack([b for _, b in pairs])
            row = {"pairs": P, "seconds": [sa, sb], "frames": [Ta, Tb], "n_ceps": n_ceps, "cells": P * Ta * Tb}
            impls = {"hip": lambda: dtw.compare_batch(pairs)}
            if not args.only_hip:
                held = {}

                def t_cost():
                    held["cost"] = torch_cost(A, B, tab)

                impls["torch_gpu_cost"] = t_cost
                impls["torch_gpu_warp"] = lambda: torch_warp(held["cost"])
                ours = dtw.compare_batch(pairs)
                t_cost()
                theirs = torch_warp(held["cost"]).tolist()
                row["totals_pair0"] = {"hip": ours[0].total, "torch_gpu": theirs[0]}
                row["hip_vs_torch_gpu_max_rel_diff"] = max(abs(r.total - t) / max(abs(t), 1e-300) for r, t in zip(ours, theirs))
                hip_cost = E.op_dtw_cost(pairs[-1][0], pairs[-1][1], n_ceps)
                row["hip_vs_torch_gpu_cost_max_abs_diff_last_pair"] = float((hip_cost - held["cost"][-1]).abs().max())
                row["mean_total"] = sum(r.total for r in ours) / P
                t0 = time.perf_counter()
                _, t_host, p_host = DR.chain(feats[0][0], feats[0][1], n_ceps)
                row["host_ref_ms_per_pair"] = round(1e3 * (time.perf_counter() - t0), 1)
                row["totals_pair0"]["host_ref"] = t_host
                row["hip_vs_host_ref_rel_diff_pair0"] = abs(ours[0].total - t_host) / max(abs(t_host), 1e-300)
                row["path_len_pair0"] = [ours[0].length, int(len(p_host))]
            inner = {}
            for k, fn in impls.items():
                inner[k] = max(1, min(200, int(0.02 / max(timed(fn, 1), 1e-6))))
            times = {k: [] for k in impls}
            for _ in range(args.reps):
                for k, fn in impls.items():
                    times[k].append(timed(fn, inner[k]))
            for k, v in times.items():
                row[k + "_ms"] = round(1e3 * statistics.median(v), 4)
                row[k + "_min_ms"] = round(1e3 * min(v), 4)
                row[k + "_inner"] = inner[k]
            out["points"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        dtw.close()
    if not args.only_hip:
        ratios = []
        for D, n_ceps in ((100, 13), (100, 0), (5, 4)):
            for Ta, Tb in ((1, 1), (33, 65), (255, 257)):
                a, b = DR.make_feats(Ta, D, 100 * D + Ta), DR.make_feats(Tb, D, 100 * D + Tb + 5000)
                ref64 = DR.chain(a, b, n_ceps)[0]
                floor = float(np.abs(DR.chain(a, b, n_ceps, np.float32)[0].astype(np.float64) - ref64).max())
                got = E.op_dtw_cost(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), n_ceps).cpu().numpy()
                err = float(np.abs(got.astype(np.float64) - ref64).max())
                ratios.append({"D": D, "n_ceps": n_ceps, "Ta": Ta, "Tb": Tb, "floor": floor, "engine": err, "ratio": round(err / floor, 3)})
        out["parity"] = ratios
        out["parity_ratio_max"] = max(r["ratio"] for r in ratios)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
