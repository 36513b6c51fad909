"""Time RANSAC fundamental-matrix estimation (fdf_fundamental_device) beside the homography
estimation it joins (fdf_ransac_device, FDF_MODEL_HOMOGRAPHY) on the same correspondences and the
same number of hypotheses: per frame pair M points before two pinhole cameras, projected to float
pixels, 30 % of the trains re-drawn uniformly, identity matches, threshold 1.

Shapes: (a) 8 frame pairs x 1024 correspondences x 512 hypotheses; (b) 64 pairs x 1024 x 512.
Per shape it reports both whole HIP calls (compaction, sampling, fit, scoring, finalisation) and
their ratio.  Where the shape has at most --torch-max-hyp hypotheses in all it also times the same
scoring written in torch float64 on the device (what a user can do without the feature): the
hypotheses' matrices come from the host restatement (tests/_fundamental_reference.py, not timed),
torch builds the hypotheses x correspondences inlier matrix with the contract's operations in
the contract's order, counts and takes the first maximum; the best hypothesis and its count must
equal the call's.  The paths alternate in one process.  Device events around back-to-back calls
(as many as fill a quarter of a second), every path warmed first, profiler off; median, minimum
and maximum over the rounds.

    python tools/fundamental_bench.py [--window-ms 250] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FLOP_PER_PAIR = 33          # the score of include/fdf.h: 19 multiplications, 14 additions


def synthetic(np, pairs, m, seed):
    """(queries, trains) as (pairs * m, 2) float32."""
    rng = np.random.default_rng(seed)
    n = pairs * m
    P = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 10, n)], 1)
    a = 0.08
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    P2 = P @ R.T + np.array([0.6, 0.1, 0.2])
    q = 700 * P[:, :2] / P[:, 2:] + (900, 700)
    t = 700 * P2[:, :2] / P2[:, 2:] + (900, 700)
    bad = rng.random(n) < 0.3
    t[bad] = rng.uniform(0, 1800, (int(bad.sum()), 2))
    return q.astype(np.float32), t.astype(np.float32)


def torch_score(torch, f, valid, xyuv, tt, chunk, out):
    """out[0][k] = the first best hypothesis of frame k, out[1][k] = its count, from the matrices
    f (F, H, 9), their validity (F, H) and the correspondences xyuv (4, F, M)."""
    for f0 in range(0, f.shape[0], chunk):
        f1 = min(f.shape[0], f0 + chunk)
        g = f[f0:f1, :, :, None]
        x, y, u, v = (xyuv[k, f0:f1, None, :] for k in range(4))
        l0 = (g[:, :, 0] * x + g[:, :, 1] * y) + g[:, :, 2]
        l1 = (g[:, :, 3] * x + g[:, :, 4] * y) + g[:, :, 5]
        l2 = (g[:, :, 6] * x + g[:, :, 7] * y) + g[:, :, 8]
        m0 = (g[:, :, 0] * u + g[:, :, 3] * v) + g[:, :, 6]
        m1 = (g[:, :, 1] * u + g[:, :, 4] * v) + g[:, :, 7]
        r = (u * l0 + v * l1) + l2
        s = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
        counts = ((s > 0) & (r * r <= tt * s)).sum(dim=2)
        counts = torch.where(valid[f0:f1], counts, torch.full_like(counts, -1))
        best = counts.max(dim=1)
        # the first maximum: the lowest hypothesis among the equal counts
        first = (counts == best.values[:, None]).to(torch.int8).argmax(dim=1)
        out[0][f0:f1] = first
        out[1][f0:f1] = best.values


def timed(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main(argv=None):
    import numpy as np
    import torch

    import _fundamental_reference as ref
    import workloads
    from feature_detector_fast_amd import fast_hip

    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="back-to-back HIP calls per timing, at least")
    ap.add_argument("--torch-max-hyp", type=int, default=4096,
                    help="frames x hypotheses up to which the torch scoring is timed; 0: never")
    ap.add_argument("--window-ms", type=float, default=250.0,
                    help="calls are added until one timing lasts about this long")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunk-elements", type=int, default=1 << 25,
                    help="elements of one torch temporary (frames per chunk follow from it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    threshold, seed = 1.0, 1
    results = []
    for label, pairs, m, n_hyp in (("(a) 8 pairs x 1024 correspondences x 512 hypotheses", 8, 1024, 512),
                                   ("(b) 64 pairs x 1024 x 512", 64, 1024, 512)):
        q, t = synthetic(np, pairs, m, 7)
        n = pairs * m
        offs = np.arange(pairs + 1, dtype=np.int64) * m
        d_q, d_t = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
        matches = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        matches[:, 0] = torch.arange(n, dtype=torch.int32, device="cuda")
        d_offs = torch.from_numpy(offs).cuda()
        models = torch.zeros((pairs, 11), dtype=torch.float64, device="cuda")
        h_models = torch.zeros((pairs, 11), dtype=torch.float64, device="cuda")
        inliers = torch.zeros(n, dtype=torch.uint8, device="cuda")
        need = fast_hip.fundamental_scratch_bytes(pairs, n, n_hyp)
        raw = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
        lead = (-raw.data_ptr()) % 256
        scratch = raw[lead:lead + need]

        def fundamental():
            fast_hip.fundamental_device(matches, d_offs, d_q, d_t, d_offs, models, scratch,
                                        inliers=inliers, n_hyp=n_hyp, threshold=threshold, seed=seed)

        def homography():
            fast_hip.ransac_device(matches, d_offs, d_q, d_t, d_offs, h_models, scratch,
                                   inliers=inliers, model="homography", n_hyp=n_hyp,
                                   threshold=threshold, seed=seed)

        paths = [("fundamental", fundamental, args.calls), ("homography", homography, args.calls)]
        use_torch = pairs * n_hyp <= args.torch_max_hyp
        if use_torch:
            # the hypotheses' matrices from the host restatement (not timed)
            f = np.zeros((pairs, n_hyp, 9))
            valid = np.zeros((pairs, n_hyp), dtype=bool)
            qf, tf = q.astype(np.float64), t.astype(np.float64)
            for k in range(pairs):
                s = slice(k * m, (k + 1) * m)
                f[k], valid[k] = ref.hypotheses(qf[s, 0], qf[s, 1], tf[s, 0], tf[s, 1], k, n_hyp, seed)
            d_f, d_valid = torch.from_numpy(f).cuda(), torch.from_numpy(valid).cuda()
            xyuv = torch.from_numpy(np.stack([qf[:, 0], qf[:, 1], tf[:, 0], tf[:, 1]])
                                    .reshape(4, pairs, m)).cuda()
            t_out = (torch.zeros(pairs, dtype=torch.int64, device="cuda"),
                     torch.zeros(pairs, dtype=torch.int64, device="cuda"))
            tt = float(np.float64(np.float32(threshold)) ** 2)
            chunk = max(1, args.chunk_elements // (n_hyp * m))

            def yardstick():
                torch_score(torch, d_f, d_valid, xyuv, tt, chunk, t_out)

            paths.append(("torch", yardstick, 1))

        for _, fn, _ in paths:
            fn()
        torch.cuda.synchronize()
        got = fast_hip.unpack_models(models.cpu().numpy())
        equal = None
        if use_torch:
            equal = bool(np.array_equal(got["hypothesis"], t_out[0].cpu().numpy()) and
                         np.array_equal(got["n_inliers"], t_out[1].cpu().numpy()))
        # warm every path, and size its timing window from the warm-up's own time per call
        paths = [(name, fn, max(c, int(args.window_ms / max(timed(torch, fn, c), 1e-3)) + 1))
                 for name, fn, c in paths]
        ms = {name: [] for name, _, _ in paths}
        for _ in range(args.rounds):                               # the paths alternate
            for name, fn, c in paths:
                ms[name].append(timed(torch, fn, c))
        med = {name: statistics.median(v) for name, v in ms.items()}
        ratios = [a / b for a, b in zip(ms["fundamental"], ms["homography"])]
        pair_count = pairs * m * n_hyp
        row = {
            "shape": label, "frame_pairs": pairs, "correspondences": m, "hypotheses": n_hyp,
            "threshold": threshold, "scored_pairs": pair_count,
            "fundamental_ms": spread(ms["fundamental"]), "homography_ms": spread(ms["homography"]),
            "fundamental_over_homography": spread(ratios),
            "gpairs_per_s": pair_count / med["fundamental"] / 1e6,
            "fp64_gflops_scoring_only": FLOP_PER_PAIR * pair_count / med["fundamental"] / 1e6,
            "mean_inliers": float(got["n_inliers"].mean()), "mean_valid": float(got["n_valid"].mean()),
            "calls": dict((name, c) for name, _, c in paths), "rounds": args.rounds,
        }
        if use_torch:
            row.update({"torch_equal": equal, "torch_score_ms": spread(ms["torch"]),
                        "torch_over_fundamental": med["torch"] / med["fundamental"],
                        "torch_frames_per_chunk": chunk})
            del d_f, d_valid, xyuv
        results.append(row)
        print(json.dumps(row), flush=True)
        del matches, models, h_models, inliers, raw, scratch
        torch.cuda.empty_cache()
    doc = {"tool": "tools/fundamental_bench.py",
           "config": "synthetic two-view scene, float pixels, 30 % outliers, identity matches, T = 1",
           "device": torch.cuda.get_device_name(0),
           "kernel_source_sha16": workloads.kernel_source_sha16(), "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0 if all(r.get("torch_equal") is not False for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
