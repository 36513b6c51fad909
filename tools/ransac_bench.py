"""Time RANSAC model estimation (fdf_ransac_device) on synthetic matches: per frame pair M random
integer query points below 1800, their rounded projections under a mild homography, 40 % of the
trains re-drawn uniformly, identity matches, homography model, threshold 3.

Shapes: (a) 511 frame pairs x 2000 correspondences x 1024 hypotheses; (b) one pair x 2000 x 1024;
(c) 511 pairs x 200 x 256.  Per shape it reports the whole HIP call (compaction, sampling, fit,
scoring, finalisation) and the same scoring written in torch float64 on the device (what a user
can do without the feature): the hypotheses' models come from the host restatement
(tests/_ransac_reference.py, not timed), torch builds the hypotheses x correspondences inlier
matrix a chunk of frames at a time with the contract's operations in the contract's order, counts
and takes the first maximum.  The two alternate in one process; the best hypothesis and its count
must be equal at the timed size.  Device events around back-to-back calls (as many as fill a
quarter of a second), every shape warmed first, profiler off; median, minimum and maximum over
the rounds.

    python tools/ransac_bench.py [--pairs 511] [--window-ms 250] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FLOP_PER_PAIR = 21          # the score of include/fdf.h: 12 multiplications, 9 additions


def synthetic(np, pairs, m, seed):
    """(queries, trains) as (pairs * m, 2) uint32."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 1800, (pairs * m, 2)).astype(np.uint32)
    H = np.array([[1.02, 0.03, 5.0], [-0.02, 0.98, 40.0], [1e-5, -2e-5, 1.0]])
    p = np.c_[q.astype(np.float64), np.ones(len(q))] @ H.T
    t = np.rint(p[:, :2] / p[:, 2:]).astype(np.uint32)
    bad = rng.random(len(q)) < 0.4
    t[bad] = rng.integers(0, 2048, (int(bad.sum()), 2))
    return q, t


def torch_score(torch, h, valid, xyuv, tt, chunk, out):
    """out[0][f] = the first best hypothesis of frame f, out[1][f] = its count, from the models
    h (F, H, 9), their validity (F, H) and the correspondences xyuv (4, F, M)."""
    for f0 in range(0, h.shape[0], chunk):
        f1 = min(h.shape[0], f0 + chunk)
        g = h[f0:f1, :, :, None]
        x, y, u, v = (xyuv[k, f0:f1, None, :] for k in range(4))
        P = (g[:, :, 0] * x + g[:, :, 1] * y) + g[:, :, 2]
        Q = (g[:, :, 3] * x + g[:, :, 4] * y) + g[:, :, 5]
        w = (g[:, :, 6] * x + g[:, :, 7] * y) + g[:, :, 8]
        rx = P - u * w
        ry = Q - v * w
        e = rx * rx + ry * ry
        lim = tt * (w * w)
        counts = ((w > 0) & (e <= lim)).sum(dim=2)
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

    import _ransac_reference as ref
    import workloads
    from feature_detector_fast_amd import fast_hip

    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=511)
    ap.add_argument("--calls", type=int, default=10, help="back-to-back HIP calls per timing, at least")
    ap.add_argument("--torch-calls", type=int, default=1, help="the same for torch; 0: no torch")
    ap.add_argument("--window-ms", type=float, default=250.0,
                    help="calls are added until one timing lasts about this long")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunk-elements", type=int, default=1 << 25,
                    help="elements of one torch temporary (frames per chunk follow from it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    threshold, seed = 3.0, 1
    results = []
    for label, pairs, m, n_hyp in (
            ("(a) %d pairs x 2000 correspondences x 1024 hypotheses" % args.pairs, args.pairs, 2000, 1024),
            ("(b) 1 pair x 2000 x 1024", 1, 2000, 1024),
            ("(c) %d pairs x 200 x 256" % args.pairs, args.pairs, 200, 256)):
        q, t = synthetic(np, pairs, m, 7)
        n = pairs * m
        offs = np.arange(pairs + 1, dtype=np.int64) * m
        # the hypotheses' models from the host restatement (not timed)
        h = np.zeros((pairs, n_hyp, 9))
        valid = np.zeros((pairs, n_hyp), dtype=bool)
        qf, tf = q.astype(np.float64), t.astype(np.float64)
        for f in range(pairs):
            s = slice(f * m, (f + 1) * m)
            h[f], valid[f] = ref.hypotheses(qf[s, 0], qf[s, 1], tf[s, 0], tf[s, 1], f,
                                            ref.HOMOGRAPHY, n_hyp, seed)
        d_h, d_valid = torch.from_numpy(h).cuda(), torch.from_numpy(valid).cuda()
        xyuv = torch.from_numpy(np.stack([qf[:, 0], qf[:, 1], tf[:, 0], tf[:, 1]])
                                .reshape(4, pairs, m)).cuda()
        d_q = torch.from_numpy(q.view(np.int32)).cuda()
        d_t = torch.from_numpy(t.view(np.int32)).cuda()
        matches = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        matches[:, 0] = torch.arange(n, dtype=torch.int32, device="cuda")
        d_offs = torch.from_numpy(offs).cuda()
        models = torch.zeros((pairs, 11), dtype=torch.float64, device="cuda")
        inliers = torch.zeros(n, dtype=torch.uint8, device="cuda")
        need = fast_hip.ransac_scratch_bytes(pairs, n, n_hyp)
        raw = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
        lead = (-raw.data_ptr()) % 256
        scratch = raw[lead:lead + need]
        t_out = (torch.zeros(pairs, dtype=torch.int64, device="cuda"),
                 torch.zeros(pairs, dtype=torch.int64, device="cuda"))
        tt = float(np.float64(np.float32(threshold)) ** 2)
        chunk = max(1, args.chunk_elements // (n_hyp * m))

        def hip():
            fast_hip.ransac_device(matches, d_offs, d_q, d_t, d_offs, models, scratch,
                                   inliers=inliers, model="homography", n_hyp=n_hyp,
                                   threshold=threshold, seed=seed)

        def yardstick():
            torch_score(torch, d_h, d_valid, xyuv, tt, chunk, t_out)

        use_torch = args.torch_calls > 0
        hip()
        if use_torch:
            yardstick()
        torch.cuda.synchronize()
        got = fast_hip.unpack_models(models.cpu().numpy())
        equal = None
        if use_torch:
            equal = bool(np.array_equal(got["hypothesis"], t_out[0].cpu().numpy()) and
                         np.array_equal(got["n_inliers"], t_out[1].cpu().numpy()))
        paths = [("hip", hip, args.calls)]
        if use_torch:
            paths.append(("torch", yardstick, args.torch_calls))
        # warm every path, and size its timing window from the warm-up's own time per call
        paths = [(name, fn, max(c, int(args.window_ms / max(timed(torch, fn, c), 1e-3)) + 1))
                 for name, fn, c in paths]
        ms = {name: [] for name, _, _ in paths}
        for _ in range(args.rounds):                               # the paths alternate
            for name, fn, c in paths:
                ms[name].append(timed(torch, fn, c))
        med = {name: statistics.median(v) for name, v in ms.items()}
        pair_count = pairs * m * n_hyp
        row = {
            "shape": label, "frame_pairs": pairs, "correspondences": m, "hypotheses": n_hyp,
            "model": "homography", "threshold": threshold, "scored_pairs": pair_count,
            "ransac_ms": spread(ms["hip"]),
            "gpairs_per_s": pair_count / med["hip"] / 1e6,
            "fp64_gflops_scoring_only": FLOP_PER_PAIR * pair_count / med["hip"] / 1e6,
            "mean_inliers": float(got["n_inliers"].mean()), "mean_valid": float(got["n_valid"].mean()),
            "calls": dict((name, c) for name, _, c in paths), "rounds": args.rounds,
        }
        if use_torch:
            row.update({"torch_equal": equal, "torch_score_ms": spread(ms["torch"]),
                        "torch_over_hip": med["torch"] / med["hip"],
                        "torch_frames_per_chunk": chunk})
        results.append(row)
        print(json.dumps(row), flush=True)
        del d_h, d_valid, xyuv, matches, models, inliers, raw, scratch
        torch.cuda.empty_cache()
    doc = {"tool": "tools/ransac_bench.py",
           "config": "synthetic planted homography, 40 % outliers, identity matches, T = 3",
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
