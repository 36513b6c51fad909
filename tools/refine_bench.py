"""Time the least-squares refinement (fdf_refine_device) on tools/ransac_bench.py's synthetic
matches: per frame pair M random integer query points below 1800, their rounded projections under
a mild homography, 40 % of the trains re-drawn uniformly, identity matches, homography model,
threshold 3.

Shapes: (a) 511 frame pairs x 2000 correspondences; (b) one pair x 2000; (c) 511 pairs x 200.  The
models to refine are fdf_ransac_device's with 1024 hypotheses.  Per shape and for 1 and 3 rounds it
reports the whole refine call (compaction and the refinement kernel) beside the RANSAC call on
the same inputs in the same process, and the same work written in torch float64 on the device as a
time yardstick only: scoring, the masked sums of the normalisation and of the normal equations
(batched over the frames), torch.linalg.solve, the denormalisation, the re-scoring and the
acceptance.  Torch sums in its own order, so its bits need not match; its inlier counts are
reported beside the HIP ones.  The paths alternate in one process.  Device events around
back-to-back calls (as many as fill a quarter of a second), every path warmed first, profiler
off; median, minimum and maximum over the rounds.

    python tools/refine_bench.py [--pairs 511] [--window-ms 250] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ransac_bench import spread, synthetic, timed  # noqa: E402


def torch_flags(h, x, y, u, v, tt):
    """(F, M) bool: the score of include/fdf.h under the models h (F, 9)."""
    g = h[:, :, None]
    P = (g[:, 0] * x + g[:, 1] * y) + g[:, 2]
    Q = (g[:, 3] * x + g[:, 4] * y) + g[:, 5]
    w = (g[:, 6] * x + g[:, 7] * y) + g[:, 8]
    rx = P - u * w
    ry = Q - v * w
    return (w > 0) & (rx * rx + ry * ry <= tt * (w * w))


def torch_refine(torch, h, xyuv, tt, n_rounds):
    """(refined (F, 9), (F,) counts): the homography rounds of include/fdf.h for all frames at
    once, summed in torch's order and solved by torch.linalg.solve."""
    x, y, u, v = xyuv
    flags = torch_flags(h, x, y, u, v, tt)
    count = flags.sum(dim=1)
    live = torch.ones_like(count, dtype=torch.bool)
    zero, one = torch.zeros_like(x), torch.ones_like(x)
    for _ in range(n_rounds):
        w = flags.to(torch.float64)
        n = w.sum(dim=1, keepdim=True)
        cx, cy, cu, cv = ((w * a).sum(dim=1, keepdim=True) / n for a in (x, y, u, v))
        s = (n + n) / (w * ((x - cx).abs() + (y - cy).abs())).sum(dim=1, keepdim=True)
        t = (n + n) / (w * ((u - cu).abs() + (v - cv).abs())).sum(dim=1, keepdim=True)
        X, Y, U, V = (x - cx) * s, (y - cy) * s, (u - cu) * t, (v - cv) * t
        r0 = torch.stack([X, Y, one, zero, zero, zero, -(U * X), -(U * Y)], dim=2)
        r1 = torch.stack([zero, zero, zero, X, Y, one, -(V * X), -(V * Y)], dim=2)
        w0, w1 = r0 * w[:, :, None], r1 * w[:, :, None]
        G = w0.transpose(1, 2) @ r0 + w1.transpose(1, 2) @ r1
        g = (w0 * U[:, :, None] + w1 * V[:, :, None]).sum(dim=1)
        ok = torch.isfinite(G).all(dim=2).all(dim=1) & torch.isfinite(g).all(dim=1) & (n[:, 0] >= 4)
        eye = torch.eye(8, dtype=torch.float64, device=h.device)
        hn = torch.linalg.solve(torch.where(ok[:, None, None], G, eye), g)
        Hn = torch.cat([hn, torch.ones_like(hn[:, :1])], dim=1).reshape(-1, 3, 3)
        T1 = torch.zeros_like(Hn)
        T2 = torch.zeros_like(Hn)
        T1[:, 0, 0], T1[:, 1, 1], T1[:, 2, 2] = s[:, 0], s[:, 0], 1.0
        T1[:, 0, 2], T1[:, 1, 2] = -(s * cx)[:, 0], -(s * cy)[:, 0]
        T2[:, 0, 0], T2[:, 1, 1], T2[:, 2, 2] = 1.0 / t[:, 0], 1.0 / t[:, 0], 1.0
        T2[:, 0, 2], T2[:, 1, 2] = cu[:, 0], cv[:, 0]
        H = T2 @ Hn @ T1
        h2 = (H / H[:, 2:, 2:]).reshape(-1, 9)
        ok &= torch.isfinite(h2).all(dim=1)
        h2 = torch.where(ok[:, None], h2, h)
        flags2 = torch_flags(h2, x, y, u, v, tt)
        count2 = flags2.sum(dim=1)
        live = live & ok & (count2 >= count)               # a frame that stops stays stopped
        h = torch.where(live[:, None], h2, h)
        flags = torch.where(live[:, None], flags2, flags)
        count = torch.where(live, count2, count)
    return h, count


def main(argv=None):
    import numpy as np
    import torch

    import workloads
    from feature_detector_fast_amd import fast_hip

    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=511)
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timing, at least")
    ap.add_argument("--torch-calls", type=int, default=1, help="the same for torch; 0: no torch")
    ap.add_argument("--window-ms", type=float, default=250.0,
                    help="calls are added until one timing lasts about this long")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    threshold, seed, n_hyp = 3.0, 1, 1024
    results = []
    for label, pairs, m in (("(a) %d pairs x 2000 correspondences" % args.pairs, args.pairs, 2000),
                            ("(b) 1 pair x 2000", 1, 2000),
                            ("(c) %d pairs x 200" % args.pairs, args.pairs, 200)):
        q, t = synthetic(np, pairs, m, 7)
        n = pairs * m
        qf, tf = q.astype(np.float64), t.astype(np.float64)
        xyuv = torch.from_numpy(np.stack([qf[:, 0], qf[:, 1], tf[:, 0], tf[:, 1]])
                                .reshape(4, pairs, m)).cuda()
        d_q = torch.from_numpy(q.view(np.int32)).cuda()
        d_t = torch.from_numpy(t.view(np.int32)).cuda()
        matches = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        matches[:, 0] = torch.arange(n, dtype=torch.int32, device="cuda")
        d_offs = torch.from_numpy(np.arange(pairs + 1, dtype=np.int64) * m).cuda()
        models = torch.zeros((pairs, 11), dtype=torch.float64, device="cuda")
        refined = torch.zeros((pairs, 11), dtype=torch.float64, device="cuda")
        inliers = torch.zeros(n, dtype=torch.uint8, device="cuda")
        accepted = torch.zeros(pairs, dtype=torch.int32, device="cuda")
        need = fast_hip.ransac_scratch_bytes(pairs, n, n_hyp)
        raw = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
        lead = (-raw.data_ptr()) % 256
        scratch = raw[lead:lead + need]
        tt = float(np.float64(np.float32(threshold)) ** 2)

        def ransac():
            fast_hip.ransac_device(matches, d_offs, d_q, d_t, d_offs, models, scratch,
                                   inliers=inliers, model="homography", n_hyp=n_hyp,
                                   threshold=threshold, seed=seed)

        def refine(n_rounds):
            fast_hip.refine_device(matches, d_offs, d_q, d_t, d_offs, models, refined, scratch,
                                   inliers=inliers, rounds=accepted, model="homography",
                                   threshold=threshold, n_rounds=n_rounds)

        ransac()
        torch.cuda.synchronize()
        start = fast_hip.unpack_models(models.cpu().numpy())
        d_h = models[:, :9].contiguous()
        paths = [("ransac", ransac, args.calls)]
        row = {"shape": label, "frame_pairs": pairs, "correspondences": m, "hypotheses": n_hyp,
               "model": "homography", "threshold": threshold,
               "mean_inliers_ransac": float(start["n_inliers"].mean())}
        for n_rounds in (1, 3):
            refine(n_rounds)
            torch.cuda.synchronize()
            got = fast_hip.unpack_models(refined.cpu().numpy())
            row["rounds_%d" % n_rounds] = {
                "mean_inliers": float(got["n_inliers"].mean()),
                "mean_accepted": float(accepted.cpu().numpy().mean())}
            paths.append(("refine_%d" % n_rounds, lambda k=n_rounds: refine(k), args.calls))
            if args.torch_calls > 0:
                _, counts = torch_refine(torch, d_h, xyuv, tt, n_rounds)
                row["rounds_%d" % n_rounds]["torch_mean_inliers"] = float(counts.double().mean())
                paths.append(("torch_%d" % n_rounds,
                              lambda k=n_rounds: torch_refine(torch, d_h, xyuv, tt, k),
                              args.torch_calls))
        # warm every path, and size its timing window from the warm-up's own time per call
        paths = [(name, fn, max(c, int(args.window_ms / max(timed(torch, fn, c), 1e-3)) + 1))
                 for name, fn, c in paths]
        ms = {name: [] for name, _, _ in paths}
        for _ in range(args.rounds):                               # the paths alternate
            for name, fn, c in paths:
                ms[name].append(timed(torch, fn, c))
        med = {name: statistics.median(v) for name, v in ms.items()}
        row["ransac_ms"] = spread(ms["ransac"])
        for n_rounds in (1, 3):
            r = row["rounds_%d" % n_rounds]
            r["refine_ms"] = spread(ms["refine_%d" % n_rounds])
            r["refine_over_ransac"] = med["refine_%d" % n_rounds] / med["ransac"]
            if args.torch_calls > 0:
                r["torch_ms"] = spread(ms["torch_%d" % n_rounds])
                r["torch_over_hip"] = med["torch_%d" % n_rounds] / med["refine_%d" % n_rounds]
        row["calls"] = dict((name, c) for name, _, c in paths)
        row["timing_rounds"] = args.rounds
        results.append(row)
        print(json.dumps(row), flush=True)
        del xyuv, matches, models, refined, inliers, raw, scratch, d_h
        torch.cuda.empty_cache()
    doc = {"tool": "tools/refine_bench.py",
           "config": "synthetic planted homography, 40 % outliers, identity matches, T = 3, "
                     "models from ransac_device with 1024 hypotheses",
           "device": torch.cuda.get_device_name(0),
           "kernel_source_sha16": workloads.kernel_source_sha16(), "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
