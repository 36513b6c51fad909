"""Time keypoint orientation (fdf_orient_device) on the benchmark's own batch: 512 x 1920x1080
S1 frames at t=16 n=9 max-threshold.

Per shape it reports the orientation alone, the detect step measured in the same run and the
ratio of the two, and the same orientation written in torch on the device (what a user can do
without the feature: a chunked clamped gather over the disc's offsets, integer sums and
torch.atan2), alternating with the HIP path in one process; the moments of the two are
compared for equality at the timed size.  Device events around back-to-back calls, every shape
warmed first, profiler off.

    python tools/orient_bench.py [--frames 512] [--calls 100] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def disc_offsets(torch, u, device):
    """(dx, dy) int64 tensors of the disc's taps."""
    r = len(u) - 1
    taps = [(d, v) for v in range(-r, r + 1) for d in range(-int(u[abs(v)]), int(u[abs(v)]) + 1)]
    t = torch.tensor(taps, dtype=torch.int64, device=device)
    return t[:, 0].contiguous(), t[:, 1].contiguous()


def torch_orient(torch, frames, pts, offs, n, dx, dy, moments, angles, budget=1 << 25):
    """The orientation in torch ops on the device; `n` (the points' total) is known on the
    host.  `budget`: gathered elements per chunk."""
    f, h, w = frames.shape
    flat = frames.reshape(-1)
    idx = torch.arange(n, device=pts.device)
    base = torch.searchsorted(offs[1:].contiguous(), idx, right=True) * (h * w)
    chunk = max(1, budget // dx.numel())
    for c in range(0, n, chunk):
        e = min(n, c + chunk)
        cx = (pts[c:e, 0].long()[:, None] + dx[None, :]).clamp_(0, w - 1)
        cy = (pts[c:e, 1].long()[:, None] + dy[None, :]).clamp_(0, h - 1)
        val = flat[base[c:e, None] + cy * w + cx].long()
        moments[c:e, 0] = (val * dx[None, :]).sum(1)
        moments[c:e, 1] = (val * dy[None, :]).sum(1)
    angles[:n] = torch.atan2(moments[:n, 1].float(), moments[:n, 0].float())


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
    import torch

    import workloads
    from feature_detector_fast_amd import Config, NonMaximalSuppression, fast_hip

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=100, help="back-to-back HIP calls per timing")
    ap.add_argument("--torch-calls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    W, H = args.width, args.height
    shape = (H, W)
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    all_frames = workloads.s1_frames_torch(0, args.frames, W, H)
    results = []
    for label, nf, radius, selected in (("batch all points r=15", args.frames, 15, False),
                                        ("batch selected 64x64 k=4 r=15", args.frames, 15, True),
                                        ("single frame all points r=15", 1, 15, False),
                                        ("batch all points r=7", args.frames, 7, False),
                                        ("batch all points r=31", args.frames, 31, False)):
        frames = all_frames[:nf]
        cap = nf * 20_000
        pts = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
        offs = torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
        angles = torch.zeros(cap, dtype=torch.float32, device="cuda")
        moments = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")

        def detect():
            fast_hip.detect_device(frames, cfg, pts, offs)

        detect()
        if selected:
            scores = torch.zeros(cap, dtype=torch.int16, device="cuda")
            sel = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
            sel_scores = torch.zeros(cap, dtype=torch.int16, device="cuda")
            sel_offs = torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
            fast_hip.score_device(frames, cfg, pts, offs, scores)
            fast_hip.select_device(pts, scores, offs, shape, (64, 64), 4, sel, sel_scores,
                                   sel_offs)
            o_pts, o_offs = sel, sel_offs
        else:
            o_pts, o_offs = pts.clone(), offs.clone()    # detect() rewrites pts while timed
        torch.cuda.synchronize()
        n = int(o_offs[-1])
        assert n <= cap, (n, cap)

        def orient():
            fast_hip.orient_device(frames, o_pts, o_offs, angles, radius=radius, moments=moments)

        def orient_angles_only():
            fast_hip.orient_device(frames, o_pts, o_offs, angles, radius=radius)

        dx, dy = disc_offsets(torch, fast_hip.orient_disc(radius), "cuda")
        t_moments = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
        t_angles = torch.zeros(n, dtype=torch.float32, device="cuda")

        def yardstick():
            torch_orient(torch, frames, o_pts, o_offs, n, dx, dy, t_moments, t_angles)

        orient()
        yardstick()
        torch.cuda.synchronize()
        equal = bool(torch.equal(t_moments, moments[:n].long()))
        diff = (angles[:n].double() - t_angles.double()).abs()
        angle_diff = float(torch.minimum(diff, 2 * torch.pi - diff).max()) if n else 0.0
        for fn, c in ((detect, 20), (orient, 20), (orient_angles_only, 20), (yardstick, 1)):
            timed(torch, fn, c)                                    # warm every path
        ms = {"orient": [], "angles_only": [], "detect": [], "torch": []}
        for _ in range(args.rounds):                               # HIP and torch alternate
            ms["orient"].append(timed(torch, orient, args.calls))
            ms["torch"].append(timed(torch, yardstick, args.torch_calls))
            ms["detect"].append(timed(torch, detect, args.calls))
            ms["angles_only"].append(timed(torch, orient_angles_only, args.calls))
        med = {name: statistics.median(v) for name, v in ms.items()}
        results.append({
            "shape": label, "frames": nf, "width": W, "height": H, "radius": radius,
            "taps": int(dx.numel()), "points": n, "torch_moments_equal": equal,
            "angle_max_diff_vs_torch": angle_diff,
            "orient_ms": spread(ms["orient"]), "orient_angles_only_ms": spread(ms["angles_only"]),
            "detect_ms": spread(ms["detect"]), "torch_orient_ms": spread(ms["torch"]),
            "orient_over_detect": med["orient"] / med["detect"],
            "torch_over_hip": med["torch"] / med["orient"],
            "calls": args.calls, "torch_calls": args.torch_calls, "rounds": args.rounds,
        })
        print(json.dumps(results[-1]), flush=True)
    doc = {"tool": "tools/orient_bench.py", "config": "t=16 n=9 max-threshold, S1 frames",
           "device": torch.cuda.get_device_name(0),
           "kernel_source_sha16": workloads.kernel_source_sha16(), "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0 if all(r["torch_moments_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
