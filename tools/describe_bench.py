"""Time 5 x 5 box smoothing (fdf_smooth_device) and steered BRIEF descriptors
(fdf_describe_device) on the benchmark's own batch: 512 x 1920x1080 S1 frames at t=16 n=9
max-threshold.

Smoothing is timed beside a plain device copy of the same frames (the traffic yardstick: one
read and one write of every byte) and beside the same smoothing written in torch on the device
(replicate-padded separable 5 x 5 sums in int16).  Per descriptor shape it reports the
describe step alone, the detect step measured in the same run and the ratio of the two, and the
same descriptors written in torch (what a user can do without the feature: the bin of every
angle, a chunked clamped gather of the 512 taps, a compare and a bit pack), alternating with
the HIP path in one process; the two results are compared for equality at the timed size.
Device events around back-to-back calls, every shape warmed first, profiler off.

    python tools/describe_bench.py [--frames 512] [--calls 50] [--rounds 5] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_smooth(torch, frames, out, chunk=32):
    """The smoothing in torch ops on the device, `chunk` frames at a time."""
    f, h, w = frames.shape
    iy = torch.arange(-2, h + 2, device=frames.device).clamp_(0, h - 1)
    ix = torch.arange(-2, w + 2, device=frames.device).clamp_(0, w - 1)
    for c in range(0, f, chunk):
        x = frames[c:c + chunk].to(torch.int16)
        p = x[:, :, ix]                                      # replicate-padded columns
        s = p[:, :, 0:w] + p[:, :, 1:w + 1] + p[:, :, 2:w + 2] + p[:, :, 3:w + 3] + p[:, :, 4:w + 4]
        p = s[:, iy]                                         # replicate-padded rows
        s = p[:, 0:h] + p[:, 1:h + 1] + p[:, 2:h + 2] + p[:, 3:h + 3] + p[:, 4:h + 4]
        out[c:c + chunk] = torch.div(s + 12, 25, rounding_mode="floor").to(torch.uint8)


def torch_describe(torch, frames, pts, offs, n, angles, table, n_bins, desc, budget=1 << 24):
    """The descriptors in torch ops on the device; `n` (the points' total) is known on the
    host, `table` is (n_bins, 256, 4) int64.  `budget`: gathered elements per chunk."""
    f, h, w = frames.shape
    flat = frames.reshape(-1)
    idx = torch.arange(n, device=pts.device)
    base = torch.searchsorted(offs[1:].contiguous(), idx, right=True) * (h * w)
    scale = torch.tensor(n_bins / (2 * math.pi), dtype=torch.float32, device=pts.device)
    weights = (1 << torch.arange(8, device=pts.device)).to(torch.int32)
    chunk = max(1, budget // 256)
    for c in range(0, n, chunk):
        e = min(n, c + chunk)
        if angles is None:
            t = table[0][None]
        else:
            a = angles[c:e]
            ok = a.abs() <= 7
            b = torch.round(torch.where(ok, a, torch.zeros_like(a)) * scale).long() % n_bins
            t = table[torch.where(ok, b, torch.zeros_like(b))]
        x = pts[c:e, 0].long()[:, None]
        y = pts[c:e, 1].long()[:, None]
        origin = base[c:e, None]
        first = flat[origin + (y + t[..., 1]).clamp_(0, h - 1) * w + (x + t[..., 0]).clamp_(0, w - 1)]
        second = flat[origin + (y + t[..., 3]).clamp_(0, h - 1) * w + (x + t[..., 2]).clamp_(0, w - 1)]
        bits = (first < second).view(e - c, 32, 8).to(torch.int32)
        desc[c:e] = (bits * weights).sum(2).to(torch.uint8)


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
    ap.add_argument("--calls", type=int, default=50, help="back-to-back HIP calls per timing")
    ap.add_argument("--torch-calls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    W, H = args.width, args.height
    shape = (H, W)
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    all_frames = workloads.s1_frames_torch(0, args.frames, W, H)
    all_smoothed = torch.zeros_like(all_frames)
    results = []

    # ---- smoothing of the batch, beside a copy and torch -----------------------------------
    scratch = torch.zeros_like(all_frames)

    def smooth():
        fast_hip.smooth_device(all_frames, all_smoothed)

    def copy():
        scratch.copy_(all_frames)

    def smooth_yardstick():
        torch_smooth(torch, all_frames, scratch)

    smooth()
    smooth_yardstick()
    torch.cuda.synchronize()
    equal = bool(torch.equal(all_smoothed, scratch))
    for fn, c in ((smooth, 10), (copy, 10), (smooth_yardstick, 1)):
        timed(torch, fn, c)
    ms = {"smooth": [], "copy": [], "torch": []}
    for _ in range(args.rounds):
        ms["smooth"].append(timed(torch, smooth, args.calls))
        ms["torch"].append(timed(torch, smooth_yardstick, args.torch_calls))
        ms["copy"].append(timed(torch, copy, args.calls))
    med = {name: statistics.median(v) for name, v in ms.items()}
    gbytes = 2 * all_frames.numel() / 1e9
    results.append({
        "shape": "smooth batch", "frames": args.frames, "width": W, "height": H,
        "torch_equal": equal, "smooth_ms": spread(ms["smooth"]), "copy_ms": spread(ms["copy"]),
        "torch_smooth_ms": spread(ms["torch"]), "smooth_over_copy": med["smooth"] / med["copy"],
        "torch_over_hip": med["torch"] / med["smooth"],
        "smooth_tb_per_s": gbytes / med["smooth"], "copy_tb_per_s": gbytes / med["copy"],
        "calls": args.calls, "torch_calls": args.torch_calls, "rounds": args.rounds,
    })
    print(json.dumps(results[-1]), flush=True)
    del scratch
    torch.cuda.empty_cache()

    # ---- descriptors -------------------------------------------------------------------------
    pattern = fast_hip.brief_pattern()
    for label, nf, n_bins, selected in (("batch all points 30 bins", args.frames, 30, False),
                                        ("batch selected 64x64 k=4 30 bins", args.frames, 30, True),
                                        ("single frame all points 30 bins", 1, 30, False),
                                        ("batch all points 1 bin, no angles", args.frames, 1, False)):
        frames = all_frames[:nf]
        smoothed = all_smoothed[:nf]
        cap = nf * 20_000
        pts = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
        offs = torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
        angles = torch.zeros(cap, dtype=torch.float32, device="cuda")
        desc = torch.zeros((cap, 32), dtype=torch.uint8, device="cuda")
        h_table = fast_hip.brief_steer(pattern, n_bins)
        table = torch.from_numpy(h_table).cuda()
        table64 = table.long()

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
        fast_hip.orient_device(frames, o_pts, o_offs, angles)
        torch.cuda.synchronize()
        n = int(o_offs[-1])
        assert n <= cap, (n, cap)
        use_angles = angles if n_bins > 1 else None

        def describe():
            fast_hip.describe_device(smoothed, o_pts, o_offs, desc, table, n_bins,
                                     angles=use_angles)

        t_desc = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")

        def yardstick():
            torch_describe(torch, smoothed, o_pts, o_offs, n, use_angles, table64, n_bins, t_desc)

        describe()
        yardstick()
        torch.cuda.synchronize()
        equal = bool(torch.equal(t_desc, desc[:n]))
        for fn, c in ((detect, 10), (describe, 10), (yardstick, 1)):
            timed(torch, fn, c)                                    # warm every path
        ms = {"describe": [], "detect": [], "torch": []}
        for _ in range(args.rounds):                               # HIP and torch alternate
            ms["describe"].append(timed(torch, describe, args.calls))
            ms["torch"].append(timed(torch, yardstick, args.torch_calls))
            ms["detect"].append(timed(torch, detect, args.calls))
        med = {name: statistics.median(v) for name, v in ms.items()}
        results.append({
            "shape": label, "frames": nf, "width": W, "height": H, "n_bins": n_bins,
            "angles": use_angles is not None, "points": n, "torch_equal": equal,
            "describe_ms": spread(ms["describe"]), "detect_ms": spread(ms["detect"]),
            "torch_describe_ms": spread(ms["torch"]),
            "describe_over_detect": med["describe"] / med["detect"],
            "torch_over_hip": med["torch"] / med["describe"],
            "ns_per_point": 1e6 * med["describe"] / max(n, 1),
            "calls": args.calls, "torch_calls": args.torch_calls, "rounds": args.rounds,
        })
        print(json.dumps(results[-1]), flush=True)
    doc = {"tool": "tools/describe_bench.py", "config": "t=16 n=9 max-threshold, S1 frames",
           "device": torch.cuda.get_device_name(0),
           "kernel_source_sha16": workloads.kernel_source_sha16(), "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0 if all(r["torch_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
