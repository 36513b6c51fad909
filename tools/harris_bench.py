"""Time the Harris response of keypoints (fdf_harris_device) on the benchmark's own batch:
512 x 1920x1080 S1 frames at t=16 n=9.

Per shape it reports the Harris stage alone (with and without the int64 output) and, in the
same process and alternating with it, two yardsticks: the same integers written in torch on the
device (what a user can do without the feature: Sobel by shifted slices of the replicated
frames in int32, the block sum by shifted integer adds, a gather at the points and int64 for
the response; whole frames, a chunk of frames at a time), whose responses are compared for
equality at the timed size, and the neighbouring stages fdf_score_device and fdf_orient_device
(radius 15) on the same lists.  Device events around back-to-back calls, every shape warmed
first, profiler off.

    python tools/harris_bench.py [--frames 512] [--calls 400] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_harris(torch, frames, pts, host_offs, block, k, out, chunk=16):
    """The responses in torch ops on the device; `host_offs` (the frames' offsets) is known on
    the host.  `chunk`: frames whose gradient planes are alive at once."""
    f, h, w = frames.shape
    hb = block // 2
    m = hb + 1
    rows = torch.arange(-m, h + m, device=frames.device).clamp_(0, h - 1)
    cols = torch.arange(-m, w + m, device=frames.device).clamp_(0, w - 1)
    k_num, k_den = k
    H, W = h + 2 * hb, w + 2 * hb                     # gradient planes: the blocks' reach
    for f0 in range(0, f, chunk):
        f1 = min(f, f0 + chunk)
        lo, hi = host_offs[f0], host_offs[f1]
        if lo == hi:
            continue
        p = frames[f0:f1].index_select(1, rows).index_select(2, cols).int()

        def at(dx, dy):                               # I(X + dx, Y + dy) over the planes
            return p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]

        ix = 2 * (at(1, 0) - at(-1, 0)) + (at(1, -1) - at(-1, -1)) + (at(1, 1) - at(-1, 1))
        iy = 2 * (at(0, 1) - at(0, -1)) + (at(-1, 1) - at(-1, -1)) + (at(1, 1) - at(1, -1))
        sums = []
        for prod in (ix * ix, iy * iy, ix * iy):
            acc = prod[:, :, 0:w].clone()
            for d in range(1, block):
                acc += prod[:, :, d:d + w]
            box = acc[:, 0:h].clone()
            for v in range(1, block):
                box += acc[:, v:v + h]
            sums.append(box)
        idx = torch.arange(lo, hi, device=frames.device)
        fr = torch.searchsorted(torch.as_tensor(host_offs[f0 + 1:f1 + 1], device=frames.device),
                                idx, right=True)
        x, y = pts[lo:hi, 0].long(), pts[lo:hi, 1].long()
        a, b, c = (s[fr, y, x].long() for s in sums)
        out[lo:hi] = k_den * (a * b - c * c) - k_num * (a + b) * (a + b)


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
    ap.add_argument("--calls", type=int, default=400, help="back-to-back HIP calls per timing")
    ap.add_argument("--torch-calls", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    W, H = args.width, args.height
    k = (1, 25)
    maxt = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    off = Config(16, 9, NonMaximalSuppression.Off)
    all_frames = workloads.s1_frames_torch(0, args.frames, W, H)
    results = []
    for label, nf, cfg, block in (("batch max-t points block 7", args.frames, maxt, 7),
                                  ("batch nms-off points (dense) block 7", args.frames, off, 7),
                                  ("single frame max-t points block 7", 1, maxt, 7),
                                  ("batch max-t points block 3", args.frames, maxt, 3)):
        frames = all_frames[:nf]
        cap = nf * 20_000
        offs = torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
        while True:
            pts = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
            fast_hip.detect_device(frames, cfg, pts, offs)
            n = int(offs[-1])
            if n <= cap:
                break
            cap = n
        host_offs = offs.cpu().tolist()
        scores = torch.zeros(cap, dtype=torch.int16, device="cuda")
        responses = torch.zeros(cap, dtype=torch.int64, device="cuda")
        fast_scores = torch.zeros(cap, dtype=torch.int16, device="cuda")
        angles = torch.zeros(cap, dtype=torch.float32, device="cuda")
        t_responses = torch.zeros(n, dtype=torch.int64, device="cuda")

        def harris():
            fast_hip.harris_device(frames, pts, offs, scores, block, k, responses=responses)

        def harris_scores_only():
            fast_hip.harris_device(frames, pts, offs, scores, block, k)

        def score():
            fast_hip.score_device(frames, cfg, pts, offs, fast_scores)

        def orient():
            fast_hip.orient_device(frames, pts, offs, angles, radius=15)

        def yardstick():
            torch_harris(torch, frames, pts, host_offs, block, k, t_responses)

        harris()
        yardstick()
        torch.cuda.synchronize()
        equal = bool(torch.equal(t_responses, responses[:n]))
        codes_equal = bool((fast_hip.harris_codes(t_responses.cpu().numpy()) ==
                            scores[:n].cpu().numpy().view("uint16")).all())
        distinct = {"harris": int(torch.unique(scores[:n]).numel())}
        score()
        torch.cuda.synchronize()
        distinct["fast"] = int(torch.unique(fast_scores[:n]).numel())
        for fn, c in ((harris, 10), (harris_scores_only, 10), (score, 10), (orient, 10),
                      (yardstick, 1)):
            timed(torch, fn, c)                                    # warm every path
        ms = {"harris": [], "scores_only": [], "score": [], "orient": [], "torch": []}
        for _ in range(args.rounds):                               # HIP and torch alternate
            ms["harris"].append(timed(torch, harris, args.calls))
            ms["torch"].append(timed(torch, yardstick, args.torch_calls))
            ms["score"].append(timed(torch, score, args.calls))
            ms["scores_only"].append(timed(torch, harris_scores_only, args.calls))
            ms["orient"].append(timed(torch, orient, args.calls))
        med = {name: statistics.median(v) for name, v in ms.items()}
        window = (block + 2) ** 2
        results.append({
            "shape": label, "frames": nf, "width": W, "height": H, "block": block,
            "k": list(k), "points": n, "torch_responses_equal": equal,
            "torch_codes_equal": codes_equal, "distinct_scores": distinct,
            "harris_ms": spread(ms["harris"]), "harris_scores_only_ms": spread(ms["scores_only"]),
            "score_device_ms": spread(ms["score"]), "orient_r15_ms": spread(ms["orient"]),
            "torch_harris_ms": spread(ms["torch"]),
            "torch_over_hip": med["torch"] / med["harris"],
            "harris_over_score": med["harris"] / med["score"],
            "harris_over_orient": med["harris"] / med["orient"],
            "points_per_us": n / (med["harris"] * 1e3),
            # bytes the algorithm needs: the window's pixels once, the point, both outputs
            "window_gbytes_per_s": n * (window + 8 + 2 + 8) / (med["harris"] * 1e6),
            "calls": args.calls, "torch_calls": args.torch_calls, "rounds": args.rounds,
        })
        print(json.dumps(results[-1]), flush=True)
        del pts, scores, responses, fast_scores, angles, t_responses
    doc = {"tool": "tools/harris_bench.py", "config": "t=16 n=9, S1 frames, k = 1/25",
           "device": torch.cuda.get_device_name(0),
           "kernel_source_sha16": workloads.kernel_source_sha16(), "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0 if all(r["torch_responses_equal"] and r["torch_codes_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
