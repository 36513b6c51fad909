"""Time brute-force Hamming matching (fdf_match_device, fdf_match_filter_device) on the
benchmark's own batch: 512 x 1920x1080 S1 frames at t=16 n=9 max-threshold, steered BRIEF
descriptors of the smoothed frames with orient_device's angles, frame f matched against frame
f + 1 through the shifted offsets of one descriptor tensor.

Shapes: (a) select_device's output (cells 64x64, k=4), no window; (b) the same with a window
of +-64 x +-48; (c) all points, no window; (d) one frame pair, all points; (e) shape (a)
forward, reverse and filter (the cross-checked matcher).  Per shape it reports the match step
alone, the detect step measured in the same run and the ratio of the two, and the same
matching written in torch on the device (what a user can do without the feature: the bits
expanded to +-1 half precision, one matrix product per frame pair -- exact for 256 terms --
and topk(2) per row, chunked to fit memory), alternating with the HIP path in one process;
the distances must be equal at the timed size and the indices wherever the best distance is
unique (topk's choice among equal values is not specified).  With --ab-lib a second build of
the library (any libfdf.so, e.g. one of another commit) is timed in the same rounds.
Device events around back-to-back calls, every shape warmed first, profiler off.

    python tools/match_bench.py [--frames 512] [--calls 20] [--rounds 5] [--ab-lib SO] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def expand(torch, desc):
    """(n, 32) uint8 descriptors as (n, 256) half precision, bit set -> -1, clear -> +1."""
    shifts = torch.arange(8, device=desc.device, dtype=torch.int16)
    bits = (desc.to(torch.int16)[:, :, None] >> shifts) & 1
    return (1 - 2 * bits.reshape(desc.shape[0], 256)).to(torch.float16)


def torch_match(torch, desc, pts, ranges, window, out, budget=1 << 25):
    """The matches in torch ops on the device.  `ranges`: per frame pair (q_lo, q_hi, t_lo,
    t_hi), known on the host; `out` = (index int64, distance int32, second int32) tensors
    indexed like the queries.  `budget`: elements of a distance chunk."""
    lo = min(min(r[0], r[2]) for r in ranges)
    hi = max(max(r[1], r[3]) for r in ranges)
    e = expand(torch, desc[lo:hi])
    index, distance, second = out
    for q_lo, q_hi, t_lo, t_hi in ranges:
        n_t = t_hi - t_lo
        if n_t == 0 or q_hi == q_lo:
            continue
        train = e[t_lo - lo:t_hi - lo]
        rows = max(1, budget // n_t)
        for c in range(q_lo, q_hi, rows):
            ce = min(q_hi, c + rows)
            dot = e[c - lo:ce - lo] @ train.T                       # 256 - 2 d, exact in half
            if window is not None:
                near = ((pts[c:ce, None, 0] - pts[None, t_lo:t_hi, 0]).abs() <= window[0]) & \
                       ((pts[c:ce, None, 1] - pts[None, t_lo:t_hi, 1]).abs() <= window[1])
                dot = torch.where(near, dot, torch.full_like(dot, -float("inf")))
            v, i = dot.topk(min(2, n_t), dim=1)
            v = v.float()
            d = torch.where(torch.isinf(v), torch.full_like(v, 0xFFFF), (256 - v) / 2).to(torch.int32)
            index[c:ce] = i[:, 0] + t_lo
            distance[c:ce] = d[:, 0]
            second[c:ce] = d[:, 1] if n_t > 1 else 0xFFFF


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


class OtherBuild:
    """fdf_match_device of another build of the library, on a context of its own."""

    def __init__(self, path, device=0):
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        self.lib = ctypes.CDLL(path)
        self.lib.fdf_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        self.lib.fdf_match_device.argtypes = [vp, u32, vp, vp, u64, vp, vp, vp, u64, vp, u32, u32,
                                              vp, vp]
        self.ctx = vp()
        assert self.lib.fdf_ctx_create(device, ctypes.byref(self.ctx)) == 0

    def match(self, torch, desc, q_offs, t_offs, matches, pts, window):
        rc = self.lib.fdf_match_device(
            self.ctx, q_offs.numel() - 1, desc.data_ptr(), pts.data_ptr() if window else None,
            desc.shape[0], q_offs.data_ptr(), desc.data_ptr(),
            pts.data_ptr() if window else None, desc.shape[0], t_offs.data_ptr(),
            window[0] if window else 0, window[1] if window else 0, matches.data_ptr(),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc


def main(argv=None):
    import torch

    import workloads
    from feature_detector_fast_amd import Config, NonMaximalSuppression, fast_hip

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back HIP calls per timing")
    ap.add_argument("--torch-calls", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ab-lib", default="", help="a second libfdf.so build to time alongside")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    W, H, F = args.width, args.height, args.frames
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    frames = workloads.s1_frames_torch(0, F, W, H)
    smoothed = torch.zeros_like(frames)
    fast_hip.smooth_device(frames, smoothed)
    cap = F * 20_000
    n_bins = 30
    table = torch.from_numpy(fast_hip.brief_steer(fast_hip.brief_pattern(), n_bins)).cuda()
    det_pts = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    det_offs = torch.zeros(F + 1, dtype=torch.int64, device="cuda")

    def detect():
        fast_hip.detect_device(frames, cfg, det_pts, det_offs)

    detect()
    scores = torch.zeros(cap, dtype=torch.int16, device="cuda")
    sel = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    sel_scores = torch.zeros(cap, dtype=torch.int16, device="cuda")
    sel_offs = torch.zeros(F + 1, dtype=torch.int64, device="cuda")
    fast_hip.score_device(frames, cfg, det_pts, det_offs, scores)
    fast_hip.select_device(det_pts, scores, det_offs, (H, W), (64, 64), 4, sel, sel_scores,
                           sel_offs)
    del scores, sel_scores
    sets = {}
    for name, p, o in (("selected", sel, sel_offs), ("all", det_pts.clone(), det_offs.clone())):
        torch.cuda.synchronize()
        n = int(o[-1])
        assert n <= cap, (n, cap)
        p = p[:n].contiguous()                       # detect() rewrites det_pts while timed
        angles = torch.zeros(n, dtype=torch.float32, device="cuda")
        desc = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        fast_hip.orient_device(frames, p, o, angles)
        fast_hip.describe_device(smoothed, p, o, desc, table, n_bins, angles=angles)
        torch.cuda.synchronize()
        sets[name] = (p, o, desc, o.cpu().tolist())
    del smoothed
    torch.cuda.empty_cache()
    other = OtherBuild(args.ab_lib) if args.ab_lib else None

    results = []
    for label, which, pairs, window, cross in (
            ("(a) selected 64x64 k=4, no window", "selected", F - 1, None, False),
            ("(b) selected 64x64 k=4, window 64x48", "selected", F - 1, (64, 48), False),
            ("(c) all points, no window", "all", F - 1, None, False),
            ("(d) one frame pair, all points", "all", 1, None, False),
            ("(e) selected, forward + reverse + filter", "selected", F - 1, None, True)):
        if pairs < 1:
            continue
        pts, offs, desc, h_offs = sets[which]
        n = desc.shape[0]
        q_offs, t_offs = offs[:pairs + 1], offs[1:pairs + 2]
        ranges = [(h_offs[f], h_offs[f + 1], h_offs[f + 1], h_offs[f + 2]) for f in range(pairs)]
        n_q = h_offs[pairs] - h_offs[0]
        pair_count = sum((r[1] - r[0]) * (r[3] - r[2]) for r in ranges)
        matches = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        ab_matches = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        reverse = torch.zeros((n, 2), dtype=torch.int32, device="cuda") if cross else None
        keep = torch.zeros(n, dtype=torch.uint8, device="cuda") if cross else None
        kw = dict(q_points=pts, t_points=pts, window=window) if window else {}

        def match():
            fast_hip.match_device(desc, q_offs, desc, t_offs, matches, **kw)
            if cross:
                fast_hip.match_device(desc, t_offs, desc, q_offs, reverse)
                fast_hip.match_filter_device(matches, q_offs, keep, reverse=reverse, ratio=(3, 4))

        def ab_match():
            other.match(torch, desc, q_offs, t_offs, ab_matches, pts, window)
            if cross:
                other.match(torch, desc, t_offs, q_offs, reverse, pts, None)

        t_out = (torch.zeros(n, dtype=torch.int64, device="cuda"),
                 torch.full((n,), 0xFFFF, dtype=torch.int32, device="cuda"),
                 torch.full((n,), 0xFFFF, dtype=torch.int32, device="cuda"))

        def yardstick():
            torch_match(torch, desc, pts, ranges, window, t_out)
            if cross:
                rev_ranges = [(r[2], r[3], r[0], r[1]) for r in ranges]
                torch_match(torch, desc, pts, rev_ranges, window, t_rev)

        t_rev = tuple(torch.zeros_like(t) for t in t_out) if cross else None
        use_torch = args.torch_calls > 0
        match()
        if use_torch:
            yardstick()
        torch.cuda.synchronize()
        lo, hi = h_offs[0], h_offs[pairs]
        got_d, got_s = matches[lo:hi, 1] & 0xFFFF, (matches[lo:hi, 1] >> 16) & 0xFFFF
        equal = None
        if use_torch:
            equal = bool((got_d == t_out[1][lo:hi]).all() and (got_s == t_out[2][lo:hi]).all() and
                         ((matches[lo:hi, 0].long() == t_out[0][lo:hi]) | (got_d >= got_s)).all())
        ab_equal = None
        if other:
            ab_match()
            torch.cuda.synchronize()
            ab_equal = bool(torch.equal(ab_matches[lo:hi], matches[lo:hi]))
        paths = [("match", match, args.calls), ("detect", detect, max(2, args.calls // 4))]
        if other:
            paths.append(("ab", ab_match, args.calls))
        if use_torch:
            paths.append(("torch", yardstick, args.torch_calls))
        for _, fn, c in paths:
            timed(torch, fn, max(1, c // 2))                       # warm every path
        ms = {name: [] for name, _, _ in paths}
        for _ in range(args.rounds):                               # the paths alternate
            for name, fn, c in paths:
                ms[name].append(timed(torch, fn, c))
        med = {name: statistics.median(v) for name, v in ms.items()}
        row = {
            "shape": label, "frame_pairs": pairs, "width": W, "height": H, "queries": n_q,
            "points_per_frame": n_q / pairs, "pairs": pair_count, "window": window,
            "match_ms": spread(ms["match"]), "detect_ms": spread(ms["detect"]),
            "match_over_detect": med["match"] / med["detect"],
            "ns_per_query": 1e6 * med["match"] / max(n_q, 1),
            "gpairs_per_s": pair_count / med["match"] / 1e6,
            "calls": args.calls, "torch_calls": args.torch_calls, "rounds": args.rounds,
        }
        if cross:
            torch.cuda.synchronize()
            row["kept"] = int(keep[lo:hi].sum())
        if use_torch:
            row.update({"torch_equal": equal, "torch_match_ms": spread(ms["torch"]),
                        "torch_over_hip": med["torch"] / med["match"]})
        if other:
            row.update({"scalar_load_equal": ab_equal, "scalar_load_match_ms": spread(ms["ab"]),
                        "scalar_load_over_lds": med["ab"] / med["match"]})
        results.append(row)
        print(json.dumps(row), flush=True)
        del matches, ab_matches, reverse, keep, t_out, t_rev
        torch.cuda.empty_cache()
    doc = {"tool": "tools/match_bench.py", "config": "t=16 n=9 max-threshold, S1 frames",
           "device": torch.cuda.get_device_name(0),
           "kernel_source_sha16": workloads.kernel_source_sha16(), "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    ok = all(r.get("torch_equal") is not False and r.get("scalar_load_equal") is not False
             for r in results)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
