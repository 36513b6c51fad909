"""Time best-K selection (fdf_select_device) on the benchmark's own batch: 512 x 1920x1080 S1
frames at t=16 n=9 max-threshold, detect_device -> score_device -> select_device.

Per selection shape it reports the selection alone, the detect step measured in the same run
and the selection's share of it, and the same selection written in torch on the device (what
a user can do without the feature: a composite frame/cell/score key, one stable sort, the rank
within each segment, a masked compaction), alternating with the HIP path in one process; the
two results are compared for equality at the timed size.  Device events around back-to-back
calls, every shape warmed first, profiler off.

    python tools/select_bench.py [--frames 512] [--calls 200] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_select(torch, pts, scores, offs, n, shape, cell, k, out, out_scores):
    """The selection in torch ops on the device; `n` (the input total) is known on the host.
    Returns sel_offsets; the kept points land in out / out_scores (n + 1 rows, last = dump)."""
    h, w = shape
    cw, ch = cell[0] or w, cell[1] or h
    cells_x = -(-w // cw)
    ncells = cells_x * -(-h // ch)
    idx = torch.arange(n, device=pts.device)
    frame = torch.searchsorted(offs[1:].contiguous(), idx, right=True)
    x = pts[:n, 0].long()
    y = pts[:n, 1].long()
    seg = frame * ncells + (y // ch) * cells_x + x // cw
    s = scores[:n].long() & 0xffff
    key = (seg << 16) | (65535 - s)
    skey, order = torch.sort(key, stable=True)
    sseg = skey >> 16
    start = torch.ones(n, dtype=torch.bool, device=pts.device)
    start[1:] = sseg[1:] != sseg[:-1]
    first = torch.cummax(torch.where(start, idx, torch.zeros_like(idx)), 0).values
    keep = torch.zeros(n, dtype=torch.bool, device=pts.device)
    keep[order] = (idx - first) < k
    incl = torch.cumsum(keep, 0)
    dest = torch.where(keep, incl - 1, torch.full_like(incl, n))
    out[dest] = pts[:n]
    out_scores[dest] = scores[:n]
    kept_before = torch.cat([incl.new_zeros(1), incl])
    return kept_before[offs.clamp(max=n)]


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
    ap.add_argument("--calls", type=int, default=200, help="back-to-back HIP calls per timing")
    ap.add_argument("--torch-calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    W, H = args.width, args.height
    shape = (H, W)
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    all_frames = workloads.s1_frames_torch(0, args.frames, W, H)
    results = []
    for label, nf, cell, k in (("batch cells 64x64 k=4", args.frames, (64, 64), 4),
                               ("batch whole frame k=1000", args.frames, (0, 0), 1000),
                               ("single frame cells 64x64 k=4", 1, (64, 64), 4),
                               ("single frame whole frame k=1000", 1, (0, 0), 1000)):
        frames = all_frames[:nf]
        cap = nf * 20_000
        pts = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
        scores = torch.zeros(cap, dtype=torch.int16, device="cuda")
        offs = torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
        sel = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
        sel_scores = torch.zeros(cap, dtype=torch.int16, device="cuda")
        sel_offs = torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
        scratch = torch.empty(fast_hip.select_scratch_bytes(nf, shape, cell, cap),
                              dtype=torch.uint8, device="cuda")

        def detect():
            fast_hip.detect_device(frames, cfg, pts, offs)

        def score():
            fast_hip.score_device(frames, cfg, pts, offs, scores)

        def select():
            fast_hip.select_device(pts, scores, offs, shape, cell, k, sel, sel_scores, sel_offs,
                                   scratch=scratch)

        def chain():
            detect()
            score()
            select()

        chain()
        torch.cuda.synchronize()
        n = int(offs[-1])
        assert n <= cap, (n, cap)
        t_out = torch.zeros((n + 1, 2), dtype=torch.int32, device="cuda")
        t_scores = torch.zeros(n + 1, dtype=torch.int16, device="cuda")

        def yardstick():
            return torch_select(torch, pts, scores, offs, n, shape, cell, k, t_out, t_scores)

        t_offs = yardstick()
        torch.cuda.synchronize()
        kept = int(sel_offs[-1])
        equal = bool(torch.equal(t_offs, sel_offs) and torch.equal(t_out[:kept], sel[:kept]) and
                     torch.equal(t_scores[:kept], sel_scores[:kept]))
        for fn, c in ((detect, 20), (score, 20), (select, 20), (chain, 20), (yardstick, 3)):
            timed(torch, fn, c)                                    # warm every path
        ms = {"detect": [], "score": [], "select": [], "chain": [], "torch": []}
        for _ in range(args.rounds):                               # HIP and torch alternate
            ms["select"].append(timed(torch, select, args.calls))
            ms["torch"].append(timed(torch, yardstick, args.torch_calls))
            ms["detect"].append(timed(torch, detect, args.calls))
            ms["score"].append(timed(torch, score, args.calls))
            ms["chain"].append(timed(torch, chain, args.calls))
        med = {name: statistics.median(v) for name, v in ms.items()}
        results.append({
            "shape": label, "frames": nf, "width": W, "height": H, "cell": list(cell), "k": k,
            "points_in": n, "points_kept": kept, "torch_result_equal": equal,
            "select_ms": spread(ms["select"]), "detect_ms": spread(ms["detect"]),
            "score_ms": spread(ms["score"]), "chain_ms": spread(ms["chain"]),
            "torch_select_ms": spread(ms["torch"]),
            "select_share_of_detect": med["select"] / med["detect"],
            "torch_over_hip": med["torch"] / med["select"],
            "calls": args.calls, "torch_calls": args.torch_calls, "rounds": args.rounds,
        })
        print(json.dumps(results[-1]), flush=True)
    doc = {"tool": "tools/select_bench.py", "config": "t=16 n=9 max-threshold, S1 frames",
           "device": torch.cuda.get_device_name(0),
           "kernel_source_sha16": workloads.kernel_source_sha16(), "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0 if all(r["torch_result_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
