"""Time the exact bilinear resize (fdf_resize_device) and the scale pyramid
(fdf_pyramid_device) on the benchmark's own batch: 512 x 1920x1080 S1 frames.

Three shapes: the batch to one level (1600 x 900), the 8-level 6 / 5 pyramid of the batch and
the 8 levels of one frame.  Each is timed beside two yardsticks that run alternating with it in
the same process: the same integer arithmetic written in torch on the device (index_select of
the two tap columns and rows, int32 products, one shift; what a user can do without the
feature), whose result is compared for equality at the timed size, and a plain device copy of
as many bytes as the kernel reads plus writes (the traffic yardstick).  Device events around
back-to-back calls, every shape warmed first, profiler off.

    python tools/pyramid_bench.py [--frames 512] [--calls 20] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def split_taps(torch, table, src_len, device):
    """(i0, i1, w0, w1) of a resize_taps table as device tensors."""
    t = torch.from_numpy(table.astype("int64")).to(device)
    i0 = t >> 12
    q = (t & 0xfff).to(torch.int32)
    return i0, (i0 + 1).clamp_(max=src_len - 1), 2048 - q, q


def torch_resize(torch, src, out, xt, yt, chunk=16):
    """The resize in torch ops on the device, `chunk` frames at a time: rows first (two
    index_selects, no arithmetic yet), then columns, all products in int32."""
    x0, x1, wx0, wx1 = xt
    y0, y1, wy0, wy1 = yt
    wy0, wy1 = wy0[None, :, None], wy1[None, :, None]
    for c in range(0, src.shape[0], chunk):
        s = src[c:c + chunk]
        top = s.index_select(1, y0)
        bot = s.index_select(1, y1)
        h_top = top.index_select(2, x0).to(torch.int32) * wx0 + top.index_select(2, x1).to(torch.int32) * wx1
        h_bot = bot.index_select(2, x0).to(torch.int32) * wx0 + bot.index_select(2, x1).to(torch.int32) * wx1
        out[c:c + chunk] = ((h_top * wy0 + h_bot * wy1 + (1 << 21)) >> 22).to(torch.uint8)


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
    from feature_detector_fast_amd import fast_hip

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back HIP calls per timing")
    ap.add_argument("--torch-calls", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    W, H = args.width, args.height
    dev = torch.device("cuda", 0)
    all_frames = workloads.s1_frames_torch(0, args.frames, W, H)
    results = []

    for label, nf, n_levels in (("batch to one level", args.frames, 2),
                                (f"batch pyramid {args.levels} levels", args.frames, args.levels),
                                (f"single frame pyramid {args.levels} levels", 1, args.levels)):
        frames = all_frames[:nf]
        pyr = fast_hip.Pyramid(frames, n_levels, (6, 5), build=False)
        plan = pyr.plan
        sizes = [(L.width, L.height) for L in plan.levels]
        # the torch yardstick's own pyramid and taps
        t_levels = [frames] + [torch.zeros((nf, h, w), dtype=torch.uint8, device=dev)
                               for w, h in sizes[1:]]
        t_taps = [(split_taps(torch, fast_hip.resize_taps(sizes[l - 1][0], sizes[l][0]),
                              sizes[l - 1][0], dev),
                   split_taps(torch, fast_hip.resize_taps(sizes[l - 1][1], sizes[l][1]),
                              sizes[l - 1][1], dev)) for l in range(1, n_levels)]
        # the copy yardstick: the bytes every level's resize reads plus writes, once each way
        moved = sum(nf * (sizes[l - 1][0] * sizes[l - 1][1] + sizes[l][0] * sizes[l][1])
                    for l in range(1, n_levels))
        c_src = torch.zeros(moved // 2, dtype=torch.uint8, device=dev)
        c_dst = torch.zeros_like(c_src)

        def hip():
            pyr.build()

        def yardstick():
            for l in range(1, n_levels):
                torch_resize(torch, t_levels[l - 1], t_levels[l], *t_taps[l - 1])

        def copy():
            c_dst.copy_(c_src)

        hip()
        yardstick()
        torch.cuda.synchronize()
        equal = all(bool(torch.equal(pyr.level(l), t_levels[l])) for l in range(1, n_levels))
        for fn, c in ((hip, 5), (copy, 5), (yardstick, 1)):
            timed(torch, fn, c)                                    # warm every path
        ms = {"hip": [], "copy": [], "torch": []}
        for _ in range(args.rounds):                               # HIP and torch alternate
            ms["hip"].append(timed(torch, hip, args.calls))
            ms["torch"].append(timed(torch, yardstick, args.torch_calls))
            ms["copy"].append(timed(torch, copy, args.calls))
        med = {name: statistics.median(v) for name, v in ms.items()}
        results.append({
            "shape": label, "frames": nf, "width": W, "height": H, "levels": n_levels,
            "sizes": sizes, "torch_equal": equal, "bytes_read_plus_written": moved,
            "hip_ms": spread(ms["hip"]), "copy_ms": spread(ms["copy"]),
            "torch_ms": spread(ms["torch"]), "hip_over_copy": med["hip"] / med["copy"],
            "torch_over_hip": med["torch"] / med["hip"],
            "hip_tb_per_s": moved / 1e9 / med["hip"], "copy_tb_per_s": moved / 1e9 / med["copy"],
            "calls": args.calls, "torch_calls": args.torch_calls, "rounds": args.rounds,
        })
        print(json.dumps(results[-1]), flush=True)
        del pyr, t_levels, t_taps, c_src, c_dst
        torch.cuda.empty_cache()

    doc = {"tool": "tools/pyramid_bench.py", "config": "S1 frames, factor 6 / 5",
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
