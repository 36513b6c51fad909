"""Time the exact bilinear warp (fdf_warp_device) on device-resident frames: 64 x 1920x1080 S1
frames by default, one model for the whole batch, four models (the identity, a 1 degree
rotation about the centre, a mild homography, a 30 degree rotation), each with and without the
mask, replicate border.

Two yardsticks run alternating with it in the same process:
  (a) fdf_resize_device 1920 x 1080 -> 1920 x 1080 on the same buffers: the same bytes moved
      through code the warp does not touch (an identity resize: every pixel read and written
      once);
  (b) the same integers written in torch on the device (float64 positions one operation at a
      time, four gathers, int32 products, one shift), whose result is compared for equality at
      the timed size.
Device events around back-to-back calls, every path warmed first, profiler off.

    python tools/warp_bench.py [--frames 64] [--calls 10] [--rounds 5] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rotation(w, h, degrees):
    a = math.radians(degrees)
    c, s = math.cos(a), math.sin(a)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    return [c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy, 0.0, 0.0, 1.0]


def models_of(w, h):
    return [("identity", [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]),
            ("rotation 1 deg", rotation(w, h, 1.0)),
            ("mild homography", [1.02, 0.01, -12.5, -0.015, 0.99, 9.25, 2e-5, -1e-5, 1.0]),
            ("rotation 30 deg", rotation(w, h, 30.0))]


def torch_warp(torch, src, h, out, mask, fill=0, chunk=8):
    """include/fdf.h's warp rule in torch ops on the device (replicate border), `chunk` frames at a
    time; eager torch never fuses a multiply with an add."""
    _, sh, sw = src.shape
    _, dh, dw = out.shape
    dev = src.device
    x = torch.arange(dw, dtype=torch.float64, device=dev)[None, :]
    y = torch.arange(dh, dtype=torch.float64, device=dev)[:, None]
    p = (h[0] * x + h[1] * y) + h[2]
    q = (h[3] * x + h[4] * y) + h[5]
    w = (h[6] * x + h[7] * y) + h[8]
    fx = torch.floor((p / w) * 2048.0 + 0.5)
    fy = torch.floor((q / w) * 2048.0 + 0.5)
    lim = float(1 << 30)
    valid = (w > 0) & (fx >= -lim) & (fx <= lim) & (fy >= -lim) & (fy <= lim)
    valid = valid.expand(dh, dw)
    X = torch.where(valid, fx, torch.zeros_like(fx)).to(torch.int64)
    Y = torch.where(valid, fy, torch.zeros_like(fy)).to(torch.int64)
    ix, qx = X >> 11, (X & 2047).to(torch.int32)
    iy, qy = Y >> 11, (Y & 2047).to(torch.int32)
    x0, x1 = ix.clamp(0, sw - 1), (ix + 1).clamp(0, sw - 1)
    y0, y1 = iy.clamp(0, sh - 1), (iy + 1).clamp(0, sh - 1)
    i00, i10, i01, i11 = (y0 * sw + x0).reshape(-1), (y0 * sw + x1).reshape(-1), \
        (y1 * sw + x0).reshape(-1), (y1 * sw + x1).reshape(-1)
    wx0, wx1, wy0, wy1 = 2048 - qx, qx, 2048 - qy, qy
    inside = valid & (X >= 0) & (X <= (sw - 1) * 2048) & (Y >= 0) & (Y <= (sh - 1) * 2048)
    for c in range(0, src.shape[0], chunk):
        s = src[c:c + chunk].reshape(-1, sh * sw)
        n = s.shape[0]

        def tap(i):
            return s.index_select(1, i).reshape(n, dh, dw).to(torch.int32)

        top = tap(i00) * wx0 + tap(i10) * wx1
        bot = tap(i01) * wx0 + tap(i11) * wx1
        v = (top * wy0 + bot * wy1 + (1 << 21)) >> 22
        out[c:c + chunk] = torch.where(valid, v, torch.full_like(v, fill)).to(torch.uint8)
        if mask is not None:
            mask[c:c + chunk] = inside.to(torch.uint8)


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

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=10, help="back-to-back HIP calls per timing")
    ap.add_argument("--torch-calls", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    if not torch.cuda.is_available():
        print("warp_bench: no HIP device is visible; nothing was measured")
        return 0

    import workloads
    from feature_detector_fast_amd import fast_hip

    W, H, F = args.width, args.height, args.frames
    dev = torch.device("cuda", 0)
    frames = workloads.s1_frames_torch(0, F, W, H)
    out = torch.zeros_like(frames)
    mask = torch.zeros_like(frames)
    t_out = torch.zeros_like(frames)
    t_mask = torch.zeros_like(frames)
    xt = torch.from_numpy(fast_hip.resize_taps(W, W).view("int32")).to(dev)
    yt = torch.from_numpy(fast_hip.resize_taps(H, H).view("int32")).to(dev)

    def resize():
        fast_hip.resize_device(frames, out, xt, yt)

    results = []
    for label, h in models_of(W, H):
        models = torch.tensor([h] * F, dtype=torch.float64, device=dev)

        def hip():
            fast_hip.warp_device(frames, models, out)

        def hip_mask():
            fast_hip.warp_device(frames, models, out, mask=mask)

        def yardstick():
            torch_warp(torch, frames, h, t_out, t_mask)

        hip_mask()
        yardstick()
        torch.cuda.synchronize()
        equal = bool(torch.equal(out, t_out)) and bool(torch.equal(mask, t_mask))
        hip()
        torch.cuda.synchronize()
        equal = equal and bool(torch.equal(out, t_out))
        inside = float(mask.to(torch.float32).mean())
        for fn, c in ((hip, 3), (hip_mask, 3), (resize, 3), (yardstick, 1)):
            timed(torch, fn, c)                                    # warm every path
        ms = {"warp": [], "warp_mask": [], "resize": [], "torch": []}
        for _ in range(args.rounds):                               # the paths alternate
            ms["warp"].append(timed(torch, hip, args.calls))
            ms["resize"].append(timed(torch, resize, args.calls))
            ms["warp_mask"].append(timed(torch, hip_mask, args.calls))
            ms["torch"].append(timed(torch, yardstick, args.torch_calls))
        med = {name: statistics.median(v) for name, v in ms.items()}
        pixels = F * W * H
        results.append({
            "model": label, "h": h, "frames": F, "width": W, "height": H, "torch_equal": equal,
            "inside_fraction": inside,
            "warp_ms": spread(ms["warp"]), "warp_mask_ms": spread(ms["warp_mask"]),
            "resize_ms": spread(ms["resize"]), "torch_ms": spread(ms["torch"]),
            "warp_over_resize": med["warp"] / med["resize"],
            "warp_mask_over_resize": med["warp_mask"] / med["resize"],
            "torch_over_warp_mask": med["torch"] / med["warp_mask"],
            "warp_gpixels_per_s": pixels / 1e6 / med["warp"],
            "calls": args.calls, "torch_calls": args.torch_calls, "rounds": args.rounds,
        })
        print(json.dumps(results[-1]), flush=True)

    doc = {"tool": "tools/warp_bench.py",
           "command": f"python tools/warp_bench.py --frames {F} --width {W} --height {H} "
                      f"--calls {args.calls} --torch-calls {args.torch_calls} "
                      f"--rounds {args.rounds}",
           "config": "S1 frames, replicate border, one model for the batch",
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
