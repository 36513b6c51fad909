"""Time the pyramidal Lucas-Kanade tracker (fdf_track_device) on device-resident frames: 64 x
1920x1080 S1 frames by default, the points of select_device (cells 64 x 64, k = 4), frame f
tracked into frame f + 1, 3 levels at 2 : 1, r = 10 and r = 5, max_iters 30, eps 20, min_eig 1.
The pyramid build (fdf_pyramid_device) is timed on its own and is not part of the tracker's time.

Two yardsticks run alternating with it in the same process:
  (a) orient_device + describe_device + match_device (window 64 x 48) on the same points: the
      other route to the same correspondences, through code the tracker does not touch (the box
      smoothing the descriptors need is timed on its own, like the pyramid);
  (b) the same integers written in torch on the device, the points of a chunk side by side with
      masked iterations (float64 solve one operation at a time), whose positions and status are
      compared for equality with the tracker's at the timed size.
Device events around back-to-back calls, every path warmed first, profiler off.

    python tools/track_bench.py [--frames 64] [--calls 5] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ONE = 2048


def fdiv(torch, a, b):
    return torch.div(a, b, rounding_mode="floor")


def map_pos(torch, x, len0, lenl):
    return (fdiv(torch, (x + 1024) * (2 * lenl) + len0, 2 * len0) - 1024).clamp(0, (lenl - 1) * ONE)


def map_disp(torch, d, a, b):
    return fdiv(torch, 2 * d * b + a, 2 * a)


def torch_sample(torch, level, base, X, Y, off):
    """S of include/fdf.h for every point (rows) at the window offsets `off` (pixels, 1-D): X, Y
    (N,) int64 positions, `base` (N,) the frame's first byte in the flattened level."""
    _, h, w = level.shape
    flat = level.reshape(-1)
    ix, qx = (X >> 11)[:, None, None] + off[None, None, :], (X & 2047)[:, None, None]
    iy, qy = (Y >> 11)[:, None, None] + off[None, :, None], (Y & 2047)[:, None, None]
    x0, x1 = ix.clamp(0, w - 1), (ix + 1).clamp(0, w - 1)
    y0, y1 = iy.clamp(0, h - 1) * w, (iy + 1).clamp(0, h - 1) * w
    b = base[:, None, None]

    def tap(yy, xx):
        return flat[(b + yy + xx).reshape(-1)].reshape(ix.shape[0], off.numel(), off.numel()).long()

    top = tap(y0, x0) * (ONE - qx) + tap(y0, x1) * qx
    bot = tap(y1, x0) * (ONE - qx) + tap(y1, x1) * qx
    return (top * (ONE - qy) + bot * qy + (1 << 16)) >> 17


def torch_track(torch, levels, strides, fidx, X0, Y0, radius, max_iters, eps, min_eig, chunk=8192):
    """The tracker's rule in torch ops, frame f into frame f + 1 of one batch: `levels` is the
    list of (F, h_l, w_l) uint8 tensors.  Returns (q11 (N, 2) int32, status (N,) uint8, iterations
    (N,) int64); eager torch never fuses a multiply with an add."""
    r, n = radius, (2 * radius + 1) ** 2
    tau = (float(torch.tensor(min_eig, dtype=torch.float32)) * float(n)) * 1048576.0
    dev = X0.device
    N = X0.numel()
    q11 = torch.full((N, 2), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(N, dtype=torch.uint8, device=dev)
    iters_out = torch.zeros(N, dtype=torch.int64, device=dev)
    rim = torch.arange(-r - 1, r + 2, device=dev)
    win = torch.arange(-r, r + 1, device=dev)
    h0, w0 = levels[0].shape[1:]
    for c in range(0, N, chunk):
        f, x0, y0 = fidx[c:c + chunk], X0[c:c + chunk], Y0[c:c + chunk]
        m = x0.numel()
        alive = (x0 >= 0) & (x0 <= (w0 - 1) * ONE) & (y0 >= 0) & (y0 <= (h0 - 1) * ONE)
        dx = torch.zeros(m, dtype=torch.int64, device=dev)
        dy = torch.zeros_like(dx)
        xn, yn = torch.zeros_like(dx), torch.zeros_like(dx)
        iters = torch.zeros_like(dx)
        tmpl = None
        for l in range(len(levels) - 1, -1, -1):
            h, w = levels[l].shape[1:]
            if l < len(levels) - 1:
                hu, wu = levels[l + 1].shape[1:]
                dx, dy = map_disp(torch, dx, wu, w), map_disp(torch, dy, hu, h)
            xp, yp = map_pos(torch, x0.clamp(min=0), w0, w), map_pos(torch, y0.clamp(min=0), h0, h)
            patch = torch_sample(torch, levels[l], f * strides[l], xp, yp, rim)
            s = slice(1, -1)
            gx = 3 * (patch[:, :-2, 2:] - patch[:, :-2, :-2]) + 10 * (patch[:, s, 2:] - patch[:, s, :-2]) \
                + 3 * (patch[:, 2:, 2:] - patch[:, 2:, :-2])
            gy = 3 * (patch[:, 2:, :-2] - patch[:, :-2, :-2]) + 10 * (patch[:, 2:, s] - patch[:, :-2, s]) \
                + 3 * (patch[:, 2:, 2:] - patch[:, :-2, 2:])
            tmpl = patch[:, s, s]
            a11 = (gx * gx).sum((1, 2)).double()
            a12 = (gx * gy).sum((1, 2)).double()
            a22 = (gy * gy).sum((1, 2)).double()
            p, q = a11 - tau, a22 - tau
            usable = (p + q > 0) & (p * q - a12 * a12 > 0)
            if l == 0:
                alive = alive & usable
            det = a11 * a22 - a12 * a12
            go = alive & usable
            xn = torch.where(go, xp + dx, xn)
            yn = torch.where(go, yp + dy, yn)
            inside = (xn >= 0) & (xn <= (w - 1) * ONE) & (yn >= 0) & (yn <= (h - 1) * ONE)
            alive = alive & (inside | ~go)
            run = go & inside
            for _ in range(max_iters):
                if not bool(run.any()):
                    break
                e = torch_sample(torch, levels[l], (f + 1) * strides[l], xn.clamp(min=0),
                                 yn.clamp(min=0), win) - tmpl
                b1 = (e * gx).sum((1, 2)).double()
                b2 = (e * gy).sum((1, 2)).double()
                iters = iters + run.long()
                sx = torch.floor(((a12 * b2 - a22 * b1) / det) * 65536.0 + 0.5)
                sy = torch.floor(((a12 * b1 - a11 * b2) / det) * 65536.0 + 0.5)
                small = (sx.abs() <= 1048576.0) & (sy.abs() <= 1048576.0)
                alive = alive & (small | ~run)
                run = run & small
                fx = torch.where(run, sx, torch.zeros_like(sx)).long()
                fy = torch.where(run, sy, torch.zeros_like(sy)).long()
                xn, yn = xn + fx, yn + fy
                inside = (xn >= 0) & (xn <= (w - 1) * ONE) & (yn >= 0) & (yn <= (h - 1) * ONE)
                alive = alive & (inside | ~run)
                run = run & inside & (fx.abs() + fy.abs() > eps)
            dx = torch.where(go & alive, xn - xp, dx)
            dy = torch.where(go & alive, yn - yp, dy)
        q11[c:c + chunk, 0] = torch.where(alive, xn, torch.full_like(xn, -1)).int()
        q11[c:c + chunk, 1] = torch.where(alive, yn, torch.full_like(yn, -1)).int()
        status[c:c + chunk] = alive.to(torch.uint8)
        iters_out[c:c + chunk] = iters
    return q11, status, iters_out


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
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5, help="back-to-back HIP calls per timing")
    ap.add_argument("--torch-calls", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    if not torch.cuda.is_available():
        print("track_bench: no HIP device is visible; nothing was measured")
        return 0

    import workloads
    from feature_detector_fast_amd import Config, NonMaximalSuppression, fast_hip

    W, H, F, L = args.width, args.height, args.frames, args.levels
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    frames = workloads.s1_frames_torch(0, F, W, H)
    cap = F * 20_000
    det_pts = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    det_offs = torch.zeros(F + 1, dtype=torch.int64, device="cuda")
    fast_hip.detect_device(frames, cfg, det_pts, det_offs)
    scores = torch.zeros(cap, dtype=torch.int16, device="cuda")
    sel = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    sel_scores = torch.zeros(cap, dtype=torch.int16, device="cuda")
    offs = torch.zeros(F + 1, dtype=torch.int64, device="cuda")
    fast_hip.score_device(frames, cfg, det_pts, det_offs, scores)
    fast_hip.select_device(det_pts, scores, det_offs, (H, W), (64, 64), 4, sel, sel_scores, offs)
    torch.cuda.synchronize()
    n_all = int(offs[-1])
    pts = sel[:n_all].contiguous()
    del det_pts, scores, sel, sel_scores
    h_offs = offs.cpu().tolist()
    n = h_offs[F - 1]                                   # the points of the frames that have a next one
    pair_offs = offs[:F].contiguous()

    pyr = fast_hip.Pyramid(frames, L, (2, 1))
    levels = [pyr.level(l) for l in range(L)]
    strides = [lv.shape[1] * lv.shape[2] for lv in levels]
    q11 = torch.zeros((n_all, 2), dtype=torch.int32, device="cuda")
    status = torch.zeros(n_all, dtype=torch.uint8, device="cuda")
    info = torch.zeros(n_all, dtype=torch.int32, device="cuda")

    # yardstick (a): the descriptor route on the same points
    smoothed = torch.zeros_like(frames)
    n_bins = 30
    table = torch.from_numpy(fast_hip.brief_steer(fast_hip.brief_pattern(), n_bins)).cuda()
    angles = torch.zeros(n_all, dtype=torch.float32, device="cuda")
    desc = torch.zeros((n_all, 32), dtype=torch.uint8, device="cuda")
    matches = torch.zeros((n_all, 2), dtype=torch.int32, device="cuda")
    q_offs, t_offs = offs[:F].contiguous(), offs[1:].contiguous()

    def smooth():
        fast_hip.smooth_device(frames, smoothed)

    def descriptor_route():
        fast_hip.orient_device(frames, pts, offs, angles)
        fast_hip.describe_device(smoothed, pts, offs, desc, table, n_bins, angles=angles)
        fast_hip.match_device(desc, q_offs, desc, t_offs, matches, q_points=pts, t_points=pts,
                              window=(64, 48))

    fidx = torch.repeat_interleave(torch.arange(F - 1, device="cuda"),
                                   (offs[1:F] - offs[:F - 1]))
    X0, Y0 = pts[:n, 0].long() * ONE, pts[:n, 1].long() * ONE

    results = []
    for radius in (10, 5):
        values = dict(radius=radius, max_iters=30, eps=20, min_eig=1.0)

        def track():
            fast_hip.track_device(pyr, pyr, pts, pair_offs, q11, status, prev_first=0, next_first=1,
                                  info=info, **values)

        t_res = [None]

        def yardstick():
            t_res[0] = torch_track(torch, levels, strides, fidx, X0, Y0, **values)

        smooth()
        track()
        yardstick()
        torch.cuda.synchronize()
        equal = bool(torch.equal(q11[:n], t_res[0][0]) and torch.equal(status[:n], t_res[0][1]) and
                     torch.equal((info[:n] >> 8).long(), t_res[0][2]))
        iterations = int((info[:n] >> 8).sum())
        tracked = int(status[:n].sum())
        paths = [("track", track, args.calls), ("pyramid", pyr.build, args.calls),
                 ("descriptors", descriptor_route, args.calls), ("smooth", smooth, args.calls),
                 ("torch", yardstick, args.torch_calls)]
        for _, fn, c in paths:
            timed(torch, fn, max(1, c // 2))                       # warm every path
        ms = {name: [] for name, _, _ in paths}
        for _ in range(args.rounds):                               # the paths alternate
            for name, fn, c in paths:
                ms[name].append(timed(torch, fn, c))
        med = {name: statistics.median(v) for name, v in ms.items()}
        row = {
            "radius": radius, "levels": L, "frames": F, "width": W, "height": H, "points": n,
            "points_per_frame": n / (F - 1), "tracked": tracked, "iterations": iterations,
            "iterations_per_point": iterations / max(n, 1), "torch_equal": equal,
            "track_ms": spread(ms["track"]), "pyramid_ms": spread(ms["pyramid"]),
            "descriptors_ms": spread(ms["descriptors"]), "smooth_ms": spread(ms["smooth"]),
            "torch_ms": spread(ms["torch"]),
            "track_over_descriptors": med["track"] / med["descriptors"],
            "torch_over_track": med["torch"] / med["track"],
            "ns_per_point": 1e6 * med["track"] / max(n, 1),
            "point_iterations_per_s": iterations / med["track"] * 1e3,
            "window_samples_per_s": iterations * (2 * radius + 1) ** 2 / med["track"] * 1e3,
            "calls": args.calls, "torch_calls": args.torch_calls, "rounds": args.rounds,
        }
        results.append(row)
        print(json.dumps(row), flush=True)

    doc = {"tool": "tools/track_bench.py",
           "command": f"python tools/track_bench.py --frames {F} --width {W} --height {H} "
                      f"--levels {L} --calls {args.calls} --torch-calls {args.torch_calls} "
                      f"--rounds {args.rounds}",
           "config": "S1 frames, t=16 n=9 max-threshold, select 64x64 k=4, frame f into f + 1, "
                     "2 : 1 levels, max_iters 30, eps 20, min_eig 1",
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
