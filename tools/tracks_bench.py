"""Time the track-set maintenance (fdf_tracks_update_device) on 64 streams of 1920x1080 S1 frames.

Tracks: frame f's detections (t=16 n=9 max-threshold), the best 4 per 64x64 cell (select_device),
followed into frame f + 1 by track_device (3 levels 2:1, r = 10); ids are the indices, ages a
fixed pseudo-random 0..31.  Candidates: detect_device + score_device on frame f + 1.  One update
call serves all 64 streams.

Per min_dist it reports the update alone, the detect + score + pyramid + track step measured in
the same run and the update's share of it, and the same integers written in torch on the device
(what a user can do without the feature: per stream the brute-force pair matrices of the rule, the
passes as masked reductions, a stable sort for the budget, nonzero for the compaction),
alternating with the HIP path in one process; the two results are compared for equality.  Device
events around back-to-back calls, every path warmed first, profiler off.

    python tools/tracks_bench.py [--frames 64] [--calls 50] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NEW = 0x80000000


def torch_suppress(torch, xy, key, state, min_dist, passes):
    n = xy.shape[0]
    dx = xy[:, None, 0] - xy[None, :, 0]
    dy = xy[:, None, 1] - xy[None, :, 1]
    idx = torch.arange(n, device=xy.device)
    dom = (dx * dx + dy * dy < min_dist * min_dist) & (
        (key[None, :] > key[:, None]) | ((key[None, :] == key[:, None]) & (idx[None, :] < idx[:, None])))
    one, two, zero = (torch.full((n,), v, dtype=torch.uint8, device=xy.device) for v in (1, 2, 0))
    for _ in range(passes):
        adm = (dom & (state == 1)[None, :]).any(dim=1)
        und = (dom & (state == 0)[None, :]).any(dim=1)
        state = torch.where(state == 0, torch.where(adm, two, torch.where(und, zero, one)), state)
    return state


def torch_update(torch, q11, status, ids, ages, t_lo, t_hi, cand, scores, c_lo, c_hi, next_id,
                 shape, min_dist, margin, max_tracks, passes):
    """One stream of the rule in torch ops on the device -> (q11, ids, ages, src)."""
    h, w = shape
    q = q11[t_lo:t_hi]
    alive = (status[t_lo:t_hi] != 0) & (q[:, 0] >= margin * 2048) & (q[:, 0] <= (w - 1 - margin) * 2048) \
        & (q[:, 1] >= margin * 2048) & (q[:, 1] <= (h - 1 - margin) * 2048)
    pix = (q + 1024) >> 11
    state = torch.where(alive, 0, 2).to(torch.uint8)
    kept = torch.nonzero(torch_suppress(torch, pix, ages[t_lo:t_hi].long(), state, min_dist,
                                        passes) == 1)[:, 0]
    c = cand[c_lo:c_hi]
    s = scores[c_lo:c_hi].long() & 0xffff
    ok = (c[:, 0] >= margin) & (c[:, 0] <= w - 1 - margin) & (c[:, 1] >= margin) & \
        (c[:, 1] <= h - 1 - margin)
    kp = pix[kept]
    dx = c[:, None, 0] - kp[None, :, 0]
    dy = c[:, None, 1] - kp[None, :, 1]
    blocked = (dx * dx + dy * dy < min_dist * min_dist).any(dim=1)
    state = torch.where(ok & ~blocked, 0, 2).to(torch.uint8)
    adm = torch.nonzero(torch_suppress(torch, c, s, state, min_dist, passes) == 1)[:, 0]
    room = max(0, max_tracks - kept.numel())
    order = torch.sort(65535 - s[adm], stable=True).indices
    new = torch.sort(adm[order[:room]]).values
    out_q = torch.cat([q[kept], c[new] * 2048])
    out_ids = torch.cat([ids[t_lo:t_hi][kept].long(),
                         (next_id + torch.arange(new.numel(), device=q.device)) & 0xffffffff])
    a = ages[t_lo:t_hi][kept].long() & 0xffffffff
    out_ages = torch.cat([torch.clamp(a + 1, max=0xffffffff), torch.zeros_like(new)])
    src = torch.cat([kept + t_lo, (new + c_lo) | NEW])
    return out_q, out_ids, out_ages, src


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
    ap.add_argument("--frames", type=int, default=64, help="streams (frame pairs)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--max-tracks", type=int, default=1500)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--calls", type=int, default=50, help="back-to-back HIP calls per timing")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    W, H, F = args.width, args.height, args.frames
    shape = (H, W)
    cfg = Config(16, 9, NonMaximalSuppression.MaxThreshold)
    frames = workloads.s1_frames_torch(0, F + 1, W, H)
    prev, nxt = frames[:F], frames[1:]
    cap = F * 20_000
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    pts, scores, offs = i32(cap, 2), torch.zeros(cap, dtype=torch.int16, device="cuda"), \
        torch.zeros(F + 1, dtype=torch.int64, device="cuda")
    sel, sel_scores, sel_offs = i32(cap, 2), torch.zeros(cap, dtype=torch.int16, device="cuda"), \
        torch.zeros(F + 1, dtype=torch.int64, device="cuda")
    cand, cand_scores, c_offs = i32(cap, 2), torch.zeros(cap, dtype=torch.int16, device="cuda"), \
        torch.zeros(F + 1, dtype=torch.int64, device="cuda")
    pyr = fast_hip.Pyramid(frames, 3, (2, 1))

    fast_hip.detect_device(prev, cfg, pts, offs)
    fast_hip.score_device(prev, cfg, pts, offs, scores)
    fast_hip.select_device(pts, scores, offs, shape, (64, 64), 4, sel, sel_scores, sel_offs)
    torch.cuda.synchronize()
    n_t = int(sel_offs[-1])
    assert int(offs[-1]) <= cap
    sel = sel[:n_t].contiguous()
    q11, status = i32(n_t, 2), torch.zeros(n_t, dtype=torch.uint8, device="cuda")
    ids = torch.arange(n_t, dtype=torch.int32, device="cuda")
    ages = torch.randint(0, 32, (n_t,), dtype=torch.int32, device="cuda",
                         generator=torch.Generator(device="cuda").manual_seed(1))

    def detect():
        fast_hip.detect_device(nxt, cfg, cand, c_offs)

    def score():
        fast_hip.score_device(nxt, cfg, cand, c_offs, cand_scores)

    def pyramid():
        pyr.build()

    def track():
        fast_hip.track_device(pyr, pyr, sel, sel_offs, q11, status, prev_first=0, next_first=1,
                              n_frames=F)

    for fn in (detect, score, pyramid, track):
        fn()
    torch.cuda.synchronize()
    n_c = int(c_offs[-1])
    assert n_c <= cap
    cand_n, cand_scores_n = cand[:n_c], cand_scores[:n_c]
    t_bounds, c_bounds = sel_offs.cpu().tolist(), c_offs.cpu().tolist()
    out_cap = n_t + F * args.max_tracks
    out_q11, out_ids, out_ages, out_src = i32(out_cap, 2), i32(out_cap), i32(out_cap), i32(out_cap)
    out_offs = torch.zeros(F + 1, dtype=torch.int64, device="cuda")
    next_id = torch.zeros(F, dtype=torch.int32, device="cuda")

    results = []
    for min_dist in (16, 30):
        values = dict(min_dist=min_dist, margin=11, max_tracks=args.max_tracks, passes=args.passes)
        scratch = torch.empty(fast_hip.tracks_scratch_bytes(F, shape, min_dist, n_t, n_c),
                              dtype=torch.uint8, device="cuda")

        def update():
            fast_hip.tracks_update_device(q11, ids, ages, sel_offs, cand_n, cand_scores_n, c_offs,
                                          next_id, out_q11, out_ids, out_ages, out_offs, shape,
                                          track_status=status, out_src=out_src, scratch=scratch,
                                          **values)

        def yardstick():
            ql, cl = q11.long(), cand_n.long()
            return [torch_update(torch, ql, status, ids, ages, t_bounds[f], t_bounds[f + 1], cl,
                                 cand_scores_n, c_bounds[f], c_bounds[f + 1], 7, shape, **values)
                    for f in range(F)]

        next_id.fill_(7)
        update()
        torch.cuda.synchronize()
        want = yardstick()
        total = int(out_offs[-1])
        lens = [len(w[1]) for w in want]
        equal = (out_offs.cpu().tolist() == [sum(lens[:f]) for f in range(F + 1)] and
                 torch.equal(torch.cat([w[0] for w in want]), out_q11[:total].long()) and
                 torch.equal(torch.cat([w[1] for w in want]), out_ids[:total].long() & 0xffffffff) and
                 torch.equal(torch.cat([w[2] for w in want]), out_ages[:total].long() & 0xffffffff) and
                 torch.equal(torch.cat([w[3] for w in want]), out_src[:total].long() & 0xffffffff))
        kept = int(((out_src[:total].long() & NEW) == 0).sum())
        for fn, c in ((detect, 5), (score, 5), (pyramid, 5), (track, 3), (update, 10)):
            timed(torch, fn, c)                                    # warm every path
        ms = {"update": [], "torch": [], "detect": [], "score": [], "pyramid": [], "track": []}
        for _ in range(args.rounds):                               # HIP and torch alternate
            ms["update"].append(timed(torch, update, args.calls))
            ms["torch"].append(timed(torch, yardstick, 1))
            ms["detect"].append(timed(torch, detect, 10))
            ms["score"].append(timed(torch, score, 10))
            ms["pyramid"].append(timed(torch, pyramid, 10))
            ms["track"].append(timed(torch, track, 5))
        med = {name: statistics.median(v) for name, v in ms.items()}
        step = med["detect"] + med["score"] + med["pyramid"] + med["track"]
        results.append({
            "streams": F, "width": W, "height": H, **values, "tracks_in": n_t, "candidates_in": n_c,
            "survivors": kept, "new_tracks": total - kept, "torch_result_equal": bool(equal),
            "update_ms": spread(ms["update"]), "torch_update_ms": spread(ms["torch"]),
            "detect_ms": spread(ms["detect"]), "score_ms": spread(ms["score"]),
            "pyramid_ms": spread(ms["pyramid"]), "track_ms": spread(ms["track"]),
            "step_ms": step, "update_share_of_step": med["update"] / step,
            "torch_over_hip": med["torch"] / med["update"],
            "calls": args.calls, "rounds": args.rounds,
        })
        print(json.dumps(results[-1]), flush=True)
    doc = {"tool": "tools/tracks_bench.py",
           "config": "t=16 n=9 max-threshold, S1 frames; select 64x64 k=4; track 3 levels r=10",
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
